// The planning step of bsx_gaussian_blur_surfaces_batch: the call's items checked and ordered into the ragged grid of its one launch.  Plain C++ on host memory — no
// HIP type, no context — so a stand-alone program can drive it (tests/test_blur_surfaces_host.py does, under the host sanitizers).
//   in:   the n items, the context's n_streams;
//   out:  the refusals that concern the call's n and items or an item alone (the text names items[i] and the value), or the plan:
//           cls      the size class of every item: the distinct (w, h) pairs numbered in the order of their first item, at most kBsMaxSizes = BSX_MAX_GEOMS;
//           pos, wg, per   kernels.hpp's GeomSpans: class g owns positions [pos[g], pos[g + 1]) of the call ordered by class (a counting sort on cls: stable) and
//                    workgroups [wg[g], wg[g + 1]) of the grid, per[g] = the 64 x 16 tiles of one surface of the class;
//           ntx      kernels.hpp's BlurTileCols: tiles per row of a surface of class g.
// Overlaps are not judged here (bsx_api.hip: spans_overlap), but the extent a plane is judged on is vcam_nv12_extent, and no plane the plan accepts extends over
// 2^31 bytes or more: the kernel's offsets into a plane are 32-bit.
#pragma once
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/bsx.h"
#include "vcam_nv12_plan.hpp"

namespace bsx {
constexpr int kBsMaxSizes = BSX_MAX_GEOMS;
constexpr int kBsTileW = 64, kBsTileH = 16;      // the blur's output tile (kernels_img.hip: kGTW x kGTH)

struct BlurSurfacesPlan {
  enum { kOk = 0, kRefused = 1, kTooLarge = 2 };
  std::vector<int> cls;                      // cls[i] = the size class of items[i]
  int sizes[kBsMaxSizes][2] = {};
  int n_sizes = 0;
  int pos[kBsMaxSizes + 1] = {}, wg[kBsMaxSizes + 1] = {}, per[kBsMaxSizes] = {}, ntx[kBsMaxSizes] = {};
  int bad = -1;                              // kRefused: the item the text names (-1: the call's n or items)
  char text[200] = {0};
};

// kOk; kRefused with plan->text and plan->bad; kTooLarge where the grid would have 2^31 workgroups or more
inline int blur_surfaces_plan(const bsx_blur_surface_item* items, int n, int n_streams, BlurSurfacesPlan* plan) {
  BlurSurfacesPlan& p = *plan;
  p = BlurSurfacesPlan{};
#define BSX_BS_REFUSE(i, ...) do { p.bad = (i); snprintf(p.text, sizeof p.text, __VA_ARGS__); return BlurSurfacesPlan::kRefused; } while (0)
  if (n < 0) BSX_BS_REFUSE(-1, "n = %d is negative", n);
  if (n > n_streams) BSX_BS_REFUSE(-1, "n = %d exceeds the context's %d streams", n, n_streams);
  if (n == 0) return BlurSurfacesPlan::kOk;
  if (!items) BSX_BS_REFUSE(-1, "items is NULL");
  p.cls.assign((size_t)n, 0);
  long count[kBsMaxSizes] = {0};
  constexpr size_t kLimit = (size_t)1 << 31;
  for (int i = 0; i < n; i++) {
    const bsx_blur_surface_item& it = items[i];
    if (it.w <= 0 || it.h <= 0) BSX_BS_REFUSE(i, "items[%d]: size %d x %d is not positive", i, it.w, it.h);
    if ((it.w | it.h) & 1) BSX_BS_REFUSE(i, "items[%d]: NV12 needs an even width and height (%d x %d)", i, it.w, it.h);
    if (it.ksize < 1 || it.ksize > 31 || !(it.ksize & 1)) BSX_BS_REFUSE(i, "items[%d]: ksize %d is not an odd number of 1 .. 31", i, it.ksize);
    if (!it.d_y) BSX_BS_REFUSE(i, "items[%d]: d_y is NULL", i);
    if (!it.d_uv) BSX_BS_REFUSE(i, "items[%d]: d_uv is NULL", i);
    if (!it.d_dst) BSX_BS_REFUSE(i, "items[%d]: d_dst is NULL", i);
    if ((uintptr_t)it.d_y & 3) BSX_BS_REFUSE(i, "items[%d]: d_y %p is not 4-byte aligned", i, (const void*)it.d_y);
    if ((uintptr_t)it.d_uv & 3) BSX_BS_REFUSE(i, "items[%d]: d_uv %p is not 4-byte aligned", i, (const void*)it.d_uv);
    if (it.pitch_y < it.w) BSX_BS_REFUSE(i, "items[%d]: pitch_y = %d is below w = %d", i, it.pitch_y, it.w);
    if (it.pitch_y & 3) BSX_BS_REFUSE(i, "items[%d]: pitch_y = %d is not a multiple of 4", i, it.pitch_y);
    if (it.pitch_uv < it.w) BSX_BS_REFUSE(i, "items[%d]: pitch_uv = %d is below w = %d", i, it.pitch_uv, it.w);
    if (it.pitch_uv & 3) BSX_BS_REFUSE(i, "items[%d]: pitch_uv = %d is not a multiple of 4", i, it.pitch_uv);
    if (it.flags) BSX_BS_REFUSE(i, "items[%d]: flags 0x%x: this call takes no flags", i, it.flags);
    if ((size_t)it.w * (size_t)it.h * 3 >= kLimit)
      BSX_BS_REFUSE(i, "items[%d]: size %d x %d is beyond the kernel's 32-bit offsets (w * h * 3 < 2^31)", i, it.w, it.h);
    if (vcam_nv12_extent(it.pitch_y, it.h, it.w) >= kLimit)
      BSX_BS_REFUSE(i, "items[%d]: the Y plane (%d rows of pitch_y = %d) extends over 2 GiB or more", i, it.h, it.pitch_y);
    if (vcam_nv12_extent(it.pitch_uv, it.h / 2, it.w) >= kLimit)
      BSX_BS_REFUSE(i, "items[%d]: the UV plane (%d rows of pitch_uv = %d) extends over 2 GiB or more", i, it.h / 2, it.pitch_uv);
    int g = 0;
    while (g < p.n_sizes && (p.sizes[g][0] != it.w || p.sizes[g][1] != it.h)) g++;
    if (g == p.n_sizes) {
      if (g == kBsMaxSizes) BSX_BS_REFUSE(i, "items[%d]: %d x %d is distinct size %d of the call (at most %d)", i, it.w, it.h, g + 1, kBsMaxSizes);
      p.sizes[g][0] = it.w; p.sizes[g][1] = it.h; p.n_sizes++;
    }
    p.cls[(size_t)i] = g;
    count[g]++;
  }
#undef BSX_BS_REFUSE
  long wg = 0;
  for (int g = 0; g < kBsMaxSizes; g++) {
    const bool live = g < p.n_sizes;
    const long ntx = live ? ((long)p.sizes[g][0] + kBsTileW - 1) / kBsTileW : 0;
    const long per = live ? ntx * (((long)p.sizes[g][1] + kBsTileH - 1) / kBsTileH) : 0;
    if (per >= (1l << 31) || wg + count[g] * per >= (1l << 31)) return BlurSurfacesPlan::kTooLarge;
    wg += count[g] * per;
    p.pos[g + 1] = p.pos[g] + (int)count[g];
    p.wg[g + 1] = (int)wg;
    p.per[g] = (int)per;
    p.ntx[g] = (int)ntx;
  }
  return BlurSurfacesPlan::kOk;
}
}  // namespace bsx
