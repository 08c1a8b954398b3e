// The planning step of bsx_resize_surfaces_batch: the call's items checked and ordered into the ragged grid of its one launch.  Plain C++ on host memory — no HIP
// type, no context — so a stand-alone program can drive it (tests/test_resize_surfaces_host.py does, under the host sanitizers).
//   in:   the n items, the context's n_streams;
//   out:  the refusals that concern the call's n and items, an item alone or two items together (the text names items[i] and the value), or the plan:
//           cls      the destination-size class of every item: the distinct (dw, dh) pairs numbered in the order of their first item, at most kRsMaxSizes =
//                    BSX_MAX_GEOMS.  Source sizes are not counted: a class holds items of any mix of them;
//           order    the items ordered by class (a counting sort on cls: stable): position q of the call is items[order[q]];
//           pos, wg, per   kernels.hpp's GeomSpans: class g owns positions [pos[g], pos[g + 1]) and workgroups [wg[g], wg[g + 1]) of the grid, per[g] =
//                    ceil(ceil(dw / 4) * dh / 256): a lane makes four adjacent pixels of one output row, 256 lanes to a workgroup.
// A destination may overlap no item's plane (its own included) and no other destination; planes may overlap each other — two items may name one surface.  The
// extent a plane is judged on is vcam_nv12_extent: it ends at byte sw of its last row, so a destination may lie in the padding [sw, pitch) of another surface's last
// row.  No plane the plan accepts extends over 2^31 bytes or more, and no destination: the kernel's offsets into them are 32-bit.
#pragma once
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/bsx.h"
#include "geoms_request.hpp"

namespace bsx {
constexpr int kRsMaxSizes = BSX_MAX_GEOMS;
constexpr int kRsLanePixels = 4, kRsThreads = 256;      // resize_surfaces_k: pixels per lane, lanes per workgroup (kernels_img.hip)

struct ResizeSurfacesPlan {
  enum { kOk = 0, kRefused = 1, kTooLarge = 2 };
  std::vector<int> cls;                      // cls[i] = the destination-size class of items[i]
  std::vector<int> order;                    // order[q] = the item at position q
  std::vector<Span> spans;                   // scratch of the overlap sweep: Span::item = 2 i for the Y plane of items[i], 2 i + 1 for its UV plane, i for its destination
  int sizes[kRsMaxSizes][2] = {};
  int n_sizes = 0;
  int pos[kRsMaxSizes + 1] = {}, wg[kRsMaxSizes + 1] = {}, per[kRsMaxSizes] = {};
  int bad = -1;                              // kRefused: the item the text names (-1: the call's n or items)
  char text[240] = {0};
};

// kOk; kRefused with plan->text and plan->bad; kTooLarge where the grid would have 2^31 workgroups or more
inline int resize_surfaces_plan(const bsx_resize_surface_item* items, int n, int n_streams, ResizeSurfacesPlan* plan) {
  ResizeSurfacesPlan& p = *plan;
  p = ResizeSurfacesPlan{};
#define BSX_RS_REFUSE(i, ...) do { p.bad = (i); snprintf(p.text, sizeof p.text, __VA_ARGS__); return ResizeSurfacesPlan::kRefused; } while (0)
  if (n < 0) BSX_RS_REFUSE(-1, "n = %d is negative", n);
  if (n > n_streams) BSX_RS_REFUSE(-1, "n = %d exceeds the context's %d streams", n, n_streams);
  if (n == 0) return ResizeSurfacesPlan::kOk;
  if (!items) BSX_RS_REFUSE(-1, "items is NULL");
  p.cls.assign((size_t)n, 0);
  long count[kRsMaxSizes] = {0};
  constexpr size_t kLimit = (size_t)1 << 31;
  for (int i = 0; i < n; i++) {
    const bsx_resize_surface_item& it = items[i];
    if (!it.d_y) BSX_RS_REFUSE(i, "items[%d]: d_y is NULL", i);
    if (!it.d_uv) BSX_RS_REFUSE(i, "items[%d]: d_uv is NULL", i);
    if (!it.d_dst) BSX_RS_REFUSE(i, "items[%d]: d_dst is NULL", i);
    if ((uintptr_t)it.d_y & 3) BSX_RS_REFUSE(i, "items[%d]: d_y %p is not 4-byte aligned", i, (const void*)it.d_y);
    if ((uintptr_t)it.d_uv & 3) BSX_RS_REFUSE(i, "items[%d]: d_uv %p is not 4-byte aligned", i, (const void*)it.d_uv);
    if (it.sw <= 0 || it.sh <= 0) BSX_RS_REFUSE(i, "items[%d]: source size %d x %d is not positive", i, it.sw, it.sh);
    if ((it.sw | it.sh) & 1) BSX_RS_REFUSE(i, "items[%d]: NV12 needs an even width and height (%d x %d)", i, it.sw, it.sh);
    if (it.pitch_y < it.sw) BSX_RS_REFUSE(i, "items[%d]: pitch_y = %d is below sw = %d", i, it.pitch_y, it.sw);
    if (it.pitch_y & 3) BSX_RS_REFUSE(i, "items[%d]: pitch_y = %d is not a multiple of 4", i, it.pitch_y);
    if (it.pitch_uv < it.sw) BSX_RS_REFUSE(i, "items[%d]: pitch_uv = %d is below sw = %d", i, it.pitch_uv, it.sw);
    if (it.pitch_uv & 3) BSX_RS_REFUSE(i, "items[%d]: pitch_uv = %d is not a multiple of 4", i, it.pitch_uv);
    if (it.dw <= 0 || it.dh <= 0) BSX_RS_REFUSE(i, "items[%d]: output size %d x %d is not positive", i, it.dw, it.dh);
    if (it.flags) BSX_RS_REFUSE(i, "items[%d]: flags 0x%x: this call takes no flags", i, it.flags);
    if (it.reserved) BSX_RS_REFUSE(i, "items[%d]: reserved = %d is not 0", i, it.reserved);
    if (vcam_nv12_extent(it.pitch_y, it.sh, it.sw) >= kLimit)
      BSX_RS_REFUSE(i, "items[%d]: the Y plane (%d rows of pitch_y = %d) extends over 2 GiB or more", i, it.sh, it.pitch_y);
    if (vcam_nv12_extent(it.pitch_uv, it.sh / 2, it.sw) >= kLimit)
      BSX_RS_REFUSE(i, "items[%d]: the UV plane (%d rows of pitch_uv = %d) extends over 2 GiB or more", i, it.sh / 2, it.pitch_uv);
    if ((size_t)it.dw * (size_t)it.dh * 3 >= kLimit)
      BSX_RS_REFUSE(i, "items[%d]: output size %d x %d is beyond the kernel's 32-bit offsets (dw * dh * 3 < 2^31)", i, it.dw, it.dh);
    int g = 0;
    while (g < p.n_sizes && (p.sizes[g][0] != it.dw || p.sizes[g][1] != it.dh)) g++;
    if (g == p.n_sizes) {
      if (g == kRsMaxSizes) BSX_RS_REFUSE(i, "items[%d]: %d x %d is distinct output size %d of the call (at most %d)", i, it.dw, it.dh, g + 1, kRsMaxSizes);
      p.sizes[g][0] = it.dw; p.sizes[g][1] = it.dh; p.n_sizes++;
    }
    p.cls[(size_t)i] = g;
    count[g]++;
  }
  std::vector<Span>& sp = p.spans;
  sp.reserve(3 * (size_t)n);
  for (int i = 0; i < n; i++) {
    const bsx_resize_surface_item& it = items[i];
    sp.push_back({(uintptr_t)it.d_y, (uintptr_t)it.d_y + vcam_nv12_extent(it.pitch_y, it.sh, it.sw), 2 * i, false});
    sp.push_back({(uintptr_t)it.d_uv, (uintptr_t)it.d_uv + vcam_nv12_extent(it.pitch_uv, it.sh / 2, it.sw), 2 * i + 1, false});
    sp.push_back({(uintptr_t)it.d_dst, (uintptr_t)it.d_dst + (size_t)it.dw * (size_t)it.dh * 3, i, true});
  }
  const Span* d = nullptr;
  const Span* o = nullptr;
  if (spans_overlap(sp, &d, &o))
    BSX_RS_REFUSE(d->item, "items[%d]: d_dst %p overlaps the %s of items[%d] (%p)", d->item, (const void*)d->begin,
                  o->dst ? "destination" : (o->item & 1) ? "UV plane" : "Y plane", o->dst ? o->item : o->item >> 1, (const void*)o->begin);
#undef BSX_RS_REFUSE
  long wg = 0;
  for (int g = 0; g < kRsMaxSizes; g++) {
    const bool live = g < p.n_sizes;
    const long groups = live ? (((long)p.sizes[g][0] + kRsLanePixels - 1) / kRsLanePixels) * (long)p.sizes[g][1] : 0;
    const long per = (groups + kRsThreads - 1) / kRsThreads;
    if (wg + count[g] * per >= (1l << 31)) return ResizeSurfacesPlan::kTooLarge;
    wg += count[g] * per;
    p.pos[g + 1] = p.pos[g] + (int)count[g];
    p.wg[g + 1] = (int)wg;
    p.per[g] = (int)per;
  }
  p.order.assign((size_t)n, 0);
  int next[kRsMaxSizes];
  for (int g = 0; g < kRsMaxSizes; g++) next[g] = p.pos[g];
  for (int i = 0; i < n; i++) p.order[(size_t)next[p.cls[(size_t)i]]++] = i;
  return ResizeSurfacesPlan::kOk;
}
}  // namespace bsx
