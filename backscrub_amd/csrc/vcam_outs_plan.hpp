// The planning step of bsx_step_batch_vcam_geoms_outs: the call's output records checked and ordered into the ragged grid of its one resize pass.  Plain C++ on
// host memory — no HIP type, no context — so a stand-alone program can drive it (tests/test_vcam_outs_host.py does, under the host sanitizers).
//   in:   the geometry class of every item of the call (the class of ids[i]), the m records, the batch's YUYV bit;
//   out:  the refusals that concern a record alone (the text names outs[j] and the value), or the plan:
//           order    the records sorted by (class of their item, size) — a counting sort, stable: records of one group keep the caller's order;
//           groups   one per (class, size) pair that occurs, at most kVoMaxClasses * kVoMaxSizes = 32: its first place in `order`, its records, its first workgroup,
//                    the workgroups of one record (64 x 32 output tiles), the tiles per output row, and whether its stores are whole dwords — the rule of
//                    launch_vcam_geoms: a YUYV output, or out_w % 4 == 0 (every d_out is 4-byte aligned);
//           sizes    the distinct (out_w, out_h) in the order of their first record.
// Overlaps are not judged here: they need the items' frames and backgrounds (bsx_api.hip).
#pragma once
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/bsx.h"

namespace bsx {
constexpr int kVoMaxClasses = BSX_MAX_GEOMS, kVoMaxSizes = BSX_MAX_OUT_SIZES, kVoMaxPerItem = BSX_MAX_OUTS_PER_ITEM, kVoMaxGroups = kVoMaxClasses * kVoMaxSizes;
constexpr int kVoTileW = 64, kVoTileH = 32;      // the resize pass's output tile (kernels_img.hip: kVW x kVH)

struct VcamOutsGroup {
  int cls, size;           // the class of its items, the index of its size in VcamOutsPlan::sizes
  int first, count;        // places [first, first + count) of VcamOutsPlan::order
  long wg0;                // its first workgroup
  int per, ntx;            // workgroups of one record = ntx * ceil(out_h / 32), ntx = ceil(out_w / 64)
  bool words;              // whole-dword stores
};
struct VcamOutsPlan {
  enum { kOk = 0, kRefused = 1, kTooLarge = 2 };
  std::vector<int> order;                    // order[k] = the caller's index j of the record at place k
  std::vector<VcamOutsGroup> groups;
  int sizes[kVoMaxSizes][2] = {};
  int n_sizes = 0;
  long total_wg = 0;
  int bad = -1;                              // kRefused: the record the text names (-1: the call's m or outs)
  char text[200] = {0};
};

// kOk; kRefused with plan->text and plan->bad; kTooLarge where the grid would have 2^31 workgroups or more
inline int vcam_outs_plan(const int* item_class, int n, const bsx_vcam_out* outs, int m, bool yuyv, VcamOutsPlan* plan) {
  VcamOutsPlan& p = *plan;
  p = VcamOutsPlan{};
#define BSX_VO_REFUSE(j, ...) do { p.bad = (j); snprintf(p.text, sizeof p.text, __VA_ARGS__); return VcamOutsPlan::kRefused; } while (0)
  if (m < 0) BSX_VO_REFUSE(-1, "m = %d is negative", m);
  if (m > 0 && !outs) BSX_VO_REFUSE(-1, "outs is NULL with m = %d", m);
  std::vector<int> named((size_t)(n > 0 ? n : 0), 0), key((size_t)m, 0);
  int count[kVoMaxGroups] = {0};
  for (int j = 0; j < m; j++) {
    const bsx_vcam_out& o = outs[j];
    if (o.item < 0 || o.item >= n) BSX_VO_REFUSE(j, "outs[%d]: item %d is outside [0, %d)", j, o.item, n);
    if (o.out_w <= 0 || o.out_h <= 0) BSX_VO_REFUSE(j, "outs[%d]: output size %d x %d must be positive", j, o.out_w, o.out_h);
    if (yuyv && (o.out_w & 1)) BSX_VO_REFUSE(j, "outs[%d]: YUYV output needs an even width (out_w = %d)", j, o.out_w);
    if (!o.d_out) BSX_VO_REFUSE(j, "outs[%d]: d_out is NULL", j);
    if ((uintptr_t)o.d_out & 3) BSX_VO_REFUSE(j, "outs[%d]: d_out %p is not 4-byte aligned", j, (const void*)o.d_out);
    if (++named[(size_t)o.item] > kVoMaxPerItem) BSX_VO_REFUSE(j, "outs[%d]: record %d of items[%d] (at most %d name one item)", j, named[(size_t)o.item], o.item, kVoMaxPerItem);
    int s = 0;
    while (s < p.n_sizes && (p.sizes[s][0] != o.out_w || p.sizes[s][1] != o.out_h)) s++;
    if (s == p.n_sizes) {
      if (s == kVoMaxSizes) BSX_VO_REFUSE(j, "outs[%d]: %d x %d is distinct output size %d of the call (at most %d)", j, o.out_w, o.out_h, s + 1, kVoMaxSizes);
      p.sizes[s][0] = o.out_w; p.sizes[s][1] = o.out_h; p.n_sizes++;
    }
    const int cls = item_class[o.item];
    if (cls < 0 || cls >= kVoMaxClasses) BSX_VO_REFUSE(j, "outs[%d]: items[%d] has class %d outside [0, %d)", j, o.item, cls, kVoMaxClasses);
    key[(size_t)j] = cls * kVoMaxSizes + s;
    count[key[(size_t)j]]++;
  }
#undef BSX_VO_REFUSE
  int next[kVoMaxGroups];
  long wg = 0;
  for (int k = 0, at = 0; k < kVoMaxGroups; k++) {
    next[k] = at;
    if (!count[k]) continue;
    const int s = k % kVoMaxSizes, w = p.sizes[s][0], h = p.sizes[s][1];
    const int ntx = (int)(((long)w + kVoTileW - 1) / kVoTileW);
    const long per = (long)ntx * (((long)h + kVoTileH - 1) / kVoTileH);
    if (per >= (1l << 31) || wg + per * count[k] >= (1l << 31)) return VcamOutsPlan::kTooLarge;
    p.groups.push_back(VcamOutsGroup{k / kVoMaxSizes, s, at, count[k], wg, (int)per, ntx, yuyv || w % 4 == 0});
    wg += per * count[k];
    at += count[k];
  }
  p.total_wg = wg;
  p.order.resize((size_t)m);
  for (int j = 0; j < m; j++) p.order[(size_t)next[key[(size_t)j]]++] = j;
  return VcamOutsPlan::kOk;
}
}  // namespace bsx
