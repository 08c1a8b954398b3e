// The planning step of bsx_step_batch_vcam_geoms_outs_nv12: vcam_outs_plan.hpp's for records that name an NV12 surface.  Plain C++ on host memory — no HIP type, no
// context — so a stand-alone program can drive it (tests/test_vcam_nv12_host.py does, under the host sanitizers).
//   in:   the geometry class of every item of the call, the m records;
//   out:  the refusals that concern a record alone (the text names outs[j] and the value), or vcam_outs_plan's plan of the records taken as (item, out_w, out_h,
//         d_y): the same order, groups, sizes and workgroup counts — the NV12 form of the resize pass keeps the 64 x 32 tile.  A group's `words` is always set and
//         not read: the NV12 stores are dwords (16 bits for the 2-pixel group that ends a row of out_w % 4 == 2), which the checks below make aligned.
// What belongs to the surface is checked here, for every record, before the rules the two entry points share (the fifth record of an item, the fifth size): item,
// a positive and even size, the pitches, the planes.  Overlaps are not judged here (bsx_api.hip), but the extent they are judged on is: vcam_nv12_extent.
#pragma once
#include "span_overlap.hpp"
#include "vcam_outs_plan.hpp"

namespace bsx {
inline int vcam_nv12_plan(const int* item_class, int n, const bsx_vcam_out_nv12* outs, int m, VcamOutsPlan* plan) {
  VcamOutsPlan& p = *plan;
  p = VcamOutsPlan{};
#define BSX_VN_REFUSE(j, ...) do { p.bad = (j); snprintf(p.text, sizeof p.text, __VA_ARGS__); return VcamOutsPlan::kRefused; } while (0)
  if (m < 0) BSX_VN_REFUSE(-1, "m = %d is negative", m);
  if (m > 0 && !outs) BSX_VN_REFUSE(-1, "outs is NULL with m = %d", m);
  std::vector<bsx_vcam_out> recs((size_t)m);
  for (int j = 0; j < m; j++) {
    const bsx_vcam_out_nv12& o = outs[j];
    if (o.item < 0 || o.item >= n) BSX_VN_REFUSE(j, "outs[%d]: item %d is outside [0, %d)", j, o.item, n);
    if (o.out_w <= 0 || o.out_h <= 0) BSX_VN_REFUSE(j, "outs[%d]: output size %d x %d must be positive", j, o.out_w, o.out_h);
    if ((o.out_w | o.out_h) & 1) BSX_VN_REFUSE(j, "outs[%d]: NV12 output needs an even width and height (%d x %d)", j, o.out_w, o.out_h);
    if (o.pitch_y < o.out_w) BSX_VN_REFUSE(j, "outs[%d]: pitch_y = %d is below out_w = %d", j, o.pitch_y, o.out_w);
    if (o.pitch_y & 3) BSX_VN_REFUSE(j, "outs[%d]: pitch_y = %d is not a multiple of 4", j, o.pitch_y);
    if (o.pitch_uv < o.out_w) BSX_VN_REFUSE(j, "outs[%d]: pitch_uv = %d is below out_w = %d", j, o.pitch_uv, o.out_w);
    if (o.pitch_uv & 3) BSX_VN_REFUSE(j, "outs[%d]: pitch_uv = %d is not a multiple of 4", j, o.pitch_uv);
    if (!o.d_y) BSX_VN_REFUSE(j, "outs[%d]: d_y is NULL", j);
    if ((uintptr_t)o.d_y & 3) BSX_VN_REFUSE(j, "outs[%d]: d_y %p is not 4-byte aligned", j, (const void*)o.d_y);
    if (!o.d_uv) BSX_VN_REFUSE(j, "outs[%d]: d_uv is NULL", j);
    if ((uintptr_t)o.d_uv & 3) BSX_VN_REFUSE(j, "outs[%d]: d_uv %p is not 4-byte aligned", j, (const void*)o.d_uv);
    recs[(size_t)j] = bsx_vcam_out{o.item, o.out_w, o.out_h, o.d_y};
  }
#undef BSX_VN_REFUSE
  return vcam_outs_plan(item_class, n, recs.data(), m, true, plan);
}
}  // namespace bsx
