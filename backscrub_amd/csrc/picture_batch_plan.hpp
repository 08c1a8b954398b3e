// The planning step of the four calls that take n pictures of their own sizes and process them in ONE launch: bsx_resize_bgr_batch, bsx_gaussian_blur_bgr_batch,
// bsx_gaussian_blur_surfaces_batch, bsx_resize_surfaces_batch.  Plain C++ on host memory — no HIP type, no context — so a stand-alone program can drive it
// (tests/test_picture_batch_host.py, test_blur_surfaces_host.py and test_resize_surfaces_host.py do, under the host sanitizers).
//   in:   the n items, the context's n_streams;
//   out:  the refusals that concern the call's n and items, an item alone or two items together (the text names items[i] and the value), or the plan:
//           cls      the size class of every item: the distinct sizes numbered in the order of their first item, at most kPbMaxSizes = BSX_MAX_GEOMS.  The size is
//                    the one the launch's grid is ragged over: (w, h) of a blur, the destination's (dw, dh) of a resize — a class holds any mix of source sizes;
//           order    the items ordered by class (a counting sort on cls: stable): position q of the call is items[order[q]];
//           pos, wg, per   kernels.hpp's GeomSpans: class g owns positions [pos[g], pos[g + 1]) and workgroups [wg[g], wg[g + 1]) of the grid, per[g] = the
//                    workgroups of one picture of the class (the 64 x 16 tiles of a blur; ceil(ceil(dw / 4) * dh / 256) of the surfaces' resize: a lane makes
//                    four adjacent pixels of one output row, 256 lanes to a workgroup);
//           ntx      kernels.hpp's BlurTileCols: tiles per row of a picture of class g (0 where the call has no tile columns).
// Every rule's text exists once (the single-rule functions below); the ORDER in which a call judges its rules is its own, stated by its planner, and decides which
// refusal a caller sees when several are broken.
// A destination may overlap no item's source (its own included) and no other destination — the launch reads and writes them in no order; sources may overlap each
// other: two items may name one picture.  A plane is judged on vcam_nv12_extent: it ends at byte w of its last row, so a destination may lie in the padding
// [w, pitch) of another surface's last row.  No plane a plan accepts extends over 2^31 bytes or more, and no destination of the three calls whose kernels address
// it by 32-bit offsets.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/bsx.h"
#include "span_overlap.hpp"

namespace bsx {
constexpr int kPbMaxSizes = BSX_MAX_GEOMS;

struct PictureBatchPlan {
  enum { kOk = 0, kRefused = 1, kTooLarge = 2 };   // kTooLarge: the grid would have 2^31 workgroups or more
  std::vector<int> cls;                      // cls[i] = the size class of items[i]
  std::vector<int> order;                    // order[q] = the item at position q
  std::vector<Span> spans;                   // scratch of the overlap sweep: Span::item = i for the destination of items[i], planes * i + k for its source plane k
  int sizes[kPbMaxSizes][2] = {};
  int n_sizes = 0;
  int pos[kPbMaxSizes + 1] = {}, wg[kPbMaxSizes + 1] = {}, per[kPbMaxSizes] = {}, ntx[kPbMaxSizes] = {};
  int bad = -1;                              // kRefused: the item the text names (-1: the call's n, items or output size)
  char text[240] = {0};
  void reset() {                             // (the vectors keep their memory: a context plans every call into the same plan)
    cls.clear(); order.clear(); spans.clear();
    memset(sizes, 0, sizeof sizes); memset(pos, 0, sizeof pos); memset(wg, 0, sizeof wg); memset(per, 0, sizeof per); memset(ntx, 0, sizeof ntx);
    n_sizes = 0; bad = -1; text[0] = 0;
  }
};

#define BSX_PB_REFUSE(i, ...) do { p->bad = (i); snprintf(p->text, sizeof p->text, __VA_ARGS__); return false; } while (0)
// ---- the rules of one item.  All return true, or false with p->bad and a text that names items[i] and the value ---------------------------------------------------
inline bool pic_ptr(const void* v, const char* name, int i, PictureBatchPlan* p) {
  if (!v) BSX_PB_REFUSE(i, "items[%d]: %s is NULL", i, name);
  return true;
}
inline bool pic_aligned(const void* v, const char* name, int i, PictureBatchPlan* p) {
  if ((uintptr_t)v & 3) BSX_PB_REFUSE(i, "items[%d]: %s %p is not 4-byte aligned", i, name, v);
  return true;
}
inline bool pic_size(int w, int h, const char* what, int i, PictureBatchPlan* p) {      // what: "size", "source size", "output size"
  if (w <= 0 || h <= 0) BSX_PB_REFUSE(i, "items[%d]: %s %d x %d is not positive", i, what, w, h);
  return true;
}
inline bool pic_nv12_even(int w, int h, int i, PictureBatchPlan* p) {
  if ((w | h) & 1) BSX_PB_REFUSE(i, "items[%d]: NV12 needs an even width and height (%d x %d)", i, w, h);
  return true;
}
inline bool pic_pitch(int pitch, const char* name, int w, const char* w_name, int i, PictureBatchPlan* p) {
  if (pitch < w) BSX_PB_REFUSE(i, "items[%d]: %s = %d is below %s = %d", i, name, pitch, w_name, w);
  if (pitch & 3) BSX_PB_REFUSE(i, "items[%d]: %s = %d is not a multiple of 4", i, name, pitch);
  return true;
}
inline bool pic_ksize(int ksize, int i, PictureBatchPlan* p) {
  if (ksize < 1 || ksize > 31 || !(ksize & 1)) BSX_PB_REFUSE(i, "items[%d]: ksize %d is not an odd number of 1 .. 31", i, ksize);
  return true;
}
inline bool pic_no_flags(unsigned flags, int i, PictureBatchPlan* p) {
  if (flags) BSX_PB_REFUSE(i, "items[%d]: flags 0x%x: this call takes no flags", i, flags);
  return true;
}
inline bool pic_yuyv_flag_only(unsigned flags, int i, PictureBatchPlan* p) {
  if (flags & ~(unsigned)BSX_STREAM_YUYV_IN) BSX_PB_REFUSE(i, "items[%d]: flags 0x%x has bits outside yuyv-in (0x%x)", i, flags, BSX_STREAM_YUYV_IN);
  return true;
}
inline bool pic_yuyv_even(int w, int i, PictureBatchPlan* p) {
  if (w & 1) BSX_PB_REFUSE(i, "items[%d]: a YUYV source needs an even width (w = %d)", i, w);
  return true;
}
inline bool pic_reserved(int reserved, int i, PictureBatchPlan* p) {
  if (reserved) BSX_PB_REFUSE(i, "items[%d]: reserved = %d is not 0", i, reserved);
  return true;
}
constexpr size_t kPbLimit = (size_t)1 << 31;      // the kernels' offsets into a plane and into a destination are 32-bit
inline size_t pic_bytes(int w, int h, int bytes_per_pixel) { return (size_t)w * (size_t)h * (size_t)bytes_per_pixel; }
// a BGR picture of w x h; what: "size" / "output size", dims: "w * h" / "dw * dh"
inline bool pic_bgr_extent(int w, int h, const char* what, const char* dims, int i, PictureBatchPlan* p) {
  if (pic_bytes(w, h, 3) >= kPbLimit) BSX_PB_REFUSE(i, "items[%d]: %s %d x %d is beyond the kernel's 32-bit offsets (%s * 3 < 2^31)", i, what, w, h, dims);
  return true;
}
inline bool pic_plane_extent(int pitch, const char* pitch_name, int rows, int w, const char* plane, int i, PictureBatchPlan* p) {
  if (vcam_nv12_extent(pitch, rows, w) >= kPbLimit) BSX_PB_REFUSE(i, "items[%d]: the %s plane (%d rows of %s = %d) extends over 2 GiB or more", i, plane, rows, pitch_name, pitch);
  return true;
}
// ... of an NV12 surface's pointers, pitches and planes, which both surface calls judge together
inline bool pic_nv12_ptrs(const void* d_y, const void* d_uv, const void* d_dst, int i, PictureBatchPlan* p) {
  return pic_ptr(d_y, "d_y", i, p) && pic_ptr(d_uv, "d_uv", i, p) && pic_ptr(d_dst, "d_dst", i, p) && pic_aligned(d_y, "d_y", i, p) && pic_aligned(d_uv, "d_uv", i, p);
}
inline bool pic_nv12_pitches(int pitch_y, int pitch_uv, int w, const char* w_name, int i, PictureBatchPlan* p) {
  return pic_pitch(pitch_y, "pitch_y", w, w_name, i, p) && pic_pitch(pitch_uv, "pitch_uv", w, w_name, i, p);
}
inline bool pic_nv12_extents(int pitch_y, int pitch_uv, int w, int h, int i, PictureBatchPlan* p) {
  return pic_plane_extent(pitch_y, "pitch_y", h, w, "Y", i, p) && pic_plane_extent(pitch_uv, "pitch_uv", h / 2, w, "UV", i, p);
}

// ---- the steps every call shares ----------------------------------------------------------------------------------------------------------------------------------
// The count rules.  n == 0 passes with items NULL, and everything below is then empty.
inline bool batch_count(int n, int n_streams, const void* items, PictureBatchPlan* p) {
  p->reset();
  if (n < 0) BSX_PB_REFUSE(-1, "n = %d is negative", n);
  if (n > n_streams) BSX_PB_REFUSE(-1, "n = %d exceeds the context's %d streams", n, n_streams);
  if (n > 0 && !items) BSX_PB_REFUSE(-1, "items is NULL");
  p->cls.assign((size_t)n, 0);
  return true;
}
// the class of items[i], whose size is w x h — or the ninth-size refusal; what: "size" / "output size"
inline bool batch_class(int w, int h, const char* what, int i, PictureBatchPlan* p) {
  int g = 0;
  while (g < p->n_sizes && (p->sizes[g][0] != w || p->sizes[g][1] != h)) g++;
  if (g == p->n_sizes) {
    if (g == kPbMaxSizes) BSX_PB_REFUSE(i, "items[%d]: %d x %d is distinct %s %d of the call (at most %d)", i, w, h, what, g + 1, kPbMaxSizes);
    p->sizes[g][0] = w; p->sizes[g][1] = h; p->n_sizes++;
  }
  p->cls[(size_t)i] = g;
  return true;
}
// the spans of items[i]: its `planes` source planes (pushed first, in order: Span::item = planes * i + k), then its destination
inline void batch_source(const void* v, size_t bytes, int item, PictureBatchPlan* p) { p->spans.push_back({(uintptr_t)v, (uintptr_t)v + bytes, item, false}); }
inline void batch_dest(const void* v, size_t bytes, int i, PictureBatchPlan* p) { p->spans.push_back({(uintptr_t)v, (uintptr_t)v + bytes, i, true}); }
// no destination over a source or another destination; names[k] = what the call's texts call source plane k
inline bool batch_overlaps(int planes, const char* const* names, PictureBatchPlan* p) {
  const Span* d = nullptr;
  const Span* o = nullptr;
  if (!spans_overlap(p->spans, &d, &o)) return true;
  BSX_PB_REFUSE(d->item, "items[%d]: d_dst %p overlaps the %s of items[%d] (%p)", d->item, (const void*)d->begin, o->dst ? "destination" : names[o->item % planes],
                o->dst ? o->item : o->item / planes, (const void*)o->begin);
}
#undef BSX_PB_REFUSE
constexpr const char* kPbNv12Planes[2] = {"Y plane", "UV plane"};

// the workgroups one picture of w x h takes in the call's launch; *ntx = its tile columns, where the kernel has them
typedef long (*PictureWorkgroups)(int w, int h, int* ntx);
constexpr int kPbTileW = 64, kPbTileH = 16;              // the blur's output tile (kernels_img.hip: kGTW x kGTH)
constexpr int kPbLanePixels = 4, kPbThreads = 256;       // resize_surfaces_k: pixels per lane, lanes per workgroup (kernels_img.hip)
inline long blur_workgroups(int w, int h, int* ntx) { *ntx = (w + kPbTileW - 1) / kPbTileW; return (long)*ntx * (((long)h + kPbTileH - 1) / kPbTileH); }
inline long resize_workgroups(int dw, int dh, int* ntx) { *ntx = 0; return ((((long)dw + kPbLanePixels - 1) / kPbLanePixels) * (long)dh + kPbThreads - 1) / kPbThreads; }
inline long no_ragged_grid(int, int, int* ntx) { *ntx = 0; return 0; }      // bsx_resize_bgr_batch: one output size, a grid of (blocks, n)
// The ragged grid of the classes and the stable order.  kOk, or kTooLarge
inline int batch_grid(PictureWorkgroups of, PictureBatchPlan* p) {
  long count[kPbMaxSizes] = {0};
  for (const int g : p->cls) count[g]++;
  long wg = 0;
  for (int g = 0; g < kPbMaxSizes; g++) {
    int ntx = 0;
    const long per = g < p->n_sizes ? of(p->sizes[g][0], p->sizes[g][1], &ntx) : 0;
    if (wg + count[g] * per >= (1l << 31)) return PictureBatchPlan::kTooLarge;
    wg += count[g] * per;
    p->pos[g + 1] = p->pos[g] + (int)count[g];
    p->wg[g + 1] = (int)wg;
    p->per[g] = (int)per;
    p->ntx[g] = ntx;
  }
  const int n = (int)p->cls.size();
  p->order.assign((size_t)n, 0);
  int next[kPbMaxSizes];
  for (int g = 0; g < kPbMaxSizes; g++) next[g] = p->pos[g];
  for (int i = 0; i < n; i++) p->order[(size_t)next[p->cls[(size_t)i]]++] = i;
  return PictureBatchPlan::kOk;
}

// ---- the four calls: kOk; kRefused with p->text and p->bad; kTooLarge.  Each judges its items in index order, an item's rules in the order written here ------------
// bsx_resize_bgr_batch: every item to dw x dh — one class; the source sizes are free.  Neither extent is bounded: the kernel addresses both by pointer.
inline int resize_bgr_batch_plan(const bsx_resize_item* items, int n, int n_streams, int dw, int dh, PictureBatchPlan* p) {
  static const char* const kNames[1] = {"source picture"};
  if (!batch_count(n, n_streams, items, p)) return PictureBatchPlan::kRefused;
  if (n == 0) return PictureBatchPlan::kOk;
  if (dw <= 0 || dh <= 0) { snprintf(p->text, sizeof p->text, "output size %d x %d is not positive", dw, dh); return PictureBatchPlan::kRefused; }
  for (int i = 0; i < n; i++) {
    const bsx_resize_item& it = items[i];
    if (!pic_ptr(it.d_src, "d_src", i, p) || !pic_ptr(it.d_dst, "d_dst", i, p) || !pic_size(it.sw, it.sh, "source size", i, p) || !batch_class(dw, dh, "output size", i, p))
      return PictureBatchPlan::kRefused;
    batch_source(it.d_src, pic_bytes(it.sw, it.sh, 3), i, p);
    batch_dest(it.d_dst, pic_bytes(dw, dh, 3), i, p);
  }
  return batch_overlaps(1, kNames, p) ? batch_grid(no_ragged_grid, p) : PictureBatchPlan::kRefused;
}

// bsx_gaussian_blur_bgr_batch: classes by (w, h); a YUYV source is judged on its real extent, 2 bytes per pixel
inline int blur_bgr_batch_plan(const bsx_blur_item* items, int n, int n_streams, PictureBatchPlan* p) {
  static const char* const kNames[1] = {"source"};
  if (!batch_count(n, n_streams, items, p)) return PictureBatchPlan::kRefused;
  for (int i = 0; i < n; i++) {
    const bsx_blur_item& it = items[i];
    const bool yin = (it.flags & BSX_STREAM_YUYV_IN) != 0;
    if (!pic_size(it.w, it.h, "size", i, p) || !pic_ksize(it.ksize, i, p) || !pic_ptr(it.d_src, "d_src", i, p) || !pic_ptr(it.d_dst, "d_dst", i, p) ||
        !pic_yuyv_flag_only(it.flags, i, p) || (yin && (!pic_yuyv_even(it.w, i, p) || !pic_aligned(it.d_src, "YUYV d_src", i, p))) ||
        !pic_bgr_extent(it.w, it.h, "size", "w * h", i, p) || !batch_class(it.w, it.h, "size", i, p))
      return PictureBatchPlan::kRefused;
    batch_source(it.d_src, pic_bytes(it.w, it.h, yin ? 2 : 3), i, p);
    batch_dest(it.d_dst, pic_bytes(it.w, it.h, 3), i, p);
  }
  return batch_overlaps(1, kNames, p) ? batch_grid(blur_workgroups, p) : PictureBatchPlan::kRefused;
}

// bsx_gaussian_blur_surfaces_batch: classes by (w, h).  This call judges an item's size before its pointers, and the grid before the overlaps: blur_surfaces_grid is
// the plan without the overlap rule
inline int blur_surfaces_grid(const bsx_blur_surface_item* items, int n, int n_streams, PictureBatchPlan* p) {
  if (!batch_count(n, n_streams, items, p)) return PictureBatchPlan::kRefused;
  for (int i = 0; i < n; i++) {
    const bsx_blur_surface_item& it = items[i];
    if (!pic_size(it.w, it.h, "size", i, p) || !pic_nv12_even(it.w, it.h, i, p) || !pic_ksize(it.ksize, i, p) || !pic_nv12_ptrs(it.d_y, it.d_uv, it.d_dst, i, p) ||
        !pic_nv12_pitches(it.pitch_y, it.pitch_uv, it.w, "w", i, p) || !pic_no_flags(it.flags, i, p) || !pic_bgr_extent(it.w, it.h, "size", "w * h", i, p) ||
        !pic_nv12_extents(it.pitch_y, it.pitch_uv, it.w, it.h, i, p) || !batch_class(it.w, it.h, "size", i, p))
      return PictureBatchPlan::kRefused;
    batch_source(it.d_y, vcam_nv12_extent(it.pitch_y, it.h, it.w), 2 * i, p);
    batch_source(it.d_uv, vcam_nv12_extent(it.pitch_uv, it.h / 2, it.w), 2 * i + 1, p);
    batch_dest(it.d_dst, pic_bytes(it.w, it.h, 3), i, p);
  }
  return batch_grid(blur_workgroups, p);
}
inline int blur_surfaces_plan(const bsx_blur_surface_item* items, int n, int n_streams, PictureBatchPlan* p) {
  if (const int rc = blur_surfaces_grid(items, n, n_streams, p)) return rc;
  return batch_overlaps(2, kPbNv12Planes, p) ? PictureBatchPlan::kOk : PictureBatchPlan::kRefused;
}

// bsx_resize_surfaces_batch: classes by the destination's (dw, dh).  This call judges an item's pointers before its sizes
inline int resize_surfaces_plan(const bsx_resize_surface_item* items, int n, int n_streams, PictureBatchPlan* p) {
  if (!batch_count(n, n_streams, items, p)) return PictureBatchPlan::kRefused;
  for (int i = 0; i < n; i++) {
    const bsx_resize_surface_item& it = items[i];
    if (!pic_nv12_ptrs(it.d_y, it.d_uv, it.d_dst, i, p) || !pic_size(it.sw, it.sh, "source size", i, p) || !pic_nv12_even(it.sw, it.sh, i, p) ||
        !pic_nv12_pitches(it.pitch_y, it.pitch_uv, it.sw, "sw", i, p) || !pic_size(it.dw, it.dh, "output size", i, p) || !pic_no_flags(it.flags, i, p) ||
        !pic_reserved(it.reserved, i, p) || !pic_nv12_extents(it.pitch_y, it.pitch_uv, it.sw, it.sh, i, p) ||
        !pic_bgr_extent(it.dw, it.dh, "output size", "dw * dh", i, p) || !batch_class(it.dw, it.dh, "output size", i, p))
      return PictureBatchPlan::kRefused;
    batch_source(it.d_y, vcam_nv12_extent(it.pitch_y, it.sh, it.sw), 2 * i, p);
    batch_source(it.d_uv, vcam_nv12_extent(it.pitch_uv, it.sh / 2, it.sw), 2 * i + 1, p);
    batch_dest(it.d_dst, pic_bytes(it.dw, it.dh, 3), i, p);
  }
  return batch_overlaps(2, kPbNv12Planes, p) ? batch_grid(resize_workgroups, p) : PictureBatchPlan::kRefused;
}
}  // namespace bsx
