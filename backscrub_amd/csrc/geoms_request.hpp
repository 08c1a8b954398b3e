// The request of the five multi-geometry steps and its ONE check.  Plain C++ on host memory — no HIP type, no context — like the planners it calls
// (vcam_outs_plan.hpp, vcam_nv12_plan.hpp), so a stand-alone program can drive it (tests/test_geoms_request_host.py does, under the host sanitizers).
//   GeomsKind / kGeomsKinds   the five entry points and the one table of what differs between them;
//   GeomsClass                what the check needs of a geometry class (the caller fills it from the context);
//   GeomsRequest              the call as its entry point received it, plus the two facts of the context's state the rules ask for;
//   geoms_check               every rule, in one order (below); leaves the spans, the class of every item, the plan of the output records and, for surfaces, the
//                             items in the form the front end reads in a GeomsChecked;
// The overlap sweep is span_overlap.hpp's.
// The order of the rules decides which refusal a caller sees when several are broken: items NULL; the vcam step's output size; the batch flags; a pending pipelined
// composite; an onmask callback; the vcam step's odd YUYV width; the items in index order; the plan of the records; the overlaps.
#pragma once
#include "span_overlap.hpp"
#include "vcam_nv12_plan.hpp"

namespace bsx {
// every entry point that advances the temporal state refuses while the two-deep pipeline holds a composite that reads it
constexpr char kPendingComposite[] = "a pipelined composite is pending (flush with bsx_step_batch_pipelined(ctx, NULL, ...) first)";

enum class GeomsKind { Geoms, VcamGeoms, VcamOuts, VcamOutsNv12, Surfaces };
enum class GeomsItemOut { None, ClassSize, CallSize };      // does an item carry d_out, and on which extent is it judged
enum class GeomsRecords { None, Bgr, Nv12 };                // the output records: none, bsx_vcam_out, bsx_vcam_out_nv12
struct GeomsKindInfo {
  const char* fn;
  struct { unsigned bits; const char* text; } flags[3];     // batch flags, in the order they are judged: a set bit of `bits` is refused with `text` (one %x: the flags)
  const char* onmask;                                       // the refusal of a context with an onmask callback
  GeomsItemOut item_out;
  bool surface;                                             // the frame of an item is an NV12 surface (bsx_surface_item), else BGR / YUYV (bsx_geom_item)
  GeomsRecords records;
  const char* unfusable;                                    // the entry point's own suffix on the "off the fused tile route" text
};
#define BSX_GQ_YUYV_IN "flags 0x%x: YUYV input frames are not taken by the multi-geometry step as a batch flag (the format belongs to the item: the yuyv-in bit, 0x40, of items[i].setting.flags)"
#define BSX_GQ_VCAM_FLAGS {{BSX_STEP_NO_MASK, "unsupported flags 0x%x (the no-mask step has no vcam form)"}, {BSX_STEP_YUYV_IN, BSX_GQ_YUYV_IN}, {~(unsigned)BSX_STEP_YUYV, "flags 0x%x has bits outside yuyv"}}
constexpr GeomsKindInfo kGeomsKinds[5] = {
  {"bsx_step_batch_geoms", {{BSX_STEP_YUYV_IN, BSX_GQ_YUYV_IN}, {~(unsigned)(BSX_STEP_YUYV | BSX_STEP_NO_MASK), "flags 0x%x has bits outside yuyv / no-mask"}, {0, nullptr}},
   "needs the fused mask + blend route (no onmask callback)", GeomsItemOut::ClassSize, false, GeomsRecords::None, ""},
  {"bsx_step_batch_vcam_geoms", BSX_GQ_VCAM_FLAGS, "needs the fused mask route (no onmask callback)", GeomsItemOut::CallSize, false, GeomsRecords::None,
   "; bsx_step_batch_vcam_mixed takes such a context"},
  {"bsx_step_batch_vcam_geoms_outs", BSX_GQ_VCAM_FLAGS, "needs the fused mask route (no onmask callback)", GeomsItemOut::None, false, GeomsRecords::Bgr, ""},
  {"bsx_step_batch_vcam_geoms_outs_nv12", {{~0u, "flags 0x%x: this step takes no flags (an item's format and flips belong to items[i].setting.flags)"}, {0, nullptr}, {0, nullptr}},
   "needs the fused mask route (no onmask callback)", GeomsItemOut::None, false, GeomsRecords::Nv12, ""},
  {"bsx_step_batch_surfaces", {{~0u, "flags 0x%x: this step takes no flags (an item's flips belong to items[i].setting.flags)"}, {0, nullptr}, {0, nullptr}},
   "needs the fused mask route (no onmask callback)", GeomsItemOut::None, true, GeomsRecords::Nv12, ""},
};
#undef BSX_GQ_VCAM_FLAGS
#undef BSX_GQ_YUYV_IN
inline const GeomsKindInfo& geoms_kind(GeomsKind k) { return kGeomsKinds[(int)k]; }

// a class as the check sees it: streams [first, ...) of W x H; fusable: on the fused tile route; tab_mode: its down-scale table; yuyv_fusable: prep_yuyv_fusable of it
struct GeomsClass { int first, width, height; bool fusable; int tab_mode, roi_x, roi_w, roi_h; bool yuyv_fusable; };

struct GeomsRequest {
  GeomsKind kind;
  const int* ids;                                  // checked by the caller: n ids of streams of the context, no duplicates
  int n;
  const bsx_geom_item* items;                      // every kind but Surfaces
  const bsx_surface_item* surfaces;                // Surfaces
  int out_w, out_h;                                // VcamGeoms
  const bsx_vcam_out* outs;                        // VcamOuts
  const bsx_vcam_out_nv12* outs_nv12;              // VcamOutsNv12, Surfaces
  int m;
  unsigned flags;
  const GeomsClass* classes;                       // the context's classes, in stream order
  int n_classes;
  bool pending, onmask;                            // the context holds a pipelined composite; it has an onmask callback
  bool yuyv() const { return (flags & BSX_STEP_YUYV) != 0; }
  bool has_items() const { return geoms_kind(kind).surface ? surfaces != nullptr : items != nullptr; }
};

constexpr unsigned kGeomStreamFlags = BSX_STEP_FLIP_H | BSX_STEP_FLIP_V | BSX_STREAM_FILTER_OFF | BSX_STREAM_YUYV_IN;
constexpr unsigned kSurfaceStreamFlags = BSX_STEP_FLIP_H | BSX_STEP_FLIP_V | BSX_STREAM_FILTER_OFF;
struct SurfaceRefusal { char text[320] = {0}; };
// what a checked request leaves behind (host scratch that a context keeps between calls)
struct GeomsChecked {
  enum { kOk = 0, kRefused = 1, kTooLarge = 2 };   // kTooLarge: the grid of the resize pass would have 2^31 workgroups or more
  std::vector<Span> spans;
  std::vector<int> item_class;
  std::vector<bsx_geom_item> front_items;          // Surfaces: the items as the front end takes them (d_frame = the Y plane)
  VcamOutsPlan plan;
  SurfaceRefusal why;                              // kRefused: the text
};

#define BSX_GQ_REFUSE(...) do { snprintf(r->text, sizeof r->text, __VA_ARGS__); return false; } while (0)
// ---- the rules of one item.  All return true, or false with a text that names items[i] and the value -------------------------------------------------------------
inline bool geoms_item_bits(unsigned f, int i, bool surface, SurfaceRefusal* r) {
  if (f & 0xFF00u) BSX_GQ_REFUSE("items[%d]: setting flags 0x%x asks for a background blur, which the multi-geometry step does not take", i, f);
  if (surface && (f & BSX_STREAM_YUYV_IN)) BSX_GQ_REFUSE("items[%d]: setting flags 0x%x has the yuyv-in bit: every frame of this call is an NV12 surface", i, f);
  if (f & ~(surface ? kSurfaceStreamFlags : kGeomStreamFlags)) BSX_GQ_REFUSE("items[%d]: setting flags 0x%x has bits outside flip / filter-off%s", i, f, surface ? "" : " / yuyv-in");
  return true;
}
inline bool geoms_item_ptr(const void* p, const char* name, int i, SurfaceRefusal* r) {
  if (!p) BSX_GQ_REFUSE("items[%d]: %s is NULL", i, name);
  if ((uintptr_t)p & 3) BSX_GQ_REFUSE("items[%d]: %s %p is not 4-byte aligned", i, name, p);
  return true;
}
inline bool geoms_item_fusable(const GeomsClass& G, int i, int id, int g, const char* suffix, SurfaceRefusal* r) {
  if (!G.fusable)
    BSX_GQ_REFUSE("items[%d]: stream %d is of class %d (%d x %d), which is off the fused tile route (width, roi.x, roi.w multiples of 4, a tiled linear mask up-scale)%s",
                  i, id, g, G.width, G.height, suffix);
  return true;
}
// A YUYV item of class g: admitted where the class has the fused YUYV prep, else the refusal names the table that is in the way.  There is no conversion fallback:
// the caller converts that stream with bsx_yuyv_to_bgr.
inline bool geoms_item_yuyv(const GeomsClass& G, int i, int id, int g, SurfaceRefusal* r) {
  if (G.yuyv_fusable) return true;
  char why[160];
  if (G.tab_mode == 1) snprintf(why, sizeof why, "its down-scale table is a copy (capture ROI %d x %d = model ROI)", G.roi_w, G.roi_h);
  else if (G.tab_mode == 2) snprintf(why, sizeof why, "its down-scale table is the 2x2 area mean (capture ROI %d x %d = twice the model ROI)", G.roi_w, G.roi_h);
  else snprintf(why, sizeof why, "its down-scale table is linear but width %d and roi.x %d must be even and the ROI row at least 4 pixels", G.width, G.roi_x);
  BSX_GQ_REFUSE("items[%d]: stream %d is of class %d (%d x %d), which has no fused YUYV prep: %s; convert that stream's frames with bsx_yuyv_to_bgr and pass them as BGR",
                i, id, g, G.width, G.height, why);
}
// is a class admitted for NV12 items?  The proper INTER_LINEAR down-scale table (mode 0), an even width and height, a width of at least 4 (the prep kernel's 4-byte
// windows).  Chroma is addressed by the frame's column and row, so the ROI's parity is free.  Item i is stream `id` of class g (W x H)
inline bool vcam_surface_class(int i, int id, int g, int W, int H, int tab_mode, int roi_w, int roi_h, SurfaceRefusal* r) {
  char why[160];
  if (tab_mode == 1) snprintf(why, sizeof why, "its down-scale table is a copy (capture ROI %d x %d = model ROI)", roi_w, roi_h);
  else if (tab_mode == 2) snprintf(why, sizeof why, "its down-scale table is the 2x2 area mean (capture ROI %d x %d = twice the model ROI)", roi_w, roi_h);
  else if (tab_mode != 0) snprintf(why, sizeof why, "its down-scale table has mode %d", tab_mode);
  else if ((W | H) & 1) snprintf(why, sizeof why, "NV12 needs an even width and height");
  else if (W < 4) snprintf(why, sizeof why, "the width %d is below 4", W);
  else return true;
  BSX_GQ_REFUSE("items[%d]: stream %d is of class %d (%d x %d), which has no fused NV12 prep: %s; convert such surfaces with bsx_nv12_to_bgr", i, id, g, W, H, why);
}
// what concerns one NV12 input surface alone: the setting bits, the two planes, the two pitches, the background where it is read
inline bool vcam_surface_item(const bsx_surface_item& it, int i, int W, int H, SurfaceRefusal* r) {
  const unsigned f = it.setting.flags;
  if (!geoms_item_bits(f, i, true, r) || !geoms_item_ptr(it.d_y, "d_y", i, r) || !geoms_item_ptr(it.d_uv, "d_uv", i, r)) return false;
  if (it.pitch_y < W) BSX_GQ_REFUSE("items[%d]: pitch_y = %d is below the width %d of its class", i, it.pitch_y, W);
  if (it.pitch_y & 3) BSX_GQ_REFUSE("items[%d]: pitch_y = %d is not a multiple of 4", i, it.pitch_y);
  if (it.pitch_uv < W) BSX_GQ_REFUSE("items[%d]: pitch_uv = %d is below the width %d of its class", i, it.pitch_uv, W);
  if (it.pitch_uv & 3) BSX_GQ_REFUSE("items[%d]: pitch_uv = %d is not a multiple of 4", i, it.pitch_uv);
  if ((unsigned long long)it.pitch_y * (unsigned long long)H >= (1ull << 31) || (unsigned long long)it.pitch_uv * (unsigned long long)(H / 2) >= (1ull << 31))
    BSX_GQ_REFUSE("items[%d]: pitch_y = %d, pitch_uv = %d at %d rows: a plane of 2 GiB or more", i, it.pitch_y, it.pitch_uv, H);
  return (f & BSX_STREAM_FILTER_OFF) || geoms_item_ptr(it.setting.d_bg, "setting.d_bg", i, r);      // (filter off: reads no background)
}

inline int geoms_class_of(const GeomsRequest& q, int stream) { int g = 0; while (g + 1 < q.n_classes && stream >= q.classes[g + 1].first) g++; return g; }

// item i of a request whose frames are BGR / YUYV: its rules, then its spans (Span::item = i)
inline bool geoms_check_item(const GeomsRequest& q, int i, int g, std::vector<Span>& sp, SurfaceRefusal* r) {
  const GeomsKindInfo& K = geoms_kind(q.kind);
  const bsx_geom_item& it = q.items[i];
  const GeomsClass& G = q.classes[g];
  const unsigned f = it.setting.flags;
  if (!geoms_item_bits(f, i, false, r) || !geoms_item_ptr(it.d_frame, "d_frame", i, r)) return false;
  if (K.item_out != GeomsItemOut::None && !geoms_item_ptr(it.d_out, "d_out", i, r)) return false;
  if (K.item_out == GeomsItemOut::ClassSize && q.yuyv() && (G.width & 1))
    BSX_GQ_REFUSE("items[%d]: YUYV output needs an even width (stream %d is of class %d, %d x %d)", i, q.ids[i], g, G.width, G.height);
  if (!geoms_item_fusable(G, i, q.ids[i], g, K.unfusable, r)) return false;
  if ((f & BSX_STREAM_YUYV_IN) && !geoms_item_yuyv(G, i, q.ids[i], g, r)) return false;
  const size_t px = (size_t)G.width * G.height, out_px = K.item_out == GeomsItemOut::CallSize ? (size_t)q.out_w * q.out_h : px;
  sp.push_back({(uintptr_t)it.d_frame, (uintptr_t)it.d_frame + px * ((f & BSX_STREAM_YUYV_IN) ? 2 : 3), i, false});      // the frame's real extent
  if (K.item_out != GeomsItemOut::None) sp.push_back({(uintptr_t)it.d_out, (uintptr_t)it.d_out + out_px * (q.yuyv() ? 2 : 3), i, true});
  if (f & BSX_STREAM_FILTER_OFF) return true;                          // reads no background
  if (!geoms_item_ptr(it.setting.d_bg, "setting.d_bg", i, r)) return false;
  sp.push_back({(uintptr_t)it.setting.d_bg, (uintptr_t)it.setting.d_bg + px * 3, i, false});
  return true;
}
// ... whose frames are NV12 surfaces: an input plane's extent is pitch * (rows - 1) + W; Span::item = 3 i for d_y, 3 i + 1 for d_uv, 3 i + 2 for the background
inline bool geoms_check_surface(const GeomsRequest& q, int i, int g, GeomsChecked* out) {
  const bsx_surface_item& it = q.surfaces[i];
  const GeomsClass& G = q.classes[g];
  SurfaceRefusal* const r = &out->why;
  if (!vcam_surface_item(it, i, G.width, G.height, r) || !geoms_item_fusable(G, i, q.ids[i], g, geoms_kind(q.kind).unfusable, r) ||
      !vcam_surface_class(i, q.ids[i], g, G.width, G.height, G.tab_mode, G.roi_w, G.roi_h, r)) return false;
  out->front_items[(size_t)i] = bsx_geom_item{it.d_y, nullptr, it.setting};
  std::vector<Span>& sp = out->spans;
  sp.push_back({(uintptr_t)it.d_y, (uintptr_t)it.d_y + vcam_nv12_extent(it.pitch_y, G.height, G.width), 3 * i, false});
  sp.push_back({(uintptr_t)it.d_uv, (uintptr_t)it.d_uv + vcam_nv12_extent(it.pitch_uv, G.height / 2, G.width), 3 * i + 1, false});
  if (it.setting.flags & BSX_STREAM_FILTER_OFF) return true;          // reads no background
  sp.push_back({(uintptr_t)it.setting.d_bg, (uintptr_t)it.setting.d_bg + (size_t)G.width * G.height * 3, 3 * i + 2, false});
  return true;
}

// the overlap of destination d with o, as the request's kind words it
inline void geoms_overlap_text(const GeomsRequest& q, const Span* d, const Span* o, SurfaceRefusal* r) {
  const GeomsKindInfo& K = geoms_kind(q.kind);
  const void* const db = (const void*)d->begin;
  const void* const ob = (const void*)o->begin;
  if (K.records == GeomsRecords::None)
    snprintf(r->text, sizeof r->text, "items[%d]: d_out %p overlaps %s of items[%d] (%p)", d->item, db, o->dst ? "the output" : "a frame or background", o->item, ob);
  else if (K.records == GeomsRecords::Bgr)
    snprintf(r->text, sizeof r->text, "outs[%d]: d_out %p overlaps %s[%d] (%p)", d->item, db, o->dst ? "the output of outs" : "a frame or background of items", o->item, ob);
  else {                                                               // Span::item of an output plane: 2 j for outs[j].d_y, 2 j + 1 for outs[j].d_uv
    static const char* const kIn[3] = {"d_y", "d_uv", "setting.d_bg"};
    const char* const plane = (d->item & 1) ? "d_uv" : "d_y";
    if (o->dst) snprintf(r->text, sizeof r->text, "outs[%d]: %s %p overlaps %s of outs[%d] (%p)", d->item / 2, plane, db, (o->item & 1) ? "d_uv" : "d_y", o->item / 2, ob);
    else snprintf(r->text, sizeof r->text, "outs[%d]: %s %p overlaps %s of items[%d] (%p)", d->item / 2, plane, db, K.surface ? kIn[o->item % 3] : "a frame or background",
                  K.surface ? o->item / 3 : o->item, ob);
  }
}

// GeomsChecked::kOk; kRefused with out->why.text; kTooLarge.  Nothing is enqueued before it passes.
inline int geoms_check(const GeomsRequest& q, GeomsChecked* out) {
  const GeomsKindInfo& K = geoms_kind(q.kind);
  SurfaceRefusal* const r = &out->why;
#define BSX_GQ_CALL(...) do { snprintf(r->text, sizeof r->text, __VA_ARGS__); return GeomsChecked::kRefused; } while (0)
  if (!q.has_items()) BSX_GQ_CALL("items is NULL");
  const bool vcam = q.kind == GeomsKind::VcamGeoms;
  if (vcam && (q.out_w <= 0 || q.out_h <= 0)) BSX_GQ_CALL("output size %d x %d must be positive", q.out_w, q.out_h);
  for (const auto& fl : K.flags) if (q.flags & fl.bits) BSX_GQ_CALL(fl.text, q.flags);
  if (q.pending) BSX_GQ_CALL("%s", kPendingComposite);
  if (q.onmask) BSX_GQ_CALL("%s", K.onmask);
  if (vcam && q.yuyv() && (q.out_w & 1)) BSX_GQ_CALL("YUYV output needs an even width (out_w = %d)", q.out_w);
#undef BSX_GQ_CALL
  std::vector<Span>& sp = out->spans;
  sp.clear();
  out->item_class.resize((size_t)q.n);
  if (K.surface) out->front_items.resize((size_t)q.n);
  for (int i = 0; i < q.n; i++) {
    const int g = out->item_class[(size_t)i] = geoms_class_of(q, q.ids[i]);
    if (!(K.surface ? geoms_check_surface(q, i, g, out) : geoms_check_item(q, i, g, sp, r))) return GeomsChecked::kRefused;
  }
  if (K.records != GeomsRecords::None) {
    VcamOutsPlan* const plan = &out->plan;
    const bool nv12 = K.records == GeomsRecords::Nv12;
    const int pr = nv12 ? vcam_nv12_plan(out->item_class.data(), q.n, q.outs_nv12, q.m, plan) : vcam_outs_plan(out->item_class.data(), q.n, q.outs, q.m, q.yuyv(), plan);
    if (pr == VcamOutsPlan::kRefused) { snprintf(r->text, sizeof r->text, "%s", plan->text); return GeomsChecked::kRefused; }
    if (pr == VcamOutsPlan::kTooLarge) return GeomsChecked::kTooLarge;
    for (int j = 0; j < q.m; j++) {
      if (nv12) {                                                      // a plane's extent: pitch * (rows - 1) + out_w
        const bsx_vcam_out_nv12& o = q.outs_nv12[j];
        sp.push_back({(uintptr_t)o.d_y, (uintptr_t)o.d_y + vcam_nv12_extent(o.pitch_y, o.out_h, o.out_w), 2 * j, true});
        sp.push_back({(uintptr_t)o.d_uv, (uintptr_t)o.d_uv + vcam_nv12_extent(o.pitch_uv, o.out_h / 2, o.out_w), 2 * j + 1, true});
      } else {
        sp.push_back({(uintptr_t)q.outs[j].d_out, (uintptr_t)q.outs[j].d_out + (size_t)q.outs[j].out_w * q.outs[j].out_h * (q.yuyv() ? 2 : 3), j, true});
      }
    }
  }
  const Span* d = nullptr;
  const Span* o = nullptr;
  if (!spans_overlap(sp, &d, &o)) return GeomsChecked::kOk;
  geoms_overlap_text(q, d, o, r);
  return GeomsChecked::kRefused;
}
#undef BSX_GQ_REFUSE
}  // namespace bsx
