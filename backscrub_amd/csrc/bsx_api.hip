// bsx_api.hip — the C ABI of libbsx.so (include/bsx.h): context, geometry, per-batch launch
// sequence.  Host-side mirror of lib/libbackscrub.cc (bs_maskgen_new :161-259,
// bs_maskgen_process :279-376, bs_maskgen_delete :261-277) and of the compositing step of
// app/deepseg.cc (:108-134, :649-661), re-designed for batches of independent streams
// resident in HBM.
#include "debug_switches.hpp"
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../include/bsx.h"
#include "gen_mid.hpp"
#include "kernels.hpp"
#include "roctx_ranges.hpp"
#include "plan.hpp"
#include "refusal.hpp"
#include "rtc.hpp"
#include "specialised.hpp"
#include "tflite_model.hpp"
#include "geoms_request.hpp"
#include "picture_batch_plan.hpp"

using namespace bsx;

namespace {
thread_local std::string g_last_error;

struct HostResizeTab {
  std::vector<int> xofs, yofs;
  std::vector<short> xa, ya;
  int sw = 0, sh = 0, dw = 0, dh = 0, mode = 0;
};

inline int cv_floor(float v) { int i = (int)v; return i - (i > v); }
inline short sat_short(long v) { return (short)(v < -32768 ? -32768 : (v > 32767 ? 32767 : v)); }

// Coefficient tables of cv::resize(INTER_LINEAR) for 8-bit images (OpenCV imgproc resize.cpp):
// scale = 1/(dst/src) in double; fx = (float)((dx+0.5)*scale-0.5); sx = floor(fx); fx -= sx;
// left/right clamps zero the fraction; coefficients = saturate_cast<short>(w*2048) (round-half-even).
HostResizeTab make_resize_tab(int sw, int sh, int dw, int dh) {
  HostResizeTab t;
  t.sw = sw; t.sh = sh; t.dw = dw; t.dh = dh;
  if (sw == dw && sh == dh) { t.mode = 1; return t; }
  double inv_x = (double)dw / sw, inv_y = (double)dh / sh;
  double scale_x = 1. / inv_x, scale_y = 1. / inv_y;
  long isx = lrint(scale_x), isy = lrint(scale_y);
  bool area_fast = std::fabs(scale_x - (double)isx) < 2.220446049250313e-16 && std::fabs(scale_y - (double)isy) < 2.220446049250313e-16;
  if (area_fast && isx == 2 && isy == 2) { t.mode = 2; return t; }
  t.xofs.resize(dw); t.xa.resize(2 * (size_t)dw); t.yofs.resize(dh); t.ya.resize(2 * (size_t)dh);
  for (int dx = 0; dx < dw; dx++) {
    float fx = (float)((dx + 0.5) * scale_x - 0.5);
    int sx = cv_floor(fx);
    fx -= sx;
    if (sx < 0) { fx = 0; sx = 0; }
    if (sx >= sw - 1) { fx = 0; sx = sw - 1; }
    t.xofs[dx] = sx;
    t.xa[2 * dx] = sat_short(lrintf((1.f - fx) * 2048.f));
    t.xa[2 * dx + 1] = sat_short(lrintf(fx * 2048.f));
  }
  for (int dy = 0; dy < dh; dy++) {
    float fy = (float)((dy + 0.5) * scale_y - 0.5);
    int sy = cv_floor(fy);
    fy -= sy;
    t.yofs[dy] = sy;
    t.ya[2 * dy] = sat_short(lrintf((1.f - fy) * 2048.f));
    t.ya[2 * dy + 1] = sat_short(lrintf(fy * 2048.f));
  }
  return t;
}

struct DevResizeTab {
  ResizeTab tab;
  void* mem = nullptr;
};
// capture size -> virtual camera size (bsx_step_batch_vcam): always a linear table (the 2x2 area mode expanded to one: kernels.hpp), and whether the tile
// footprints fit the kernel's LDS staging area
struct VcamTab {
  DevResizeTab d;
  bool direct = false;
};

}  // namespace

struct bsx_ctx {
  // callbacks (lib/libbackscrub.cc:37-41)
  bsx_debug_fn ondebug = nullptr;
  bsx_stage_fn onprep = nullptr, oninfer = nullptr, onmask = nullptr;
  void* caller_ctx = nullptr;
  // model
  Graph graph;
  Plan plan;
  int model_type = BSX_MODEL_UNKNOWN;
  float norm_scale = 0, norm_offset = 0;
  // geometry
  int width = 0, height = 0, n_streams = 0, device = 0;
  int inW = 0, inH = 0, inC = 0, outW = 0, outH = 0, outC = 0;
  Rect4 roi{}, in_roi{};
  size_t threads = 0;
  // device state
  hipStream_t own_stream = nullptr;
  float* d_arena = nullptr;
  float* d_net_in = nullptr;        // network input  [n][inH][inW][inC] f32 (written by the prep kernels)
  uint32_t* d_net_in_u8 = nullptr;  // the same tensor before convertTo: [n][inH][inW] R | G<<8 | B<<16 — what the stems with a byte path read (in_u8)
  // bs_maskgen_process for ONE frame is a chain of 7 (Meet / MLKit) to ~45 (DeepLab) dependent launches of a few microseconds each: launch-bound.  The chain of
  // a stream slot is captured once into a hipGraph and replayed (BSX_NO_GRAPH=1, or any stage callback — they need host synchronisation between stages — keeps
  // the direct launches).  graph_state: 0 = not tried, 1 = usable, -1 = capture failed on this runtime (direct launches from then on).
  std::map<int, hipGraphExec_t> host_graphs;
  int graph_state = 0;
  bool in_u8 = false;               // the step's prep writes ONLY the 8-bit form and the stem normalises on load (seg_head_k / dl_head0_k; bit-identical).
                                    //   BSX_F32_INPUT=1 (read at bsx_new) keeps the f32 tensor for A/B timing; the stage-debug entry writes both.
  float* d_net_out = nullptr;       // network output [n][outH][outW][outC] f32 (read by the decode kernel)
  float* d_weights = nullptr;
  uint16_t* d_weights16 = nullptr;   // split-f16 copies of the large pointwise-conv weights (Plan::weights16)
  int f16_terms = 3;                 // per-launch path: 3 = split-f16 MFMA GEMM (f32-grade, default), 1 = plain f16 inputs (BSX_F16_GEMM=fast), 0 = f32 MFMA (BSX_F16_GEMM=off)
  uint8_t* d_ofinal = nullptr;
  uint8_t* d_masks = nullptr;
  uint8_t* d_host_frame = nullptr;  // staging for bsx_process_host
  uint8_t* d_bgr_scratch = nullptr; // BGR composite of bsx_step_batch_yuyv / _ex when the fused epilogue does not apply (lazy)
  uint8_t* d_bgr_scratch2 = nullptr; // ... its flipped copy when a YUYV pack follows (lazy)
  uint8_t* d_mask_scratch = nullptr; // BSX_STEP_NO_MASK on the unfused route: the batch's full-resolution masks for the blend alone, 255 outside the ROI (lazy)
  uint8_t* d_bgblur_scratch = nullptr; // BSX_STEP_BGBLUR when the single pass does not apply: the blurred frames (lazy)
  uint8_t* d_bgr_in_scratch = nullptr; // BSX_STEP_YUYV_IN where the fused kernels do not apply: the batch converted to BGR (lazy)
  float* d_color_lut = nullptr;
  MicroOp* d_program = nullptr;     // per-frame network program (kernels_frame.hip)
  bool use_program = false;
  SpecialisedKernels kern;          // the program as ONE graph-specialised kernel and the segment kernels specialised to this graph (specialised.hpp); null: the
                                    // interpreter / the ahead-of-time segment kernels run
  BilateralParams bilateral{};
  DevResizeTab tab_down, tab_up;
  uint8_t* d_tile_class = nullptr;    // [n_streams][mask tiles]: 1 / 2 = the tile's source block is all 0xFF / 0x00 (tile_class_k), read by mask_tile_k
  size_t tiles_per_frame = 0;
  std::map<std::pair<std::pair<int, int>, std::pair<int, int>>, DevResizeTab> bg_tabs;
  std::map<std::pair<int, int>, VcamTab> vcam_tabs;   // (out_w, out_h) -> the capture -> vcam table of bsx_step_batch_vcam
  std::string last_error, plan_text;
  bool arena_poison = false;           // BSX_ARENA_POISON (debug build): the activation arena is filled with 0xFF bytes — NaNs — in front of every network stage, so a tensor
                                       // the read-back entry serves although nothing wrote it comes back non-finite (tests/test_gpu_layers.py)
  bool last_net_logits = true;         // did the last network stage write the logits buffer (false: its last kernel decoded straight into the temporal state)
  int last_net_n = 0;                  // frames of the last network stage: the launchers choose some fusions by batch size (chain3_on), the read-back entry answers for that run
  bool keep_logits = false;            // BSX_KEEP_LOGITS: segmented plans write the logits and run the stand-alone decode (A/B, debugging)
  bool no_mask_blend_fusion = false;   // BSX_NO_MASK_BLEND_FUSION, read once at bsx_new (no getenv on the per-step path)
  bool no_bgblur_fusion = false;       // BSX_NO_BGBLUR_FUSION: BSX_STEP_BGBLUR always as blur pass + step (the A/B switch of the single-pass form)
  bool no_mask_tile = false;           // BSX_NO_MASK_TILE (tests: the generic mask kernel), likewise
  bool vcam_direct = false;            // BSX_VCAM_DIRECT (tests: bsx_step_batch_vcam's per-tap path on every table), likewise
  bool no_uniform_tiles = false;       // BSX_NO_UNIFORM_TILES (A/B timing, tests: every mask tile on the general path), likewise
  bool tail_generic = false;           // BSX_TAIL_GENERIC (tests: the scalar argmax scan of the DeepLab tail), likewise
  // Lanes (BSX_LANES=k, experiment): the fused step splits its batch into k contiguous groups of streams and runs each group's launch sequence on its own
  // HIP stream — streams are independent, so the HBM-bound tail of one group (mask + blend) can overlap the latency-bound network kernels of another.
  int lanes = 1;
  hipStream_t lane_stream[4] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t ev_fork = nullptr, ev_join[4] = {nullptr, nullptr, nullptr, nullptr};
  // Two-deep pipeline (bsx_step_batch_pipelined): the composite of the batch handed over by the PREVIOUS call (mask up-scale + blur + alpha blend: HBM-bound) runs
  // on comp_stream while the caller's stream runs the mask pipeline of THIS call's batch (prep → network: latency-bound) — the batch-level form of the reference's
  // CalcMask worker thread next to its capture / blend loop (app/deepseg.cc:159-285, 634-661).  The one shared object is the model-resolution temporal state:
  // the kernel that advances it (tail / argmax tail / decode) waits for ev_pcomp first (state_write_fence).
  struct PendingComposite { bool active = false; const uint8_t* frames = nullptr; const uint8_t* bg = nullptr; size_t bg_stride = 0; uint8_t* out = nullptr; int n = 0; unsigned flags = 0; } pend;
  hipStream_t comp_stream = nullptr;
  hipEvent_t ev_pdone = nullptr, ev_pcomp = nullptr;   // ev_pdone: end of the mask pipeline of the PENDING batch, recorded on the stream of the call that enqueued it — the composite
                                                       // (and the next call's network) wait for THAT event, so a caller may alternate streams between calls
  hipEvent_t wait_before_state = nullptr;   // consumed by the next launch that writes d_ofinal
  int pipe_wgs = 0;                         // BSX_PIPE_WGS (read at bsx_new, experiment): workgroups per CU the pipelined composite may hold (occupancy cap by an LDS pad; 0 = no cap,
                                            // the default: every cap measured slower — the tile kernel needs its waves, profiles/r04l)
  // Stream ids of bsx_step_batch_streams / bsx_reset_streams: the host array is copied into the next entry of a pinned ring, from there into the same entry of a device
  // ring that the call's kernels read (slot_of).  An entry is reused only after the event recorded behind the call that used it has completed — with kIdRing entries
  // the host waits only when it runs more than kIdRing calls ahead of the GPU.  Allocated on the first call (n_streams ints per entry).
  static constexpr int kIdRing = 4;
  int* h_ids = nullptr;                     // pinned [kIdRing][n_streams]
  int* d_ids = nullptr;                     // device [kIdRing][n_streams]
  hipEvent_t ev_ids[kIdRing] = {};
  bool ids_used[kIdRing] = {};
  int ids_next = 0;
  std::vector<int> ids_seen;                // host scratch of the duplicate check: [n_streams], -1 = not listed
  // bsx_step_batch_mixed: per ring entry (the same entries and events as the ids) the batch's descriptor table — n MixDesc (kernels.hpp), then the positions of its
  // blur streams grouped by blur size (ints) — built in the pinned entry, copied to the device entry in one hipMemcpyAsync.  Allocated on the first mixed call.
  uint8_t* h_mix = nullptr;                 // pinned [kIdRing][n_streams * (16 + 4)]
  uint8_t* d_mix = nullptr;                 // device, likewise
  struct MixBlur { int ksize, off, count; };
  std::vector<MixBlur> mix_blur;            // the staged call's blur groups: ksize, first index into the position list, count
  size_t mix_entry_bytes() const { return (size_t)n_streams * (sizeof(MixDesc) + sizeof(int)); }
  // The n-picture image batches (bsx_resize_bgr_batch, bsx_gaussian_blur_bgr_batch, bsx_gaussian_blur_surfaces_batch, bsx_resize_surfaces_batch): per ring entry
  // (the same entries and events again) the call's n_streams descriptors (kernels.hpp: ResizeBatchDesc, BlurDesc, BlurSurfDesc, ResizeSurfDesc) in the plan's order,
  // built in the pinned entry, copied to the device entry in one hipMemcpyAsync.  A ring is allocated on its call's first use (picture_batch_run).
  struct DescRing { void* h = nullptr; void* d = nullptr; };      // pinned [kIdRing][n_streams] descriptors of the call's type; device, likewise
  DescRing rsz_ring, blur_ring, blur_surf_ring, rsz_surf_ring;
  GaussCoef* d_blur_coef = nullptr;         // device [blur_coef_table_bytes()]: the coefficient records of every (ksize, staging path), uploaded by the first call of either blur batch
  PictureBatchPlan pic_plan;                // host scratch: the plan of the call (picture_batch_plan.hpp)
  // Geometry classes (bsx_new_geoms): class 0 IS the context's own geometry — width, height, roi, in_roi, both tables and the first bytes of d_masks above — so every
  // one-geometry path reads what it always read; classes 1.. add their own ROIs and tables and their own slice of the ONE d_masks allocation.  Streams are numbered
  // class after class.  Model-side state (ofinal by slot, arena, network buffers, weights, kernels) exists once.  bsx_step_batch_geoms advances streams of any mix of
  // classes in one launch sequence (kernels.hpp: GeomClass / GeomDesc / GeomSpans); every other stepping entry point refuses a context with more than one class.
  struct Geom {
    int width = 0, height = 0, n_streams = 0, first = 0;
    Rect4 roi{}, in_roi{};
    DevResizeTab tab_down, tab_up;     // class 0: copies of the context's (the device memory is owned there)
    size_t mask_offset = 0, tiles_per_frame = 0;
    int outside_blocks = 0;            // outside-ROI workgroups of one position (0: the ROI is the frame)
    bool fusable = false, xcd = false; // on the fused tile route (geom_class_fusable); mask tiles of a frame on one XCD (geom_class_xcd)
    // a context made with BSX_GEOMS_EDGE_ROI: `edge` = roi.x or roi.w is off the 4-pixel grid — the geoms step then tiles the class in frame-anchored columns
    // (tiles_per_frame counts those; kernels.hpp: launch_mask_blend_geoms_edge), the vcam step in ROI-anchored ones (vg_tiles_per_frame)
    bool edge = false, shifted_tiles_fit = false;
    size_t vg_tiles_per_frame = 0;
  };
  std::vector<Geom> geoms;
  bool edge_roi = false;                    // made by bsx_new_geoms_ex with BSX_GEOMS_EDGE_ROI
  GeomClass* d_geom_classes_vg = nullptr;   // the class records with ROI-anchored tile columns, where a class is `edge` (else the vcam step reads d_geom_classes)
  size_t mask_bytes = 0;                    // the whole d_masks allocation
  GeomClass* d_geom_classes = nullptr;      // device copy of the class records (uploaded by bsx_new_geoms; for a one-class context on its first geoms step)
  uint8_t* d_geom_tile_class = nullptr;     // one byte per workgroup of the largest ragged tile grid (every stream of every class) + 4; null: BSX_NO_UNIFORM_TILES
  GeomDesc* h_geo = nullptr;                // pinned [kIdRing][geo_entry_bytes()]: the descriptors of a geoms step, ordered by class (the ring entries and events of the ids)
  GeomDesc* d_geo = nullptr;                // device, likewise
  // an entry: n_streams GeomDesc, then room for n_streams VgSurfRec — bsx_step_batch_surfaces puts its n surface records right behind its n descriptors, so that
  // its copy is one too
  size_t geo_entry_bytes() const { return (size_t)n_streams * (sizeof(GeomDesc) + sizeof(VgSurfRec)); }
  GeomDesc* geo_entry(GeomDesc* ring, int k) const { return reinterpret_cast<GeomDesc*>(reinterpret_cast<uint8_t*>(ring) + (size_t)k * geo_entry_bytes()); }
  GeomsChecked geo_checked;                 // host scratch of the multi-geometry steps: what geoms_check leaves (geoms_request.hpp)
  std::vector<int> geo_order, geo_ids;      // host scratch: the call's positions ordered by class, their stream ids in that order
  // bsx_step_batch_vcam_geoms: per output size the device array of one VgClass per class (kernels.hpp) — capture size, capture -> output table, per-tap bit — built
  // and uploaded on the first call at that size.  Class 0's table is the one in vcam_tabs (shared with bsx_step_batch_vcam); the others' memory is owned here.
  struct VgGeoms { VgClass* d_rec = nullptr; std::vector<void*> mem; std::vector<VgClass> h_rec; };      // h_rec: the host's copy (bsx_step_batch_vcam_geoms_outs stages group records from it)
  std::map<std::pair<int, int>, VgGeoms> vg_geoms;
  // bsx_step_batch_vcam_geoms_outs: per ring entry (the same entries and events as the ids) the call's group records — kMaxOutGroups VgOutGroup — then its output
  // descriptors, at most BSX_MAX_OUTS_PER_ITEM * n_streams GeomDesc in group order, built in the pinned entry and copied to the device entry in one hipMemcpyAsync.
  // Allocated on the first call of that entry point.  bsx_step_batch_vcam_geoms_outs_nv12 uses the same entries: behind the call's m descriptors its m plane
  // records (VgNv12Rec, in the same order), so that its copy is one too.
  uint8_t* h_vo = nullptr;                  // pinned [kIdRing][vo_entry_bytes()]
  uint8_t* d_vo = nullptr;                  // device, likewise
  size_t vo_entry_bytes() const { return (size_t)kMaxOutGroups * sizeof(VgOutGroup) + (size_t)BSX_MAX_OUTS_PER_ITEM * (size_t)n_streams * (sizeof(GeomDesc) + sizeof(VgNv12Rec)); }
  std::vector<int> vo_pos;                  // host scratch: the position (place in the class-ordered descriptors) of each item
  int geom_of(int stream) const { int g = 0; while (g + 1 < (int)geoms.size() && stream >= geoms[g + 1].first) g++; return g; }
  bool act16 = false;                  // BSX_ACT16=1: 16-bit activation STORAGE for the segmented Meet / MLKit networks (g1) — opt-in, IoU-gated; needs the specialised middle kernel

  // stream-0 view of a graph tensor (network input/output have dedicated buffers; intermediates are batch-major in
  // the per-launch path and frame-major — frame 0 first — in the per-frame program)
  float* tensor_ptr(int t) const {
    if (t == plan.input) return d_net_in;
    if (t == plan.output) return d_net_out;
    return use_program ? d_arena + plan.tensor_off[t] : d_arena + (size_t)plan.tensor_off[t] * (size_t)n_streams;
  }
};

namespace {

// HIP's current device is per THREAD and defaults to 0: the reference application creates the context on its main thread
// (app/deepseg.cc:246) and calls bs_maskgen_process on a worker thread (:203,258), so every entry point that touches the
// GPU switches to the context's device for its duration and restores the caller's device afterwards.
struct DeviceGuard {
  int prev = -1, dev;
  explicit DeviceGuard(int d) : dev(d) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; if (prev != dev) (void)hipSetDevice(dev); }
  ~DeviceGuard() { if (prev >= 0 && prev != dev) (void)hipSetDevice(prev); }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

void report(bsx_ctx* c, bsx_debug_fn fn, void* user, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->last_error = buf;
  g_last_error = buf;
  if (fn) fn(user, buf); else fputs(buf, stderr);   // same routing as _dbg(), lib/libbackscrub.cc:72-83
}

#define BSX_HIP(c, expr)                                                                                    \
  do {                                                                                                      \
    hipError_t e_ = (expr);                                                                                 \
    if (e_ != hipSuccess) {                                                                                 \
      report((c), (c) ? (c)->ondebug : nullptr, (c) ? (c)->caller_ctx : nullptr, "error: HIP %s at %s:%d (%s)\n", \
             hipGetErrorString(e_), __FILE__, __LINE__, #expr);                                             \
      return BSX_EDEVICE;                                                                                   \
    }                                                                                                       \
  } while (0)

int upload_tab(bsx_ctx* c, const HostResizeTab& h, DevResizeTab* d) {
  d->tab.sw = h.sw; d->tab.sh = h.sh; d->tab.dw = h.dw; d->tab.dh = h.dh; d->tab.mode = h.mode;
  if (h.mode != 0) return BSX_OK;
  d->tab.tile_ok = (mask_tile_fits(h.xofs.data(), h.yofs.data(), h.sw, h.sh, h.dw, h.dh) && !c->no_mask_tile) ? 1 : 0;
  d->tab.tile_class = nullptr;
  size_t b_xofs = h.xofs.size() * 4, b_yofs = h.yofs.size() * 4, b_xa = h.xa.size() * 2, b_ya = h.ya.size() * 2;
  auto up16 = [](size_t v) { return (v + 15) / 16 * 16; };
  size_t total = up16(b_xofs) + up16(b_yofs) + up16(b_xa) + up16(b_ya);
  BSX_HIP(c, hipMalloc(&d->mem, total));
  char* p = (char*)d->mem;
  BSX_HIP(c, hipMemcpy(p, h.xofs.data(), b_xofs, hipMemcpyHostToDevice)); d->tab.xofs = (const int*)p; p += up16(b_xofs);
  BSX_HIP(c, hipMemcpy(p, h.yofs.data(), b_yofs, hipMemcpyHostToDevice)); d->tab.yofs = (const int*)p; p += up16(b_yofs);
  BSX_HIP(c, hipMemcpy(p, h.xa.data(), b_xa, hipMemcpyHostToDevice)); d->tab.xa = (const short*)p; p += up16(b_xa);
  BSX_HIP(c, hipMemcpy(p, h.ya.data(), b_ya, hipMemcpyHostToDevice)); d->tab.ya = (const short*)p;
  return BSX_OK;
}

int model_type_from_name(const std::string& n) {  // lib/libbackscrub.cc:116-130 (same precedence)
  if (n.find("body-pix") != n.npos) return BSX_MODEL_BODYPIX;
  if (n.find("deeplab") != n.npos) return BSX_MODEL_DEEPLAB;
  if (n.find("segm_") != n.npos) return BSX_MODEL_MEET;
  if (n.find("selfie") != n.npos) return BSX_MODEL_MLKIT;
  return BSX_MODEL_UNKNOWN;
}

// what bsx_step_batch_geoms needs on the device beyond the context's own state: the class records, the class bytes of the ragged tile grid, the descriptor ring.
// Idempotent: bsx_new_geoms calls it for a context of several classes, the first geoms step of a one-class context does (like h_mix: allocated on first use).
int geoms_device_state(bsx_ctx* c) {
  if (c->d_geo) return BSX_OK;
  const size_t G = c->geoms.size();
  std::vector<GeomClass> rec(G), rec_vg(G);
  size_t tiles = 0;
  bool any_edge = false;
  for (size_t g = 0; g < G; g++) {
    const bsx_ctx::Geom& q = c->geoms[g];
    rec[g] = GeomClass{q.width, q.height, geom_tile_cols(q.roi, q.edge), (q.roi.h + mask_tile_height() - 1) / mask_tile_height(), q.roi, q.in_roi,
                       q.tab_down.tab, q.tab_up.tab};
    rec_vg[g] = rec[g];
    rec_vg[g].ntx = geom_tile_cols(q.roi, false);
    any_edge = any_edge || q.edge;
    tiles += (size_t)q.n_streams * q.tiles_per_frame;                // (frame-anchored columns are never fewer than ROI-anchored ones: one scratch serves both steps)
  }
  if (!c->d_geom_classes) {
    BSX_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->d_geom_classes), G * sizeof(GeomClass)));
    BSX_HIP(c, hipMemcpy(c->d_geom_classes, rec.data(), G * sizeof(GeomClass), hipMemcpyHostToDevice));
  }
  if (any_edge && !c->d_geom_classes_vg) {
    BSX_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->d_geom_classes_vg), G * sizeof(GeomClass)));
    BSX_HIP(c, hipMemcpy(c->d_geom_classes_vg, rec_vg.data(), G * sizeof(GeomClass), hipMemcpyHostToDevice));
  }
  if (!c->no_uniform_tiles && !c->d_geom_tile_class) {
    BSX_HIP(c, hipMalloc(&c->d_geom_tile_class, tiles + 4));        // (+4: the tile kernel reads the aligned word around a byte)
    BSX_HIP(c, hipMemset(c->d_geom_tile_class, 0, tiles + 4));
  }
  if (!c->h_geo) BSX_HIP(c, hipHostMalloc(reinterpret_cast<void**>(&c->h_geo), bsx_ctx::kIdRing * c->geo_entry_bytes(), hipHostMallocDefault));
  BSX_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->d_geo), bsx_ctx::kIdRing * c->geo_entry_bytes()));
  return BSX_OK;
}

int init_device_state(bsx_ctx* c) {
  BSX_HIP(c, hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
  const size_t N = (size_t)c->n_streams;
  BSX_HIP(c, hipMalloc(&c->d_arena, c->plan.arena_floats_per_stream * N * sizeof(float)));
  BSX_HIP(c, hipMalloc(&c->d_net_in, N * c->inW * c->inH * c->inC * sizeof(float)));
  BSX_HIP(c, hipMalloc(&c->d_net_in_u8, N * c->inW * c->inH * sizeof(uint32_t)));
  BSX_HIP(c, hipMalloc(&c->d_net_out, N * c->outW * c->outH * c->outC * sizeof(float)));
  BSX_HIP(c, hipMalloc(&c->d_weights, std::max<size_t>(c->plan.weights.size(), 4) * sizeof(float)));
  BSX_HIP(c, hipMemcpy(c->d_weights, c->plan.weights.data(), c->plan.weights.size() * sizeof(float), hipMemcpyHostToDevice));
  BSX_HIP(c, hipMalloc(&c->d_weights16, std::max<size_t>(c->plan.weights16.size(), 8) * sizeof(uint16_t)));
  BSX_HIP(c, hipMemcpy(c->d_weights16, c->plan.weights16.data(), c->plan.weights16.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
  // off = f32 MFMA; fast = plain f16 operands (1 term); fast16 = fast + the depthwise outputs of the fused blocks STORED as f16 (bit 4: kernels.hpp)
  if (const char* m = getenv("BSX_F16_GEMM")) c->f16_terms = !strcmp(m, "off") ? 0 : (!strcmp(m, "fast") ? 1 : (!strcmp(m, "fast16") ? 17 : 3));
  // The per-frame program pays off when most tensors stay in LDS (Meet / MLKit families); graphs whose tensors mostly
  // spill (DeepLab: 33x33x480) run faster as one batch-wide launch per step.  BSX_FORCE_FRAME_PROGRAM / BSX_NO_FRAME_PROGRAM override.
  c->use_program = !c->plan.program.empty() && BSX_DBG_ENV("BSX_NO_FRAME_PROGRAM") == nullptr &&
                   (c->plan.seg.on || c->plan.program_lds_tensors >= c->plan.program_global_tensors || BSX_DBG_ENV("BSX_FORCE_FRAME_PROGRAM") != nullptr);
  hipDeviceProp_t prop;                       // the architecture the graph-specialised kernels are compiled for (below)
  const bool have_prop = c->use_program && !BSX_DBG_ENV("BSX_NO_RTC") && hipGetDeviceProperties(&prop, c->device) == hipSuccess;
  const KernelVariant v = kernel_variant(c->plan);
  if (c->use_program) {
    BSX_HIP(c, hipMalloc(&c->d_program, c->plan.program.size() * sizeof(MicroOp)));
    BSX_HIP(c, hipMemcpy(c->d_program, c->plan.program.data(), c->plan.program.size() * sizeof(MicroOp), hipMemcpyHostToDevice));
    BSX_HIP(c, frame_program_prepare(c->plan.program_lds_floats));
    if (c->plan.seg.on) BSX_HIP(c, seg_prepare());
    // Specialise the program and the segment kernels to this graph: straight-line code with compile-time geometry instead of the interpreted micro-op table, the
    // segment kernels' source with this plan's descriptors as compile-time constants.  Compiled by hipRTC for this device's architecture (cached on disk;
    // bsx_model_precompile fills the cache without a GPU).  Anything that goes wrong leaves the interpreter / the ahead-of-time kernels in charge — never an error.
    c->act16 = v.act16;
    if (BSX_DBG_ENV("BSX_NO_RTC")) no_specialised("BSX_NO_RTC", &c->kern);
    else if (!have_prop) no_specialised("no device properties", &c->kern);
    else load_specialised(build_specialised(c->plan, v, prop.gcnArchName), &c->kern);
    if (c->act16 && !c->kern.mid) {          // the interpreter has f32 tensors only: the mode needs the generated kernel
      c->last_error = "BSX_ACT16: the specialised middle kernel is not available (" + c->kern.mid_note + ")";
      return BSX_EDEVICE;
    }
    if (c->act16) c->kern.mid_note += ", 16-bit activation storage";
  } else {
    BSX_HIP(c, nn_prepare());                 // per-launch path: the fused kernels' dynamic-LDS limits on this device
  }
  if (const char* l = BSX_DBG_ENV("BSX_PIPE_WGS")) c->pipe_wgs = std::min(8, std::max(0, atoi(l)));
  if (const char* l = BSX_DBG_ENV("BSX_LANES")) c->lanes = std::min(4, std::max(1, atoi(l)));
  if (c->lanes > 1) {
    BSX_HIP(c, hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    for (int k = 1; k < c->lanes; k++) {
      BSX_HIP(c, hipStreamCreateWithFlags(&c->lane_stream[k], hipStreamNonBlocking));
      BSX_HIP(c, hipEventCreateWithFlags(&c->ev_join[k], hipEventDisableTiming));
    }
  }
  // stems with a byte path take the 8-bit network input: the segmented Meet / MLKit head and DeepLab's fused head kernel
  if (BSX_DBG_ENV("BSX_NO_GRAPH")) c->graph_state = -1;
  c->in_u8 = v.u8in && ((c->use_program && c->plan.seg.on) || (!c->use_program && head0_u8_ok(c->plan)));
  BSX_HIP(c, hipMalloc(&c->d_ofinal, N * c->outW * c->outH));
  BSX_HIP(c, hipMalloc(&c->d_masks, c->mask_bytes));                       // (one geometry: N * width * height)
  BSX_HIP(c, hipMemset(c->d_ofinal, 0, N * c->outW * c->outH));            // :257 leaves it uninitialised; defined as 0
  BSX_HIP(c, hipMemset(c->d_masks, 255, c->mask_bytes));                   // :248
  // bilateralFilter(d=5, sigmaColor=100, sigmaSpace=100) tables (OpenCV bilateral_filter):
  {
    const double sigma_color = 100.0, sigma_space = 100.0;
    const double gc = -0.5 / (sigma_color * sigma_color), gs = -0.5 / (sigma_space * sigma_space);
    const int radius = 2;
    std::vector<float> lut(768);
    for (int i = 0; i < 768; i++) lut[i] = (float)std::exp(i * i * gc);
    BSX_HIP(c, hipMalloc(&c->d_color_lut, 768 * sizeof(float)));
    BSX_HIP(c, hipMemcpy(c->d_color_lut, lut.data(), 768 * sizeof(float), hipMemcpyHostToDevice));
    int k = 0;
    for (int i = -radius; i <= radius; i++) for (int j = -radius; j <= radius; j++) {
      double r = std::sqrt((double)i * i + (double)j * j);
      if (r > radius) continue;
      c->bilateral.space_w[k] = (float)std::exp(r * r * gs);
      c->bilateral.off_y[k] = i; c->bilateral.off_x[k] = j;
      k++;
    }
    c->bilateral.color_lut = c->d_color_lut;
    c->bilateral.scale = c->norm_scale; c->bilateral.offset = c->norm_offset;
    if (k != 13 || !bilateral_taps_match(c->bilateral)) { c->last_error = "bilateral tap table does not match the kernel"; return BSX_EDEVICE; }
  }
  int rc = upload_tab(c, make_resize_tab(c->roi.w, c->roi.h, c->in_roi.w, c->in_roi.h), &c->tab_down);
  if (rc) return rc;
  rc = upload_tab(c, make_resize_tab(c->in_roi.w, c->in_roi.h, c->roi.w, c->roi.h), &c->tab_up);
  if (rc) return rc;
  // one class byte per (stream, mask tile) for the tile kernel's uniform-tile shortcut (kernels_img.hip: tile_class_k); absent = every tile on the general path
  c->tiles_per_frame = (size_t)((c->roi.w + mask_tile_width() - 1) / mask_tile_width()) * (size_t)((c->roi.h + mask_tile_height() - 1) / mask_tile_height());
  if (!c->no_uniform_tiles && c->tab_up.tab.mode == 0 && c->tab_up.tab.tile_ok && c->geoms.size() <= 1) {      // (several classes: only the geoms step runs, with its own)
    BSX_HIP(c, hipMalloc(&c->d_tile_class, N * c->tiles_per_frame + 4));          // (+4: the tile kernel reads the aligned word around a byte)
    BSX_HIP(c, hipMemset(c->d_tile_class, 0, N * c->tiles_per_frame + 4));
    c->tab_up.tab.tile_class = c->d_tile_class;
  }
  // canvas outside in_roi is written as 0 by the prep kernel on every frame (the reference keeps a
  // persistent zeroed in_u8_bgr, :251); nothing else to initialise.
  // geometry classes: class 0 is what was just built; the others get their own tables; with more than one class the device records go up now
  for (size_t g = 0; g < c->geoms.size(); g++) {
    bsx_ctx::Geom& G = c->geoms[g];
    if (g == 0) { G.tab_down = c->tab_down; G.tab_up = c->tab_up; }
    else {
      if ((rc = upload_tab(c, make_resize_tab(G.roi.w, G.roi.h, G.in_roi.w, G.in_roi.h), &G.tab_down))) return rc;
      if ((rc = upload_tab(c, make_resize_tab(G.in_roi.w, G.in_roi.h, G.roi.w, G.roi.h), &G.tab_up))) return rc;
    }
    G.tab_up.tab.tile_class = nullptr;                             // (the geoms step's class bytes travel as a kernel argument)
    G.edge = c->edge_roi && !geom_class_on_grid(G.roi);
    const size_t tile_rows = (size_t)((G.roi.h + mask_tile_height() - 1) / mask_tile_height());
    G.tiles_per_frame = (size_t)geom_tile_cols(G.roi, G.edge) * tile_rows;
    G.vg_tiles_per_frame = (size_t)geom_tile_cols(G.roi, false) * tile_rows;
    G.outside_blocks = geom_outside_blocks(G.width, G.height, G.roi);
    G.fusable = G.edge ? geom_class_edge_fusable(G.width, G.roi, G.tab_up.tab, G.shifted_tiles_fit) : geom_class_fusable(G.width, G.roi, G.tab_up.tab);
    G.xcd = geom_class_xcd(G.width, G.roi);
  }
  if (c->geoms.size() > 1) return geoms_device_state(c);
  return BSX_OK;
}

// NULL means the HIP default (null) stream, exactly as in every HIP API; the context's own
// non-blocking stream is only used by the synchronous host path.
hipStream_t pick(bsx_ctx*, void* s) { return (hipStream_t)s; }

// bsx_profile_batch times launch k of the step from event ev[k - 1] to ev[k] (ev[0]: in front of the first), for as many launches as its table has rows.  The
// launches of the step take a nullable timer: without one the cost is one null-pointer test per launch.
struct LaunchTimer { std::vector<hipEvent_t> ev; int k = 0; ~LaunchTimer() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); } };
int timed(bsx_ctx* c, LaunchTimer* t, hipStream_t s) {
  if (t->k + 1 >= (int)t->ev.size()) { c->last_error = "error: bsx_profile_batch: the step made more launches than the profile counts\n"; return BSX_EDEVICE; }
  BSX_HIP(c, hipEventRecord(t->ev[++t->k], s));
  return BSX_OK;
}
#define BSX_LAUNCH(c, t, s, expr) do { BSX_HIP(c, (expr)); if (t) { const int trc_ = timed(c, t, s); if (trc_) return trc_; } } while (0)

// with_f32: also materialise the f32 input tensor when the stem reads the 8-bit form (the stage-debug entry: tests inspect the tensor)
int run_prep(bsx_ctx* c, const uint8_t* d_frames, int n, hipStream_t s, bool with_f32 = false, bool yuyv_in = false, LaunchTimer* t = nullptr) {
  bsx_roctx::Range range("bsx:prep");
  float* f32 = (!c->in_u8 || with_f32) ? c->tensor_ptr(c->plan.input) : nullptr;
  uint32_t* u8 = c->in_u8 ? c->d_net_in_u8 : nullptr;
  BSX_LAUNCH(c, t, s, launch_prep_fused(d_frames, c->width, c->height, c->roi, f32, u8, c->inW, c->inH, c->in_roi, c->tab_down.tab, c->bilateral, n, s, yuyv_in));
  return BSX_OK;
}
// logits = true: the network output tensor is written (stage tests, the stand-alone decode follows); false: the tail kernel of a
// segmented plan decodes straight into the temporal state of slots [slot, slot + n) and no logits exist
// per-launch path (DeepLab): the graph's final RESIZE_BILINEAR runs fused with the argmax decode + IIR — no full-resolution logits
bool argmax_tail(const bsx_ctx* c) {
  return !c->use_program && !c->keep_logits && c->model_type == BSX_MODEL_DEEPLAB && !c->plan.steps.empty() && c->plan.steps.back().out == c->plan.output &&
         resize_argmax_fusable(c->plan.steps.back());
}
// the middle of a segmented plan / the whole-network program: the specialised kernel when one was built, else the interpreter
hipError_t launch_program(bsx_ctx* c, int n, hipStream_t s, unsigned long long* timeline = nullptr) {
  long pf = (long)c->plan.arena_floats_per_stream;
  if (c->kern.mid) {
    float* arena = c->d_arena;
    const float* weights = c->d_weights;
    void* args[] = {&arena, &pf, &weights, &timeline};
    return hipModuleLaunchKernel(c->kern.mid, (unsigned)n, 1, 1, (unsigned)c->plan.mid_lanes, 1, 1, 0, s, args, nullptr);
  }
  return launch_frame_program(c->d_program, (int)c->plan.program.size(), c->plan.program_lds_floats, c->d_arena, pf, c->d_net_in, c->d_net_out, c->d_weights, n, s,
                              timeline);
}
// bsx_step_batch_pipelined: the launch that advances the temporal state (d_ofinal) waits until the composite of the previous batch — which reads that state on
// comp_stream — has finished.  Called right in front of every such launch; a no-op outside a pipelined call.
int state_write_fence(bsx_ctx* c, hipStream_t s) {
  if (!c->wait_before_state) return BSX_OK;
  hipEvent_t ev = c->wait_before_state;
  c->wait_before_state = nullptr;
  BSX_HIP(c, hipStreamWaitEvent(s, ev, 0));
  return BSX_OK;
}
// does the specialised middle kernel compute micro-op i's arena output chunk by chunk inside the depthwise after it (gen_mid.cpp: the tensor is never stored)?
bool program_op_elided(const bsx_ctx* c, int i) { return c->kern.mid && !BSX_DBG_ENV("BSX_RTC_FINE") && mid_pw_feeds_dw(c->plan, i); }

// Is tensor t — one that debug_tensor_unstored() says this path writes — held as packed halves?  The same predicates as the writers:
//   BSX_ACT16 (segmented frame program): what the segment kernels exchange (H16: Plan::seg_stored) and every arena ACTIVATION operand of the generated middle kernel
//     (generate_mid_source's asp(): convolution, depthwise and resize outputs); a squeeze-excite op's vectors stay f32 (fc_apply stores through sp_of());
//   BSX_F16_GEMM=fast16 (per-launch path): the depthwise output of a fused expand + depthwise pair when ir_out16() held for the last network stage's batch.
// The halves start at the tensor's own arena place (frame-major or batch-major like the f32 form), element i at half i.
bool debug_tensor_half(const bsx_ctx* c, int t) {
  const Plan& p = c->plan;
  if (t == p.input || t == p.output) return false;
  if (c->use_program) {
    if (!c->act16) return false;
    if (p.seg.on && std::find(p.seg_stored.begin(), p.seg_stored.end(), t) != p.seg_stored.end()) return true;
    for (size_t i = 0; i < p.program.size() && i < p.program_out_tensor.size(); i++)
      if (p.program_out_tensor[i] == t) return p.program[i].kind != kMicroSe;
    return false;
  }
  const int n = c->last_net_n > 0 ? c->last_net_n : c->n_streams;
  for (int j = 1; j < (int)p.steps.size(); j++)
    if (p.steps[j].out == t) return p.steps[j - 1].fuse_dw == j && ir_out16(p, p.steps[j - 1], n, c->d_weights16, c->f16_terms, BSX_DBG_ENV("BSX_NO_PW_GEMM") != nullptr);
  return false;
}

// k3 runs in its per-frame form: the plan takes it and the context loaded the specialised module (the ahead-of-time fallback is the tile form and the gate launch)
bool k3_frame_runs(const bsx_ctx* c) { return c->use_program && c->plan.seg.on && c->plan.seg.k3f.on && c->kern.k3_frame != nullptr; }
bool infer_decodes(const bsx_ctx* c) { return (c->use_program && c->plan.seg.on && !c->keep_logits) || argmax_tail(c); }
// ids (device, nullable): the id form of a step — frame i's temporal state is slot ids[i] (then slot == 0); nullptr = slots [slot, slot + n)
int run_infer(bsx_ctx* c, int n, hipStream_t s, bool logits = true, int slot = 0, const int* ids = nullptr, LaunchTimer* t = nullptr) {
  bsx_roctx::Range range("bsx:network");
  c->last_net_n = n;
  c->last_net_logits = logits;
  if (c->arena_poison) {       // (the logits buffer too: a stage that decodes inside its last kernel never writes it, and the entry must not serve the previous stage's)
    BSX_HIP(c, hipMemsetAsync(c->d_arena, 0xFF, c->plan.arena_floats_per_stream * (size_t)c->n_streams * sizeof(float), s));
    BSX_HIP(c, hipMemsetAsync(c->d_net_out, 0xFF, (size_t)c->n_streams * c->outW * c->outH * c->outC * sizeof(float), s));
  }
  if (c->use_program && c->plan.seg.on) {
    // the four segment kernels: the graph-specialised ones where the context loaded them (c->kern.seg), else the ahead-of-time instances
    const SegPlan& sp = c->plan.seg;
    const hipFunction_t* fn = c->kern.seg;
    const long pf = (long)c->plan.arena_floats_per_stream;
    const void* in = c->in_u8 ? (const void*)c->d_net_in_u8 : (const void*)c->d_net_in;
    BSX_LAUNCH(c, t, s, launch_seg_head(fn[0], sp.head, c->d_arena, pf, in, c->d_weights, n, s, c->act16, c->in_u8, c->norm_scale, c->norm_offset));
    BSX_LAUNCH(c, t, s, launch_seg_k2(fn[1], sp.k2, c->d_arena, pf, c->d_weights, n, s, c->act16));
    BSX_LAUNCH(c, t, s, launch_program(c, n, s));
    if (k3_frame_runs(c)) {    // k3's per-frame form: lo, its partial sums and the tail's gate vector in one launch
      BSX_LAUNCH(c, t, s, launch_seg_k3_frame(c->kern.k3_frame, sp.k3f, c->d_arena, pf, c->d_weights, n, s));
    } else {
      BSX_LAUNCH(c, t, s, launch_seg_k3(fn[2], sp.k3, c->d_arena, pf, c->d_weights, n, s, c->act16));
      if (sp.tail.pre_gate_off >= 0) BSX_LAUNCH(c, t, s, launch_seg_gate(sp.tail.gate, c->d_arena, pf, c->d_weights, sp.tail.pre_gate_off, n, s));
    }
    if (!logits) { const int frc = state_write_fence(c, s); if (frc) return frc; }       // the decoding tail reads and writes d_ofinal
    BSX_LAUNCH(c, t, s, launch_seg_tail(fn[3], sp.tail, c->d_arena, pf, c->d_net_out, c->d_ofinal + (size_t)slot * c->outW * c->outH, c->d_weights, logits, n, s,
                                        c->act16, ids));
    return BSX_OK;
  }
  if (c->use_program) {
    BSX_LAUNCH(c, t, s, launch_program(c, n, s));
    return BSX_OK;
  }
  const bool fused_tail = !logits && argmax_tail(c);
  const size_t ns = c->plan.steps.size() - (fused_tail ? 1 : 0);
  for (size_t i = 0; i < ns; i++)
    BSX_LAUNCH(c, t, s, launch_step(c->plan.steps[i], c->plan, c->d_arena, c->d_net_in, c->d_net_out, c->d_weights, n, c->n_streams, s, c->d_weights16, c->f16_terms, c->in_u8 ? c->d_net_in_u8 : nullptr, c->norm_scale, c->norm_offset));
  if (fused_tail) {
    const Step& last = c->plan.steps.back();
    { const int frc = state_write_fence(c, s); if (frc) return frc; }
    BSX_LAUNCH(c, t, s, launch_resize_argmax_iir(last, c->d_arena + (size_t)c->plan.tensor_off[last.in0] * (size_t)c->n_streams,
                                                 c->d_ofinal + (size_t)slot * c->outW * c->outH, n, s, c->tail_generic, ids));
  }
  return BSX_OK;
}
// `slot` = first state slot (stream index) of the batch: frame i uses ofinal / mask slot `slot + i`
int run_decode(bsx_ctx* c, int n, hipStream_t s, int slot = 0, const int* ids = nullptr, LaunchTimer* t = nullptr) {
  bsx_roctx::Range range("bsx:decode");
  { const int frc = state_write_fence(c, s); if (frc) return frc; }
  BSX_LAUNCH(c, t, s, launch_decode(c->model_type, c->tensor_ptr(c->plan.output), c->d_ofinal + (size_t)slot * c->outW * c->outH, c->outW * c->outH, c->outC, n, s, ids));
  return BSX_OK;
}
// the mask up-scale table with its tile-class scratch re-based to stream `slot` (lanes run concurrently on disjoint slot ranges)
ResizeTab tab_up_at(const bsx_ctx* c, int slot) { ResizeTab t = c->tab_up.tab; if (t.tile_class) t.tile_class += (size_t)slot * c->tiles_per_frame; return t; }
int run_mask(bsx_ctx* c, int n, hipStream_t s, int slot = 0, const int* ids = nullptr, LaunchTimer* t = nullptr, uint8_t* masks = nullptr) {
  bsx_roctx::Range range("bsx:mask");
  BSX_LAUNCH(c, t, s, launch_mask_upscale_blur(c->d_ofinal + (size_t)slot * c->outW * c->outH, c->outW, c->outH, c->in_roi, tab_up_at(c, slot),
                                      (masks ? masks : c->d_masks) + (size_t)slot * c->width * c->height, c->width, c->height, c->roi, n, s, ids));
  return BSX_OK;
}
// what follows prep, whichever launch did it: [onprep] → network → [oninfer] → decode (unless the network decodes) for n frames whose state lives in slots
// [slot, slot + n) — or, with ids (device, slot = 0), in slots ids[0..n).  t: bsx_profile_batch's timer (launches only, no callbacks).
int infer_after_prep(bsx_ctx* c, int n, hipStream_t s, int slot, const int* ids, LaunchTimer* t = nullptr) {
  if (c->onprep && !t) { BSX_HIP(c, hipStreamSynchronize(s)); c->onprep(c->caller_ctx); }   // :303
  const bool fused_decode = infer_decodes(c);
  if (const int rc = run_infer(c, n, s, !fused_decode, slot, ids, t)) return rc;
  if (c->oninfer && !t) { BSX_HIP(c, hipStreamSynchronize(s)); c->oninfer(c->caller_ctx); } // :311
  return fused_decode ? BSX_OK : run_decode(c, n, s, slot, ids, t);
}
// prep, then the above.  yuyv_in: YUYV frames (only where prep_yuyv_fusable).
int enqueue_masks(bsx_ctx* c, const uint8_t* d_frames, int n, hipStream_t s, bool yuyv_in, int slot, const int* ids, LaunchTimer* t = nullptr) {
  if (const int rc = run_prep(c, d_frames, n, s, false, yuyv_in, t)) return rc;
  return infer_after_prep(c, n, s, slot, ids, t);
}
// bs_maskgen_process: the masks of n frames into the persistent masks of their slots
// masks: where the full-resolution masks go instead of the persistent ones (run_composite's BSX_STEP_NO_MASK form)
int process_impl(bsx_ctx* c, const uint8_t* d_frames, int n, int slot, hipStream_t s, bool yuyv_in = false, const int* ids = nullptr, uint8_t* masks = nullptr) {
  if (const int rc = enqueue_masks(c, d_frames, n, s, yuyv_in, slot, ids)) return rc;
  if (c->onmask) { BSX_HIP(c, hipStreamSynchronize(s)); c->onmask(c->caller_ctx); }   // :363
  return run_mask(c, n, s, slot, ids, nullptr, masks);
}

// ---- the batch step: every step entry point builds a StepReq, check_step refuses it before anything is enqueued, run_step takes the routes route_of picks -----

// A refused call: its own message (never one an earlier call left), built only here; nothing has been enqueued
int refuse(bsx_ctx* c, const char* fn, const char* fmt, ...) {
  char buf[256];
  va_list ap;                                                     // (only here: messages are built only for a refused call)
  va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
  c->last_error = std::string("error: ") + fn + ": " + buf + "\n";
  return BSX_EINVAL;
}
}  // namespace
// the same for a call made from live.cpp (refusal.hpp): also kept per thread, for the call that has no context to name (bsx_last_error(NULL))
int bsx::refuse_call(bsx_ctx* c, const char* fn, const char* fmt, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
  g_last_error = std::string("error: ") + fn + ": " + buf + "\n";
  if (c) c->last_error = g_last_error;
  return BSX_EINVAL;
}
namespace {
// every entry point that advances the temporal state refuses while the two-deep pipeline holds a composite that reads it
int refuse_pending(bsx_ctx* c, const char* fn) {
  return c->pend.active ? refuse(c, fn, "%s", kPendingComposite) : BSX_OK;
}
// a grid of 2^31 workgroups or more: nothing has been enqueued
int too_many_workgroups(bsx_ctx* c, const char* fn) { c->last_error = std::string("error: ") + fn + ": the batch needs more than 2^31 workgroups\n"; return BSX_EDEVICE; }

// every entry point that works at "the" capture size refuses a context of several geometry classes (bsx_new_geoms): only bsx_step_batch_geoms and bsx_step_batch_vcam_geoms step those
int refuse_geoms(bsx_ctx* c, const char* fn) {
  return c->geoms.size() > 1 ? refuse(c, fn, "context has %d geometries (only bsx_step_batch_geoms and bsx_step_batch_vcam_geoms step such a context)", (int)c->geoms.size()) : BSX_OK;
}

// flags (bsx.h): BSX_STEP_YUYV (the composite leaves as YUYV 4:2:2), BSX_STEP_FLIP_H / _V (cv::flip of the composite), BSX_STEP_NO_MASK, BSX_STEP_YUYV_IN (the
// camera's raw 4:2:2 frames instead of BGR), BSX_STEP_BGBLUR(ksize) (background = blur of the stream's own frame); all folded into the kernels where they apply
struct StepReq {
  const uint8_t* frames; const uint8_t* bg; size_t bg_stride; uint8_t* out;
  int out_w, out_h, n;            // out_w x out_h: the capture size, except for bsx_step_batch_vcam / _vcam_mixed
  unsigned flags; hipStream_t s;
  const int* ids;                 // bsx_step_batch_streams: the DEVICE copy of the stream ids (staged after the checks): frame i's state is slot ids[i]
  const MixDesc* mix = nullptr;   // bsx_step_batch_mixed / _vcam_mixed: the DEVICE descriptor table (staged after the checks) — position i's background / flip / filter-off
  const int* mix_pos = nullptr;   // ... followed by the positions of its blur streams, grouped by blur size (bsx_ctx::mix_blur)
  bool mix_bgr = false;           // ... some position composites over a blur of its frame: a YUYV batch is converted to BGR first
  bool mix_blur_due = false;      // ... blur groups not yet launched (BlurToScratch)
  bool yuyv() const { return (flags & BSX_STEP_YUYV) != 0; }
  bool yin() const { return (flags & BSX_STEP_YUYV_IN) != 0; }
  unsigned flip() const { return flags & (BSX_STEP_FLIP_H | BSX_STEP_FLIP_V); }
  int bgblur() const { return (int)((flags >> 8) & 255u); }
  bool resize(const bsx_ctx* c) const { return out_w != c->width || out_h != c->height; }
  size_t out_bytes() const { return (size_t)n * out_w * out_h * (yuyv() ? 2 : 3); }
  bool out_overlaps(const uint8_t* p, size_t bytes) const { return out < p + bytes && p < out + out_bytes(); }
  bool overlap(const bsx_ctx* c) const { return out_overlaps(frames, (size_t)n * c->width * c->height * (yin() ? 2 : 3)); }
};
enum class Entry { Step, Streams, Vcam, Pipelined, Mixed, VcamMixed };

// The fused tile kernel — mask up-scale + blur + blend [+ flip][+ YUYV pack] per tile, YUYV input converted on load — takes the request: no onmask callback
// (the persistent masks are written by the same launch), the kernel's geometry and alignment, and no overlap it would read after writing
bool tile_fusable(const bsx_ctx* c, const StepReq& r) {
  return !c->onmask && !c->no_mask_blend_fusion && (!r.yuyv() || ((uintptr_t)r.out & 3) == 0) && !(r.overlap(c) && (r.yin() || r.yuyv() || r.flip())) &&
         (!r.yin() || prep_yuyv_fusable(c->width, c->roi, c->tab_down.tab)) &&
         mask_blend_fusable(c->width, c->height, c->roi, r.bg, r.bg_stride, r.frames, r.yuyv() ? r.frames : r.out);
}

// The rules of every step entry point, with their differences: the virtual camera refuses BSX_STEP_NO_MASK and any overlap, the pipeline refuses the blur, any
// overlap and every geometry its fused kernel does not take; the plain step runs in place, and with a flip / YUYV flag on any overlap (through a scratch).
int check_step(bsx_ctx* c, const char* fn, const StepReq& r, Entry kind) {
  const bool vcam = kind == Entry::Vcam, pipe = kind == Entry::Pipelined, blur = r.bgblur() != 0;
  if (kind == Entry::Mixed) {
    // the batch's own rules (the per-position ones ran in mix_check): layout flags only, no overlap at all, the fused tile route's geometry and buffers
    if (!r.frames || !r.out || r.n <= 0 || r.n > c->n_streams) return refuse(c, fn, "null buffer or batch size out of range");
    if (r.flags & ~(BSX_STEP_YUYV | BSX_STEP_NO_MASK | BSX_STEP_YUYV_IN)) return refuse(c, fn, "flags 0x%x has bits outside yuyv / no-mask / yuyv-in", r.flags);
    if (const int rc = refuse_pending(c, fn)) return rc;
    if (r.yuyv() && (c->width & 1)) return refuse(c, fn, "YUYV output needs an even width");
    if (r.yin() && (c->width & 1)) return refuse(c, fn, "YUYV input needs an even capture width");
    if (r.overlap(c)) return refuse(c, fn, "output overlaps the frames (the mixed step has no in-place form)");
    if (c->onmask || !mask_blend_fusable(c->width, c->height, c->roi, nullptr, 0, r.frames, r.out))
      return refuse(c, fn, "needs the fused mask + blend geometry (width, ROI x and width multiples of 4, 4-byte aligned buffers, no onmask callback)");
    return BSX_OK;
  }
  if (kind == Entry::VcamMixed) {
    // the batch's own rules at the virtual camera's geometry: the vcam step's (any capture width, ROI and alignment: its kernel has a byte-wise form and the masks
    // come from process_impl), with the mixed step's layout-only flags; the per-position rules ran in mix_check
    if (!r.frames || !r.out || r.n <= 0 || r.n > c->n_streams) return refuse(c, fn, "null buffer or batch size out of range");
    if (r.flags & BSX_STEP_NO_MASK) return refuse(c, fn, "unsupported flags 0x%x (the no-mask step has no vcam form)", r.flags);
    if (r.flags & ~(BSX_STEP_YUYV | BSX_STEP_YUYV_IN)) return refuse(c, fn, "flags 0x%x has bits outside yuyv / yuyv-in", r.flags);
    if (r.out_w <= 0 || r.out_h <= 0) return refuse(c, fn, "output size %d x %d must be positive", r.out_w, r.out_h);
    if (const int rc = refuse_pending(c, fn)) return rc;
    if (r.yuyv() && (r.out_w & 1)) return refuse(c, fn, "YUYV output needs an even width (out_w = %d)", r.out_w);
    if (r.yin() && (c->width & 1)) return refuse(c, fn, "YUYV input needs an even capture width (width = %d)", c->width);
    if (r.overlap(c)) return refuse(c, fn, "output overlaps the frames (each output pixel reads a neighbourhood of input pixels)");
    return BSX_OK;
  }
  if (!r.frames || (!r.bg && !blur) || !r.out || r.n <= 0 || r.n > c->n_streams) return refuse(c, fn, "null buffer or batch size out of range");
  if ((r.flags & ~(pipe ? 31u : 31u | 0xFF00u)) || (vcam && (r.flags & BSX_STEP_NO_MASK)))
    return refuse(c, fn, vcam ? "unsupported flags (the no-mask step has no vcam form)" : "unsupported flags 0x%x", r.flags);
  if (blur && (r.bgblur() > 31 || !(r.bgblur() & 1))) return refuse(c, fn, "background blur size must be odd and <= 31");
  if (vcam && (r.out_w <= 0 || r.out_h <= 0)) return refuse(c, fn, "output size must be positive");
  if (blur && !vcam && r.frames == r.out) return refuse(c, fn, "the background blur cannot run in place");
  if (!pipe) { if (const int rc = refuse_pending(c, fn)) return rc; }
  if (r.yuyv() && (r.out_w & 1)) return refuse(c, fn, "YUYV output needs an even width");     // 4:2:2 pairs pixels horizontally
  if (r.yin() && (c->width & 1)) return refuse(c, fn, "YUYV input needs an even capture width");
  // vcam: each output pixel reads a neighbourhood of input pixels; pipeline: out(k) is written while frames(k + 1) are read
  const bool overlap = r.overlap(c);
  if (vcam && overlap) return refuse(c, fn, "output overlaps the frames");
  if (vcam && !blur && r.out_overlaps(r.bg, r.bg_stride * (size_t)(r.n - 1) + (size_t)c->width * c->height * 3)) return refuse(c, fn, "output overlaps the background");
  if (pipe && (overlap || c->onprep || c->oninfer || !tile_fusable(c, r)))
    return refuse(c, fn, "needs the fused mask + blend geometry, no stage callbacks and non-overlapping buffers");
  // Aliasing (bsx.h): the reference flips `raw` in place (app/deepseg.cc:667-673), so a caller following it passes d_out == d_frames.  A plain composite in place
  // (same address read, then written, by the same lane) is fine; with a flip or YUYV flag the fused tile kernel would store to addresses another tile has not read
  // yet, so those take the unfused sequence through the context's scratch (tile_fusable); YUYV input is converted into a scratch first.  Partial overlap is refused.
  if (overlap && !r.yin() && !r.yuyv() && !r.flip() && r.out != r.frames) return refuse(c, fn, "output partially overlaps the frames");
  return BSX_OK;
}

// YuyvToBgr: YUYV frames the fused kernels do not read (or the blur needs as BGR) into the BGR scratch, then the BGR form; BlurToScratch: the blurred frames
// into a scratch background, then the step with it; BlurBlend: masks, then blur + blend in one pass; Tile: masks, then mask up-scale + blur + blend per tile in
// ONE launch; Composite: masks, then the plain blend [into a scratch, + flip][+ YUYV pack]; Vcam: masks, then blend + flip + resize [+ pack] in one pass (with
// r.mix: every position by its own descriptor)
enum class Route { YuyvToBgr, BlurToScratch, BlurBlend, Tile, Composite, Vcam };
Route route_of(const bsx_ctx* c, const StepReq& r) {
  if (r.mix) {                    // bsx_step_batch_mixed / _vcam_mixed: [YUYV -> BGR] -> [blur groups into the scratch] -> ONE tile launch / ONE resize-pass launch
    if (r.yin() && (r.mix_bgr || !prep_yuyv_fusable(c->width, c->roi, c->tab_down.tab))) return Route::YuyvToBgr;
    if (r.mix_blur_due) return Route::BlurToScratch;
    return r.resize(c) ? Route::Vcam : Route::Tile;
  }
  const bool resize = r.resize(c);
  if (r.yin() && (r.bgblur() || !(resize ? prep_yuyv_fusable(c->width, c->roi, c->tab_down.tab) : tile_fusable(c, r)))) return Route::YuyvToBgr;
  if (r.bgblur())
    return !resize && !(r.flags & 15u) && !c->no_bgblur_fusion && gauss_blend_fusable(r.frames, c->d_masks, r.out, c->width, r.bgblur()) ? Route::BlurBlend
                                                                                                                                       : Route::BlurToScratch;
  if (resize) return Route::Vcam;
  return tile_fusable(c, r) ? Route::Tile : Route::Composite;
}

// BSX_LANES: the context's batch buffers re-based to streams [f0, f0 + cap) inside the scope; the batch-major arena of the per-launch path becomes a compact one
struct LaneView {
  bsx_ctx* c; float* net_in; uint32_t* net_in_u8; float* net_out; float* arena; int n_streams;
  LaneView(bsx_ctx* ctx, int f0, int cap) : c(ctx), net_in(ctx->d_net_in), net_in_u8(ctx->d_net_in_u8), net_out(ctx->d_net_out), arena(ctx->d_arena), n_streams(ctx->n_streams) {
    c->d_net_in += (size_t)f0 * c->inW * c->inH * c->inC;
    c->d_net_in_u8 += (size_t)f0 * c->inW * c->inH;
    c->d_net_out += (size_t)f0 * c->outW * c->outH * c->outC;
    c->d_arena += (size_t)f0 * c->plan.arena_floats_per_stream;
    c->n_streams = cap;
  }
  ~LaneView() { c->d_net_in = net_in; c->d_net_in_u8 = net_in_u8; c->d_net_out = net_out; c->d_arena = arena; c->n_streams = n_streams; }
};

int run_tile(bsx_ctx* c, const StepReq& r) {
  const size_t fb = (size_t)c->width * c->height * (r.yin() ? 2 : 3), ob = (size_t)c->width * c->height * (r.yuyv() ? 2 : 3), sm = (size_t)c->outW * c->outH;
  // frames [f0, f0 + nb) on stream ls, their state in slots [f0, f0 + nb) or ids[f0 .. f0 + nb); per > 0: a lane, whose buffers are re-based (LaneView)
  auto tile = [&](int f0, int nb, int per, hipStream_t ls) -> int {
    const int st0 = r.ids ? 0 : f0, *lids = r.ids ? r.ids + f0 : nullptr;
    int rc;
    if (per) { LaneView view(c, f0, per); rc = enqueue_masks(c, r.frames + (size_t)f0 * fb, nb, ls, r.yin(), st0, lids); }
    else rc = enqueue_masks(c, r.frames, nb, ls, r.yin(), 0, r.ids);
    if (rc) return rc;
    bsx_roctx::Range range("bsx:mask+blend");
    if (r.mix)
      BSX_HIP(c, launch_mask_blend_mixed(c->d_ofinal + (size_t)st0 * sm, c->outW, c->outH, c->in_roi, tab_up_at(c, f0), c->d_masks + (size_t)st0 * c->width * c->height,
                                         c->width, c->height, c->roi, r.mix + f0, r.frames + (size_t)f0 * fb, r.out + (size_t)f0 * ob, nb, ls, (int)r.flags, lids));
    else
      BSX_HIP(c, launch_mask_blend(c->d_ofinal + (size_t)st0 * sm, c->outW, c->outH, c->in_roi, tab_up_at(c, f0), c->d_masks + (size_t)st0 * c->width * c->height, c->width,
                                   c->height, c->roi, r.bg + (size_t)f0 * r.bg_stride, r.bg_stride, r.frames + (size_t)f0 * fb, r.out + (size_t)f0 * ob, nb, ls, (int)r.flags, 0, lids));
    return BSX_OK;
  };
  // (the per-launch path's arena is batch-major: a lane's compact arena is laid out for `per` streams starting at stream f0, so the LAST lane ends at
  //  K * per streams — lanes are only taken when that still fits the allocation, e.g. not for n = n_streams = 66, K = 4: 4 * 17 = 68)
  const int n = r.n, K = c->lanes, per = (n + K - 1) / std::max(K, 1);
  if (!(K > 1 && n >= 16 * K && !c->onprep && !c->oninfer && !c->keep_logits && (c->use_program || K * per <= c->n_streams))) return tile(0, n, 0, r.s);
  BSX_HIP(c, hipEventRecord(c->ev_fork, r.s));
  int lane_rc = BSX_OK;
  for (int k = 0; k < K && lane_rc == BSX_OK; k++) {
    const int f0 = k * per, nb = std::min(per, n - f0);
    if (nb <= 0) break;
    hipStream_t ls = k == 0 ? r.s : c->lane_stream[k];
    if (k > 0 && hipStreamWaitEvent(ls, c->ev_fork, 0) != hipSuccess) { lane_rc = BSX_EDEVICE; break; }
    lane_rc = tile(f0, nb, per, ls);
    // forked lanes are ALWAYS joined, also after an error: the caller's stream must not be left with work in flight on streams it cannot see
    if (k > 0 && (hipEventRecord(c->ev_join[k], ls) != hipSuccess || hipStreamWaitEvent(r.s, c->ev_join[k], 0) != hipSuccess)) lane_rc = lane_rc ? lane_rc : BSX_EDEVICE;
  }
  if (lane_rc == BSX_EDEVICE && c->last_error.empty()) c->last_error = "error: HIP failure while enqueuing a lane of the step\n";
  return lane_rc;
}

// the unfused geometry: the composite with the persistent masks of the batch's slots, into a context-owned BGR scratch when a flip and / or a pack follows
int run_composite(bsx_ctx* c, const StepReq& r) {
  const size_t px = (size_t)c->width * c->height, need = (size_t)c->n_streams * px * 3;
  // BSX_STEP_NO_MASK (bsx.h): the persistent masks keep what the last storing call wrote — here the blend is a launch of its own and reads the masks from memory, so
  // they go to a scratch that only this route sees (the mask kernels write the ROI; outside it the mask is 255 for good: set once, before the first use)
  uint8_t* masks = c->d_masks;
  if ((r.flags & BSX_STEP_NO_MASK) && !c->onmask) {
    if (!c->d_mask_scratch) {
      BSX_HIP(c, hipMalloc(&c->d_mask_scratch, (size_t)c->n_streams * px));
      BSX_HIP(c, hipMemsetAsync(c->d_mask_scratch, 0xFF, (size_t)c->n_streams * px, r.s));
      BSX_HIP(c, hipStreamSynchronize(r.s));                      // (once per context: a later call may come on another stream)
    }
    masks = c->d_mask_scratch;
  }
  if (const int rc = process_impl(c, r.frames, r.n, 0, r.s, false, r.ids, masks == c->d_masks ? nullptr : masks)) return rc;
  if ((r.yuyv() || r.flip()) && !c->d_bgr_scratch) BSX_HIP(c, hipMalloc(&c->d_bgr_scratch, need));
  uint8_t* dst = (r.yuyv() || r.flip()) ? c->d_bgr_scratch : r.out;
  { bsx_roctx::Range range("bsx:blend"); BSX_HIP(c, launch_blend(r.bg, r.bg_stride, r.frames, masks, dst, px, r.n, r.s, r.ids)); }
  const uint8_t* bgr = dst;
  if (r.flip()) {
    const int code = r.flip() == (BSX_STEP_FLIP_H | BSX_STEP_FLIP_V) ? -1 : (r.flip() == BSX_STEP_FLIP_H ? 1 : 0);
    uint8_t* fdst = r.out;
    if (r.yuyv()) { if (!c->d_bgr_scratch2) BSX_HIP(c, hipMalloc(&c->d_bgr_scratch2, need)); fdst = c->d_bgr_scratch2; }
    BSX_HIP(c, launch_flip_bgr(bgr, fdst, c->width, c->height, code, r.n, r.s));
    bgr = fdst;
  }
  if (r.yuyv()) BSX_HIP(c, launch_bgr_to_yuyv(bgr, r.out, c->width, c->height, r.n, r.s));
  return BSX_OK;
}

// A (sw, sh) -> (dw, dh) table as the resize pass of the vcam kernels takes it: always linear.  The 2x2 area mean becomes taps 2d and 2d + 1 with coefficients
// 1024 / 1024, the copy of equal sizes taps d and d + 1 with 2048 / 0 (the same integers in both cases: kernels_img.hip); `direct`: the tile footprints do not fit
// the kernel's LDS staging area
int vcam_tab_build(bsx_ctx* c, int sw, int sh, int dw, int dh, VcamTab* v) {
  HostResizeTab h = make_resize_tab(sw, sh, dw, dh);
  if (h.mode != 0) {
    const int step = h.mode == 2 ? 2 : 1;
    const short a0 = h.mode == 2 ? 1024 : 2048, a1 = h.mode == 2 ? 1024 : 0;
    h.mode = 0;
    h.xofs.resize(dw); h.xa.resize(2 * (size_t)dw); h.yofs.resize(dh); h.ya.resize(2 * (size_t)dh);
    for (int d = 0; d < dw; d++) { h.xofs[d] = step * d; h.xa[2 * d] = a0; h.xa[2 * d + 1] = a1; }
    for (int d = 0; d < dh; d++) { h.yofs[d] = step * d; h.ya[2 * d] = a0; h.ya[2 * d + 1] = a1; }
  }
  v->direct = !vcam_tile_fits(h.xofs.data(), h.yofs.data(), h.sw, h.sh, h.dw, h.dh);
  const int rc = upload_tab(c, h, &v->d);
  if (rc && v->d.mem) { (void)hipFree(v->d.mem); v->d.mem = nullptr; }
  return rc;
}
// the capture -> (out_w, out_h) table of bsx_step_batch_vcam (class 0 of bsx_step_batch_vcam_geoms), built once per output size
int vcam_tab(bsx_ctx* c, int out_w, int out_h, const VcamTab** out) {
  auto key = std::make_pair(out_w, out_h);
  auto it = c->vcam_tabs.find(key);
  if (it == c->vcam_tabs.end()) {
    VcamTab v;
    if (const int rc = vcam_tab_build(c, c->width, c->height, out_w, out_h, &v)) return rc;
    it = c->vcam_tabs.emplace(key, v).first;
  }
  *out = &it->second;
  return BSX_OK;
}

// a checked request, on the context's device: its route, until the batch is composited (the scratch conversions rewrite the request and decide again)
int run_step(bsx_ctx* c, StepReq r) {
  const size_t px = (size_t)c->width * c->height;
  const VcamTab* vt = nullptr;
  if (r.resize(c)) { if (const int rc = vcam_tab(c, r.out_w, r.out_h, &vt)) return rc; }
  for (;;) {
    switch (route_of(c, r)) {
      case Route::YuyvToBgr:
        if (!c->d_bgr_in_scratch) BSX_HIP(c, hipMalloc(&c->d_bgr_in_scratch, (size_t)c->n_streams * px * 3));
        BSX_HIP(c, launch_yuyv_to_bgr(r.frames, c->d_bgr_in_scratch, c->width, c->height, r.n, r.s));
        r.frames = c->d_bgr_in_scratch; r.flags &= ~BSX_STEP_YUYV_IN;
        continue;
      case Route::BlurToScratch:
        if (r.mix) {              // one launch per blur size over its positions, each blurred frame into the scratch at its position (the descriptors point there)
          for (const bsx_ctx::MixBlur& g : c->mix_blur)
            BSX_HIP(c, launch_gauss_blur(r.frames, c->d_bgblur_scratch, c->width, c->height, g.ksize, g.count, r.s, r.mix_pos + g.off));
          r.mix_blur_due = false;
          continue;
        }
        if (!c->d_bgblur_scratch) BSX_HIP(c, hipMalloc(&c->d_bgblur_scratch, (size_t)c->n_streams * px * 3));
        BSX_HIP(c, launch_gauss_blur(r.frames, c->d_bgblur_scratch, c->width, c->height, r.bgblur(), r.n, r.s));
        r.bg = c->d_bgblur_scratch; r.bg_stride = px * 3; r.flags &= ~0xFF00u;
        continue;
      case Route::BlurBlend:
        if (const int rc = process_impl(c, r.frames, r.n, 0, r.s, false, r.ids)) return rc;
        BSX_HIP(c, launch_gauss_blend(r.frames, c->d_masks, r.out, c->width, c->height, r.bgblur(), r.n, r.s, r.ids));
        return BSX_OK;
      case Route::Tile: return run_tile(c, r);
      case Route::Composite: return run_composite(c, r);
      case Route::Vcam: {
        if (const int rc = process_impl(c, r.frames, r.n, 0, r.s, r.yin(), r.ids)) return rc;
        bsx_roctx::Range range("bsx:vcam");
        if (r.mix)                // (vt->direct holds for every flip combination: vcam_tile_fits)
          BSX_HIP(c, launch_vg_mixed(r.frames, r.yin(), r.mix, c->d_masks, r.ids, r.out, c->width, c->height, vt->d.tab, vt->direct || c->vcam_direct, r.n, r.s,
                                     r.yuyv() ? 1u : 0u));
        else
          BSX_HIP(c, launch_vcam_blend_resize(r.frames, r.yin(), r.bg, r.bg_stride, c->d_masks, r.out, c->width, c->height, vt->d.tab, vt->direct || c->vcam_direct, r.n,
                                              r.s, r.flags & 7u));
        return BSX_OK;
      }
    }
  }
}

// ---- a chosen subset of the context's streams, addressed by stream id (bsx.h): frame i of the call belongs to stream ids[i].  The kernels that read or write
// per-stream state take the ids as a device array (slot_of) and address that state in place; everything else stays indexed by position.

// host-side validation of ids[0..n): nothing is enqueued before it passes
int ids_check(bsx_ctx* c, const char* fn, const int* ids, int n) {
  if (n < 0) return refuse(c, fn, "n = %d is negative", n);
  if (n > c->n_streams) return refuse(c, fn, "n = %d exceeds the context's %d streams", n, c->n_streams);
  if (n > 0 && !ids) return refuse(c, fn, "ids is NULL");
  if (c->ids_seen.size() != (size_t)c->n_streams) c->ids_seen.assign((size_t)c->n_streams, -1);
  int rc = BSX_OK, i = 0;
  for (; i < n; i++) {
    const int v = ids[i];
    if (v < 0 || v >= c->n_streams) { rc = refuse(c, fn, "ids[%d] = %d is out of range [0, %d)", i, v, c->n_streams); break; }
    if (c->ids_seen[v] >= 0) { rc = refuse(c, fn, "ids[%d] = %d repeats ids[%d]", i, v, c->ids_seen[v]); break; }
    c->ids_seen[v] = i;
  }
  for (int j = 0; j < i; j++) c->ids_seen[ids[j]] = -1;
  return rc;
}
// the next entry of the staging ring (bsx_ctx::kIdRing: the ids, the mixed step's descriptors), once the event recorded behind its previous user has completed
int ring_acquire(bsx_ctx* c, int* entry) {
  for (hipEvent_t& e : c->ev_ids) if (!e) BSX_HIP(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  const int k = c->ids_next;
  if (c->ids_used[k]) {
    hipError_t e;
    while ((e = hipEventQuery(c->ev_ids[k])) == hipErrorNotReady) std::this_thread::yield();
    BSX_HIP(c, e);
  }
  c->ids_next = (k + 1) % bsx_ctx::kIdRing;
  *entry = k;
  return BSX_OK;
}
// ids[0..n) → entry k of the pinned ring → the same entry of the device ring, on s
int ids_copy(bsx_ctx* c, const int* ids, int n, hipStream_t s, int k, const int** d_ids) {
  const size_t N = (size_t)c->n_streams;
  if (!c->h_ids) BSX_HIP(c, hipHostMalloc(reinterpret_cast<void**>(&c->h_ids), bsx_ctx::kIdRing * N * sizeof(int), hipHostMallocDefault));
  if (!c->d_ids) BSX_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->d_ids), bsx_ctx::kIdRing * N * sizeof(int)));
  memcpy(c->h_ids + (size_t)k * N, ids, (size_t)n * sizeof(int));
  BSX_HIP(c, hipMemcpyAsync(c->d_ids + (size_t)k * N, c->h_ids + (size_t)k * N, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
  *d_ids = c->d_ids + (size_t)k * N;
  return BSX_OK;
}
// ids[0..n) → the next ring entry, on s; ids_release guards the entry behind the call
int ids_stage(bsx_ctx* c, const int* ids, int n, hipStream_t s, const int** d_ids, int* entry) {
  if (const int rc = ring_acquire(c, entry)) return rc;
  return ids_copy(c, ids, n, s, *entry, d_ids);
}
// the ring entry is free again once everything enqueued on s so far has run (recorded also after a failed call: whatever it enqueued may read the entry)
int ids_release(bsx_ctx* c, int entry, hipStream_t s, int rc) {
  c->ids_used[entry] = true;
  const hipError_t e = hipEventRecord(c->ev_ids[entry], s);
  if (rc == BSX_OK && e != hipSuccess) BSX_HIP(c, e);
  return rc;
}

// ---- bsx_step_batch_mixed: every position with its own background, flip and filter switch (bsx.h), in ONE mask pipeline and ONE tile launch --------------------

constexpr unsigned kStreamFlags = BSX_STEP_FLIP_H | BSX_STEP_FLIP_V | 0xFF00u | BSX_STREAM_FILTER_OFF;
static_assert(BSX_STEP_FLIP_H == kMixFlipH && BSX_STEP_FLIP_V == kMixFlipV && BSX_STREAM_FILTER_OFF == kMixFilterOff, "descriptor flags = the public bits");
inline int setting_blur(const bsx_stream_setting& st) { return (st.flags & BSX_STREAM_FILTER_OFF) ? 0 : (int)((st.flags >> 8) & 255u); }   // 0: no blur to make

// host-side validation of settings[0..n), next to ids_check: nothing is enqueued before it passes.  any_align (the step at the virtual camera's geometry): a
// background may lie at any address — its stream then takes the kernel's byte form
int mix_check(bsx_ctx* c, const char* fn, const bsx_stream_setting* st, const StepReq& r, bool any_align) {
  if (r.n > 0 && !st) return refuse(c, fn, "settings is NULL");
  const size_t img = (size_t)c->width * c->height * 3;
  for (int i = 0; i < r.n; i++) {
    const unsigned f = st[i].flags;
    const int k = (int)((f >> 8) & 255u);
    if (f & ~kStreamFlags) return refuse(c, fn, "settings[%d]: flags 0x%x has bits outside flip / blur / filter-off", i, f);
    if (k && (k > 31 || !(k & 1))) return refuse(c, fn, "settings[%d]: blur size %d must be odd and <= 31", i, k);
    if ((f & BSX_STREAM_FILTER_OFF) || k) continue;               // reads no background
    if (!st[i].d_bg) return refuse(c, fn, "settings[%d]: d_bg is NULL", i);
    if (!any_align && ((uintptr_t)st[i].d_bg & 3)) return refuse(c, fn, "settings[%d]: d_bg %p is not 4-byte aligned", i, (const void*)st[i].d_bg);
    if (r.frames && r.out && r.out_w > 0 && r.out_h > 0 && r.out_overlaps(st[i].d_bg, img)) return refuse(c, fn, "settings[%d]: output overlaps the background %p", i, (const void*)st[i].d_bg);
  }
  return BSX_OK;
}
// the descriptor table of settings[0..n) into ring entry k (pinned), the blur positions grouped by size behind it, one copy to the device entry on r.s.  A blur
// stream's background is its slot of the blur scratch (filled by the BlurToScratch route before the tile launch); blur size 1 is the frame itself.
int mix_stage(bsx_ctx* c, const bsx_stream_setting* st, StepReq& r, int k) {
  const size_t eb = c->mix_entry_bytes(), img = (size_t)c->width * c->height * 3;
  if (!c->h_mix) BSX_HIP(c, hipHostMalloc(reinterpret_cast<void**>(&c->h_mix), bsx_ctx::kIdRing * eb, hipHostMallocDefault));
  if (!c->d_mix) BSX_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->d_mix), bsx_ctx::kIdRing * eb));
  int count[32] = {0};
  for (int i = 0; i < r.n; i++) count[setting_blur(st[i])]++;
  r.mix_bgr = false;
  for (int ks = 1; ks < 32; ks++) r.mix_bgr = r.mix_bgr || count[ks] > 0;
  if (r.mix_bgr && !c->d_bgblur_scratch) BSX_HIP(c, hipMalloc(&c->d_bgblur_scratch, (size_t)c->n_streams * img));
  if (r.mix_bgr && r.yin() && !c->d_bgr_in_scratch) BSX_HIP(c, hipMalloc(&c->d_bgr_in_scratch, (size_t)c->n_streams * img));
  const uint8_t* const bgr = r.yin() ? c->d_bgr_in_scratch : r.frames;     // the BGR frames a blur reads (YuyvToBgr converts a YUYV batch first)
  int next[32] = {0};
  c->mix_blur.clear();
  int npos = 0;
  for (int ks = 3; ks < 32; ks += 2)
    if (count[ks]) { c->mix_blur.push_back({ks, npos, count[ks]}); next[ks] = npos; npos += count[ks]; }
  MixDesc* hd = reinterpret_cast<MixDesc*>(c->h_mix + (size_t)k * eb);
  int* hp = reinterpret_cast<int*>(hd + r.n);
  for (int i = 0; i < r.n; i++) {
    const int ks = setting_blur(st[i]);
    const uint8_t* bg = st[i].d_bg;
    if (st[i].flags & BSX_STREAM_FILTER_OFF) bg = nullptr;
    else if (ks == 1) bg = bgr + (size_t)i * img;                  // GaussianBlur(frame, 1) is the frame
    else if (ks) { bg = c->d_bgblur_scratch + (size_t)i * img; hp[next[ks]++] = i; }
    hd[i] = MixDesc{bg, st[i].flags & (kMixFlipH | kMixFlipV | kMixFilterOff), 0u};
  }
  uint8_t* const dd = c->d_mix + (size_t)k * eb;
  BSX_HIP(c, hipMemcpyAsync(dd, hd, (size_t)r.n * sizeof(MixDesc) + (size_t)npos * sizeof(int), hipMemcpyHostToDevice, r.s));
  r.mix = reinterpret_cast<const MixDesc*>(dd);
  r.mix_pos = reinterpret_cast<const int*>(r.mix + r.n);
  r.mix_blur_due = npos > 0;
  return BSX_OK;
}

// a step entry point: the request checked (ids and settings included) before anything is enqueued, then on the context's device [the ids / descriptors staged]
// and run
int step_call(bsx_ctx* c, const char* fn, Entry kind, StepReq r, const int* host_ids = nullptr, const bsx_stream_setting* settings = nullptr) {
  if (!c) return BSX_EINVAL;
  if (const int rc = refuse_geoms(c, fn)) return rc;
  if (kind != Entry::Vcam && kind != Entry::VcamMixed) { r.out_w = c->width; r.out_h = c->height; }
  if (kind == Entry::VcamMixed && !r.resize(c)) {                 // the capture size: bsx_step_batch_mixed with its own refusals (the no-mask form stays refused)
    if (r.flags & BSX_STEP_NO_MASK) return refuse(c, fn, "unsupported flags 0x%x (the no-mask step has no vcam form)", r.flags);
    kind = Entry::Mixed;
  }
  const bool mixed = kind == Entry::Mixed || kind == Entry::VcamMixed;
  if (kind == Entry::Streams || (mixed && host_ids)) {
    if (const int rc = ids_check(c, fn, host_ids, r.n)) return rc;
  } else if (mixed) {                                             // the dense form: the count rules of ids_check
    if (r.n < 0) return refuse(c, fn, "n = %d is negative", r.n);
    if (r.n > c->n_streams) return refuse(c, fn, "n = %d exceeds the context's %d streams", r.n, c->n_streams);
  }
  if ((kind == Entry::Streams || mixed) && r.n == 0) return refuse_pending(c, fn);   // (check_step refuses a pending composite for n > 0)
  if (mixed) { if (const int rc = mix_check(c, fn, settings, r, kind == Entry::VcamMixed)) return rc; }
  if (const int rc = check_step(c, fn, r, kind)) return rc;
  DeviceGuard guard(c->device);
  if (kind != Entry::Streams && !mixed) return run_step(c, r);
  int entry = 0;
  if (const int rc = ring_acquire(c, &entry)) return rc;
  int rc = BSX_OK;
  if (host_ids) rc = ids_copy(c, host_ids, r.n, r.s, entry, &r.ids);
  if (!rc && mixed) rc = mix_stage(c, settings, r, entry);
  return ids_release(c, entry, r.s, rc ? rc : run_step(c, r));
}

// ---- bsx_resize_bgr / bsx_resize_bgr_batch: the resize tables of the backgrounds, one per distinct (sw, sh, dw, dh), uploaded on first use ---------------------
int bg_tab(bsx_ctx* c, int sw, int sh, int dw, int dh, const DevResizeTab** out) {
  if (const DevResizeTab* t = *out) { if (t->tab.sw == sw && t->tab.sh == sh && t->tab.dw == dw && t->tab.dh == dh) return BSX_OK; }      // (a run of equal sizes looks its table up once)
  auto key = std::make_pair(std::make_pair(sw, sh), std::make_pair(dw, dh));
  auto it = c->bg_tabs.find(key);
  if (it == c->bg_tabs.end()) {
    DevResizeTab d;
    int rc = upload_tab(c, make_resize_tab(sw, sh, dw, dh), &d);
    if (rc) return rc;
    it = c->bg_tabs.emplace(key, d).first;
  }
  *out = &it->second;
  return BSX_OK;
}

// ---- the n-picture image batches: n pictures of their own sizes in ONE launch ----------------------------------------------------------------------------------------
// the context's ONE device copy of blur_coef_table, made by the first call of either blur batch
int blur_coef_upload(bsx_ctx* c) {
  if (c->d_blur_coef) return BSX_OK;
  std::vector<uint8_t> tab(blur_coef_table_bytes(), 0);
  blur_coef_table(reinterpret_cast<GaussCoef*>(tab.data()));
  GaussCoef* dev = nullptr;
  BSX_HIP(c, hipMalloc(reinterpret_cast<void**>(&dev), tab.size()));
  const hipError_t e = hipMemcpy(dev, tab.data(), tab.size(), hipMemcpyHostToDevice);      // (once per context: complete before the first launch on any stream)
  if (e != hipSuccess) { (void)hipFree(dev); BSX_HIP(c, e); }
  c->d_blur_coef = dev;
  return BSX_OK;
}
// a plan's ragged grid as the launchers take it by value
struct PictureGrid { GeomSpans spans{}; BlurTileCols cols{}; ResizeDstSizes sizes{}; };
PictureGrid picture_grid(const PictureBatchPlan& p) {
  static_assert(kPbMaxSizes == kMaxGeoms, "the plan's arrays are GeomSpans', BlurTileCols' and ResizeDstSizes'");
  PictureGrid g;
  for (int k = 0; k <= kMaxGeoms; k++) { g.spans.pos[k] = p.pos[k]; g.spans.wg[k] = p.wg[k]; }
  for (int k = 0; k < kMaxGeoms; k++) { g.spans.per[k] = p.per[k]; g.cols.ntx[k] = p.ntx[k]; g.sizes.dw[k] = p.sizes[k][0]; g.sizes.dh[k] = p.sizes[k][1]; }
  return g;
}
// Ring entry k of a planned call: the ring and, with `coef`, the blur coefficients on first use; fill(i, &desc) for the items in the plan's order into the pinned
// entry (a resize uploads a table it meets for the first time); ONE copy to the device entry on s; launch(descriptors, grid, s)
template <class Desc, class Fill, class Launch>
int picture_batch_run(bsx_ctx* c, bsx_ctx::DescRing* ring, bool coef, const char* doing, hipStream_t s, int k, Fill fill, Launch launch) {
  const size_t N = (size_t)c->n_streams;
  if (!ring->h) BSX_HIP(c, hipHostMalloc(&ring->h, bsx_ctx::kIdRing * N * sizeof(Desc), hipHostMallocDefault));
  if (!ring->d) BSX_HIP(c, hipMalloc(&ring->d, bsx_ctx::kIdRing * N * sizeof(Desc)));
  if (coef) { if (const int rc = blur_coef_upload(c)) return rc; }
  Desc* const hd = static_cast<Desc*>(ring->h) + (size_t)k * N;
  Desc* const dd = static_cast<Desc*>(ring->d) + (size_t)k * N;
  const std::vector<int>& order = c->pic_plan.order;
  for (size_t q = 0; q < order.size(); q++) { if (const int rc = fill(order[q], &hd[q])) return rc; }
  BSX_HIP(c, hipMemcpyAsync(dd, hd, order.size() * sizeof(Desc), hipMemcpyHostToDevice, s));
  const hipError_t e = launch(dd, picture_grid(c->pic_plan), s);
  if (e != hipSuccess) { report(c, c->ondebug, c->caller_ctx, "error: HIP %s while %s\n", hipGetErrorString(e), doing); return BSX_EDEVICE; }
  return BSX_OK;
}
// The one path of the four entry points, their items planned into c->pic_plan (picture_batch_plan.hpp: nothing is enqueued before the plan passes): the plan's
// result, the empty batch, then on the context's device a ring entry and the run.  The entry points only plan and name their ring, fill and launch.
template <class Desc, class Fill, class Launch>
int picture_batch_call(bsx_ctx* c, const char* fn, int planned, bsx_ctx::DescRing* ring, bool coef, const char* doing, void* stream, Fill fill, Launch launch) {
  if (planned == PictureBatchPlan::kRefused) return refuse(c, fn, "%s", c->pic_plan.text);
  if (planned == PictureBatchPlan::kTooLarge) return too_many_workgroups(c, fn);
  if (c->pic_plan.order.empty()) return BSX_OK;
  DeviceGuard guard(c->device);
  hipStream_t s = pick(c, stream);
  int entry = 0;
  if (const int rc = ring_acquire(c, &entry)) return rc;
  return ids_release(c, entry, s, picture_batch_run<Desc>(c, ring, coef, doing, s, entry, fill, launch));
}

// ---- bsx_step_batch_geoms: streams of any mix of geometry classes in ONE prep launch, ONE network pass, ONE tile-class and ONE tile launch ----------------------
// Checked on the host (geoms_call: the ids, then geoms_request.hpp's geoms_check), then: the positions ordered by class, their ids and descriptors
// through the staging ring, the per-class spans of the ragged grids by value in the kernel arguments.
static_assert(BSX_STREAM_YUYV_IN == kGeomYuyvIn, "descriptor flags = the public bits");

// does any item of the call bring a YUYV frame?  Then the call takes the launchers whose kernels read the format per position (kernels.hpp: launch_*_geoms_fmt)
inline bool geoms_any_yuyv(const bsx_geom_item* items, int n) {
  for (int i = 0; i < n; i++) if (items[i].setting.flags & BSX_STREAM_YUYV_IN) return true;
  return false;
}
// the class records of the vcam steps: ROI-anchored tile columns where a class is `edge`
const GeomClass* vg_classes(const bsx_ctx* c) { return c->d_geom_classes_vg ? c->d_geom_classes_vg : c->d_geom_classes; }

// The front of a checked geoms call on the context's device, ring entry k acquired: the positions ordered by class, ids and descriptors through the ring, ONE prep
// launch and the network.  Leaves the descriptors' device copy, the ragged grids of the back end and the classes whose tiles keep to one XCD.
// edge: some position's class is off the 4-pixel grid (bsx_new_geoms_ex) — the geoms step then takes launch_mask_blend_geoms_edge
struct GeomsStaged { const GeomDesc* desc = nullptr; GeomSpans tiles{}, outside{}; unsigned xcd_mask = 0; bool fmt = false, edge = false; };      // fmt: some item is YUYV — the *_fmt launchers
// Every kind but Geoms: the tile grid of the vcam step (ROI-anchored tile columns for every class).
// Surfaces: items[i].d_frame is the Y plane of the NV12 surface surf[i] (geoms_check left such items) — the surface records follow the descriptors in the ring entry,
// a descriptor names its position in pad[0], and the prep launch is launch_prep_geoms_nv12
int geoms_front(bsx_ctx* c, const GeomsRequest& q, hipStream_t s, int k, GeomsStaged* st) {
  const char* fn = geoms_kind(q.kind).fn;
  const bool vg = q.kind != GeomsKind::Geoms;
  const bsx_surface_item* const surf = q.kind == GeomsKind::Surfaces ? q.surfaces : nullptr;
  const bsx_geom_item* const items = surf ? c->geo_checked.front_items.data() : q.items;
  const int* const ids = q.ids;
  const int n = q.n, G = (int)c->geoms.size();
  // positions ordered by class (a counting sort: stable, so a class keeps the caller's order)
  int count[kMaxGeoms] = {0};
  for (int i = 0; i < n; i++) count[c->geom_of(ids[i])]++;
  GeomSpans prep{};
  GeomSpans &tiles = st->tiles, &outside = st->outside;
  unsigned xcd_mask = 0;
  for (int g = 0; g < kMaxGeoms; g++) {
    const int cnt = g < G ? count[g] : 0;
    const int per_t = g < G ? (int)(vg ? c->geoms[g].vg_tiles_per_frame : c->geoms[g].tiles_per_frame) : 0, per_o = g < G ? c->geoms[g].outside_blocks : 0;
    if ((long)tiles.wg[g] + (long)cnt * per_t >= (1l << 31) || (long)outside.wg[g] + (long)cnt * per_o >= (1l << 31))
      return too_many_workgroups(c, fn);
    prep.pos[g + 1] = tiles.pos[g + 1] = outside.pos[g + 1] = tiles.pos[g] + cnt;
    tiles.wg[g + 1] = tiles.wg[g] + cnt * per_t; tiles.per[g] = per_t;
    outside.wg[g + 1] = outside.wg[g] + cnt * per_o; outside.per[g] = per_o;
    if (g < G && c->geoms[g].xcd) xcd_mask |= 1u << g;
    if (cnt && c->geoms[g].edge) st->edge = true;
  }
  st->xcd_mask = xcd_mask;
  c->geo_order.resize((size_t)n); c->geo_ids.resize((size_t)n);
  int next[kMaxGeoms];
  for (int g = 0; g < kMaxGeoms; g++) next[g] = tiles.pos[g];
  for (int i = 0; i < n; i++) c->geo_order[(size_t)next[c->geom_of(ids[i])]++] = i;
  GeomDesc* hd = c->geo_entry(c->h_geo, k);
  VgSurfRec* const hs = reinterpret_cast<VgSurfRec*>(hd + n);          // (48 n bytes behind a 16-byte aligned address)
  for (int j = 0; j < n; j++) {
    const int i = c->geo_order[(size_t)j], id = ids[i];
    const bsx_ctx::Geom& q = c->geoms[c->geom_of(id)];
    const bsx_geom_item& it = items[i];
    c->geo_ids[(size_t)j] = id;
    const bool off = (it.setting.flags & BSX_STREAM_FILTER_OFF) != 0;
    hd[j] = GeomDesc{it.d_frame, it.d_out, off ? nullptr : it.setting.d_bg, c->d_masks + q.mask_offset + (size_t)(id - q.first) * q.width * q.height,
                     it.setting.flags & (kMixFlipH | kMixFlipV | kMixFilterOff | kGeomYuyvIn), id, {0, 0}};
    if (surf) { hd[j].pad[0] = j; hs[j] = VgSurfRec{surf[i].d_uv, surf[i].pitch_y, surf[i].pitch_uv}; }
  }
  st->fmt = geoms_any_yuyv(items, n);
  const int* d_ids = nullptr;
  if (const int rc = ids_copy(c, c->geo_ids.data(), n, s, k, &d_ids)) return rc;
  GeomDesc* const dd = c->geo_entry(c->d_geo, k);
  BSX_HIP(c, hipMemcpyAsync(dd, hd, (size_t)n * (sizeof(GeomDesc) + (surf ? sizeof(VgSurfRec) : 0)), hipMemcpyHostToDevice, s));
  st->desc = dd;
  {
    bsx_roctx::Range range("bsx:prep");
    float* f32 = !c->in_u8 ? c->tensor_ptr(c->plan.input) : nullptr;
    if (surf) BSX_HIP(c, launch_prep_geoms_nv12(c->d_geom_classes, dd, reinterpret_cast<const VgSurfRec*>(dd + n), prep, f32, c->in_u8 ? c->d_net_in_u8 : nullptr, c->inW, c->inH, c->bilateral, n, s));
    else BSX_HIP(c, (st->fmt ? launch_prep_geoms_fmt : launch_prep_geoms)(c->d_geom_classes, dd, prep, f32, c->in_u8 ? c->d_net_in_u8 : nullptr, c->inW, c->inH, c->bilateral, n, s));
  }
  return infer_after_prep(c, n, s, 0, d_ids);
}

// the checked call on the context's device, ring entry k acquired
int geoms_run(bsx_ctx* c, const GeomsRequest& q, hipStream_t s, int k) {
  GeomsStaged st;
  if (const int rc = geoms_front(c, q, s, k, &st)) return rc;
  bsx_roctx::Range range("bsx:mask+blend");
  BSX_HIP(c, (st.edge ? launch_mask_blend_geoms_edge : st.fmt ? launch_mask_blend_geoms_fmt : launch_mask_blend_geoms)(c->d_geom_classes, st.desc, st.tiles, st.xcd_mask, st.outside, c->d_ofinal, c->outW, c->outH, c->d_geom_tile_class, q.n, s, (int)q.flags));
  return BSX_OK;
}

// ---- bsx_step_batch_vcam_geoms: the geoms step with every composite written at ONE common size, the virtual camera's ------------------------------------------
// geoms_run's shape: the same front, then [one tile-class launch,] ONE masks-only tile launch and ONE resize pass over every position's frame, background and mask
// taps.  Outside a ROI the persistent mask is 255 from reset on, so nothing there needs a launch; no capture-size composite is stored.
// the class records of (out_w, out_h), built and uploaded on the first call at that size
int vg_geoms_records(bsx_ctx* c, int out_w, int out_h, const VgClass** out, const VgClass** host = nullptr) {
  const auto key = std::make_pair(out_w, out_h);
  auto it = c->vg_geoms.find(key);
  if (it == c->vg_geoms.end()) {
    const size_t G = c->geoms.size();
    std::vector<VgClass> rec(G);
    bsx_ctx::VgGeoms v;
    int rc = BSX_OK;
    for (size_t g = 0; g < G && rc == BSX_OK; g++) {
      const bsx_ctx::Geom& q = c->geoms[g];
      VcamTab own;
      const VcamTab* t = &own;
      if (g == 0) rc = vcam_tab(c, out_w, out_h, &t);
      else if ((rc = vcam_tab_build(c, q.width, q.height, out_w, out_h, &own)) == BSX_OK) v.mem.push_back(own.d.mem);
      if (rc == BSX_OK) rec[g] = VgClass{q.width, q.height, (t->direct || c->vcam_direct) ? 1 : 0, 0, t->d.tab};
    }
    if (rc == BSX_OK && hipMalloc(reinterpret_cast<void**>(&v.d_rec), G * sizeof(VgClass)) != hipSuccess) rc = BSX_EDEVICE;
    if (rc == BSX_OK && hipMemcpy(v.d_rec, rec.data(), G * sizeof(VgClass), hipMemcpyHostToDevice) != hipSuccess) rc = BSX_EDEVICE;
    if (rc != BSX_OK) {
      for (void* m : v.mem) if (m) (void)hipFree(m);
      if (v.d_rec) (void)hipFree(v.d_rec);
      if (c->last_error.empty()) c->last_error = "error: bsx_step_batch_vcam_geoms: the class records could not be uploaded\n";
      return rc;
    }
    v.h_rec = std::move(rec);
    it = c->vg_geoms.emplace(key, std::move(v)).first;
  }
  *out = it->second.d_rec;
  if (host) *host = it->second.h_rec.data();
  return BSX_OK;
}

int vcam_geoms_run(bsx_ctx* c, const GeomsRequest& q, hipStream_t s, int k) {
  const long out_tiles = (long)((q.out_w + 63) / 64) * ((q.out_h + 31) / 32);      // the resize pass's 64 x 32 output tiles (kernels_img.hip)
  if (out_tiles * q.n >= (1l << 31)) return too_many_workgroups(c, geoms_kind(q.kind).fn);
  const VgClass* vg = nullptr;
  if (const int rc = vg_geoms_records(c, q.out_w, q.out_h, &vg)) return rc;
  GeomsStaged st;
  if (const int rc = geoms_front(c, q, s, k, &st)) return rc;
  bsx_roctx::Range range("bsx:mask+vcam");
  BSX_HIP(c, (st.fmt ? launch_vcam_geoms_fmt : launch_vcam_geoms)(vg_classes(c), vg, st.desc, st.tiles, st.xcd_mask, c->d_ofinal, c->outW, c->outH, c->d_geom_tile_class, q.out_w, q.out_h, q.n, s, q.flags & 1u));
  return BSX_OK;
}

// ---- bsx_step_batch_vcam_geoms_outs: the vcam geoms step with several outputs per position, each of its own size -----------------------------------------------
// vcam_geoms_run's shape: the same front, then [one tile-class launch,] ONE masks-only tile launch and ONE resize pass whose grid ranges over the output records
// (geoms_check left the plan: the records ordered into (class, size) groups).  The three kinds with records — VcamOuts: BGR / YUYV; VcamOutsNv12 and Surfaces: NV12,
// whose plane records follow the descriptors in the ring entry; Surfaces: the items' frames are NV12 surfaces too (geoms_front) — differ in the resize pass the
// launcher picks.
int vcam_outs_run(bsx_ctx* c, const GeomsRequest& q, hipStream_t s, int k) {
  const VcamOutsPlan& plan = c->geo_checked.plan;
  const bool nv12 = geoms_kind(q.kind).records == GeomsRecords::Nv12, surf = geoms_kind(q.kind).surface;
  const int n = q.n;
  const size_t eb = c->vo_entry_bytes(), m = plan.order.size();
  if (!c->h_vo) BSX_HIP(c, hipHostMalloc(reinterpret_cast<void**>(&c->h_vo), bsx_ctx::kIdRing * eb, hipHostMallocDefault));
  if (!c->d_vo) BSX_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->d_vo), bsx_ctx::kIdRing * eb));
  // the class records of every size of the call, from the per-size cache (built and uploaded on the first call at a size)
  const VgClass* rec[kVoMaxSizes] = {};
  for (int q = 0; q < plan.n_sizes; q++) {
    const VgClass* dev = nullptr;
    if (const int rc = vg_geoms_records(c, plan.sizes[q][0], plan.sizes[q][1], &dev, &rec[q])) return rc;
  }
  GeomsStaged st;
  if (const int rc = geoms_front(c, q, s, k, &st)) return rc;
  // groups and output descriptors into ring entry k: a record's descriptor is its position's (geoms_front left them in the pinned entry) with `out` replaced
  VgOutGroup* const hg = reinterpret_cast<VgOutGroup*>(c->h_vo + (size_t)k * eb);
  GeomDesc* const ho = reinterpret_cast<GeomDesc*>(hg + kMaxOutGroups);
  const GeomDesc* const hd = c->geo_entry(c->h_geo, k);
  c->vo_pos.resize((size_t)n);
  for (int j = 0; j < n; j++) c->vo_pos[(size_t)c->geo_order[(size_t)j]] = j;
  OutSpans sp{};
  sp.ng = (int)plan.groups.size();
  const unsigned yuyv = q.flags & 1u;
  for (int g = 0; g < kMaxOutGroups; g++) {
    sp.wg[g] = (int)plan.total_wg;
    if (g >= sp.ng) { hg[g] = VgOutGroup{}; continue; }
    const VcamOutsGroup& G = plan.groups[(size_t)g];
    sp.wg[g] = (int)G.wg0; sp.rec[g] = G.first; sp.per[g] = G.per;
    hg[g] = VgOutGroup{rec[G.size][G.cls], G.ntx, (int)yuyv | (G.words ? 16 : 0), {0, 0}};
  }
  sp.wg[kMaxOutGroups] = (int)plan.total_wg;
  VgNv12Rec* const hn = reinterpret_cast<VgNv12Rec*>(ho + m);          // (48 m bytes behind a 16-byte aligned address)
  for (size_t r = 0; r < m; r++) {
    if (nv12) {
      const bsx_vcam_out_nv12& o = q.outs_nv12[plan.order[r]];
      ho[r] = hd[c->vo_pos[(size_t)o.item]];
      ho[r].out = o.d_y;
      hn[r] = VgNv12Rec{o.d_uv, o.pitch_y, o.pitch_uv};
    } else {
      const bsx_vcam_out& o = q.outs[plan.order[r]];
      ho[r] = hd[c->vo_pos[(size_t)o.item]];
      ho[r].out = o.d_out;
    }
  }
  uint8_t* const dv = c->d_vo + (size_t)k * eb;
  const size_t desc_at = (size_t)kMaxOutGroups * sizeof(VgOutGroup), nrec_at = desc_at + m * sizeof(GeomDesc);
  if (m) BSX_HIP(c, hipMemcpyAsync(dv, hg, nrec_at + (nv12 ? m * sizeof(VgNv12Rec) : 0), hipMemcpyHostToDevice, s));
  bsx_roctx::Range range("bsx:mask+vcam");
  BSX_HIP(c, launch_vcam_geoms_outs(vg_classes(c), reinterpret_cast<const VgOutGroup*>(dv), reinterpret_cast<const GeomDesc*>(dv + desc_at),
                                    nv12 ? reinterpret_cast<const VgNv12Rec*>(dv + nrec_at) : nullptr, surf ? reinterpret_cast<const VgSurfRec*>(st.desc + n) : nullptr, sp,
                                    st.desc, st.tiles, st.xcd_mask, c->d_ofinal, c->outW, c->outH, c->d_geom_tile_class, n, s, st.fmt));
  return BSX_OK;
}

// The one path of the five entry points: the ids, the empty batch, the request's check (geoms_request.hpp: nothing is enqueued before it passes), then on the
// context's device a ring entry and the run of the request's kind.  The entry points only build the request.
int geoms_call(bsx_ctx* c, GeomsRequest q, void* stream) {
  if (!c) return BSX_EINVAL;
  const char* fn = geoms_kind(q.kind).fn;
  if (const int rc = ids_check(c, fn, q.ids, q.n)) return rc;
  if (q.n == 0) return refuse_pending(c, fn);
  GeomsClass classes[kMaxGeoms];
  q.classes = classes; q.n_classes = (int)c->geoms.size();
  for (int g = 0; g < q.n_classes; g++) {
    const bsx_ctx::Geom& G = c->geoms[(size_t)g];
    classes[g] = GeomsClass{G.first, G.width, G.height, G.fusable, G.tab_down.tab.mode, G.roi.x, G.roi.w, G.roi.h, prep_yuyv_fusable(G.width, G.roi, G.tab_down.tab)};
  }
  q.pending = c->pend.active; q.onmask = c->onmask != nullptr;
  const int checked = geoms_check(q, &c->geo_checked);
  if (checked == GeomsChecked::kRefused) return refuse(c, fn, "%s", c->geo_checked.why.text);
  if (checked == GeomsChecked::kTooLarge) return too_many_workgroups(c, fn);
  DeviceGuard guard(c->device);
  hipStream_t s = pick(c, stream);
  if (const int rc = geoms_device_state(c)) return rc;
  int entry = 0;
  if (const int rc = ring_acquire(c, &entry)) return rc;
  return ids_release(c, entry, s, (q.kind == GeomsKind::Geoms ? geoms_run : q.kind == GeomsKind::VcamGeoms ? vcam_geoms_run : vcam_outs_run)(c, q, s, entry));
}

// ---- two-deep pipeline: mask pipeline of batch k  ||  composite of batch k - 1 ------------------------------------------------------------------
// The composite (HBM-bound) of the batch handed over by the previous call goes to comp_stream, the mask pipeline (latency-bound) of this call's batch to the
// caller's stream (the reference's CalcMask worker next to its blend loop, app/deepseg.cc:182-216, 634-681); the only shared object, the model-resolution
// temporal state, is protected by ev_pcomp in front of the launch that advances it.  Every frame is composited with ITS OWN mask (bsx.h).

int pipelined_objects(bsx_ctx* c) {
  if (c->comp_stream) return BSX_OK;
  // the composite fills the gaps of the network kernels, not the other way round: lowest priority the device offers (BSX_PIPE_PRIO=0: default priority)
  int lo = 0, hi = 0;
  const char* pe = BSX_DBG_ENV("BSX_PIPE_PRIO");
  if (!(pe && atoi(pe) == 0) && hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && lo != hi) BSX_HIP(c, hipStreamCreateWithPriority(&c->comp_stream, hipStreamNonBlocking, lo));
  else BSX_HIP(c, hipStreamCreateWithFlags(&c->comp_stream, hipStreamNonBlocking));
  BSX_HIP(c, hipEventCreateWithFlags(&c->ev_pdone, hipEventDisableTiming));
  BSX_HIP(c, hipEventCreateWithFlags(&c->ev_pcomp, hipEventDisableTiming));
  return BSX_OK;
}
int composite_pending(bsx_ctx* c, hipStream_t s, bool concurrent) {
  const bsx_ctx::PendingComposite& p = c->pend;
  // next to the network kernels the composite holds at most pipe_wgs workgroups per CU (an unused LDS pad: static 16.7 KB + pad <= 64 KB, i.e. >= 2 per CU)
  int pad = 0;
  if (concurrent && c->pipe_wgs > 0) pad = std::max(0, std::min(47 * 1024, (160 * 1024 / c->pipe_wgs - 17 * 1024) & ~255));
  bsx_roctx::Range range("bsx:mask+blend");
  BSX_HIP(c, launch_mask_blend(c->d_ofinal, c->outW, c->outH, c->in_roi, c->tab_up.tab, c->d_masks, c->width, c->height, c->roi, p.bg, p.bg_stride, p.frames, p.out, p.n, s,
                               (int)p.flags, pad));
  return BSX_OK;
}

// workgroup barriers one launch of the specialised middle kernel executes per frame: one in front of every micro-op, the ones inside squeeze-excite ops (pool | FC | FC)
// and between the channel chunks of staged depthwise ops — counted in the generated source itself (gen_mid.cpp), so the line cannot drift from the kernel
std::string mid_barrier_line(const Plan& p, bool act16) {
  std::string why;
  const std::string src = generate_mid_source(p, &why, act16);
  if (src.empty()) return "specialised middle kernel: none (" + why + ")\n";
  const size_t k0 = src.find("extern \"C\" __global__");
  auto count = [&](const char* pat) { size_t n = 0; for (size_t q = src.find(pat, k0); q != std::string::npos; q = src.find(pat, q + 1)) n++; return n; };
  const size_t ob = count("op_barrier();"), sy = count("__syncthreads();");
  char line[256];
  snprintf(line, sizeof line, "specialised middle kernel: %zu micro-ops, %zu workgroup barriers per launch (%zu between ops + %zu inside ops)\n", p.program.size(), ob + sy, ob, sy);
  return line;
}
}  // namespace

extern "C" {

const char* bsx_version(void) { return "bsx 0.1 (HIP gfx950, f32 NHWC)"; }

int bsx_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char* bsx_last_error(const bsx_ctx* ctx) { return ctx ? ctx->last_error.c_str() : g_last_error.c_str(); }

// ROI geometry of a width x height capture for the loaded model, float arithmetic truncated to int exactly as lib/libbackscrub.cc:230-246; false: empty or out of range
static bool capture_rois(const bsx_ctx* c, size_t width, size_t height, Rect4* roi, Rect4* in_roi) {
  float ratio = (float)c->inH / (float)c->inW;
  float frameratio = (float)height / (float)width;
  if (frameratio < ratio) {
    *roi = Rect4{(int)((width - height / ratio) / 2), 0, (int)(height / ratio), (int)height};
    *in_roi = Rect4{0, 0, c->inW, c->inH};
  } else {
    *roi = Rect4{0, 0, (int)width, (int)height};
    *in_roi = Rect4{(int)((c->inW - c->inH / frameratio) / 2), 0, (int)(c->inH / frameratio), c->inH};
  }
  return !(roi->w <= 0 || roi->h <= 0 || roi->x < 0 || roi->x + roi->w > (int)width || in_roi->w <= 0 || in_roi->x < 0 || in_roi->x + in_roi->w > c->inW ||
           in_roi->x + in_roi->w > c->outW || in_roi->h > c->outH);
}

// bsx_new / bsx_new_geoms: geoms[0..n_geoms) checked by the caller (positive sizes and counts, total <= 65535); class 0 becomes the context's own geometry
// geom_flags: bsx_new_geoms_ex's (BSX_GEOMS_EDGE_ROI), 0 from the other two
static bsx_ctx* new_ctx(const char* model_path, size_t threads, const bsx_geometry* geoms, int n_geoms, int device, bsx_debug_fn ondebug, bsx_stage_fn onprep,
                        bsx_stage_fn oninfer, bsx_stage_fn onmask, void* caller_ctx, unsigned geom_flags = 0) {
  const size_t width = (size_t)geoms[0].width, height = (size_t)geoms[0].height;
  int n_streams = 0;
  for (int g = 0; g < n_geoms; g++) n_streams += geoms[g].n_streams;
  try {   // nothing may throw across the C ABI (std::bad_alloc / length_error from a hostile model file included)
  std::unique_ptr<bsx_ctx> c(new bsx_ctx);
  c->ondebug = ondebug; c->onprep = onprep; c->oninfer = oninfer; c->onmask = onmask; c->caller_ctx = caller_ctx;
  c->threads = threads; c->width = (int)width; c->height = (int)height; c->n_streams = n_streams; c->device = device;
  c->edge_roi = (geom_flags & BSX_GEOMS_EDGE_ROI) != 0;
  std::string err;
  if (!load_tflite(model_path, &c->graph, &err)) { report(nullptr, ondebug, caller_ctx, "error: %s\n", err.c_str()); return nullptr; }
  c->model_type = model_type_from_name(model_path);
  if (c->model_type == BSX_MODEL_UNKNOWN) { report(nullptr, ondebug, caller_ctx, "error: unknown model type '%s'.\n", model_path); return nullptr; }
  // normalisation (lib/libbackscrub.cc:132-148)
  if (c->model_type == BSX_MODEL_DEEPLAB) { c->norm_scale = (float)(1 / 127.5); c->norm_offset = -1.f; }
  else { c->norm_scale = (float)(1 / 255.0); c->norm_offset = 0.f; }
  const TensorInfo& ti = c->graph.tensors[c->graph.input];
  const TensorInfo& to = c->graph.tensors[c->graph.output];
  if (ti.shape.size() != 4 || to.shape.size() != 4 || ti.dims[0] != 1) {  // cf. getTensorMat, :85-112
    report(nullptr, ondebug, caller_ctx, "error: model input/output is not a single 4-D float tensor\n");
    return nullptr;
  }
  c->inH = ti.dims[1]; c->inW = ti.dims[2]; c->inC = ti.dims[3];
  c->outH = to.dims[1]; c->outW = to.dims[2]; c->outC = to.dims[3];
  if (c->inC != 3) { report(nullptr, ondebug, caller_ctx, "error: model input must have 3 channels\n"); return nullptr; }
  if ((c->model_type == BSX_MODEL_MEET && c->outC != 2) || (c->model_type == BSX_MODEL_DEEPLAB && c->outC < 16)) {
    report(nullptr, ondebug, caller_ctx, "error: model output has %d channels, unexpected for this model type\n", c->outC);
    return nullptr;
  }
  bool no_reuse = BSX_DBG_ENV("BSX_ARENA_NO_REUSE") != nullptr;
  // the per-launch path (BSX_NO_FRAME_PROGRAM) executes the plain step list: it needs the unsegmented plan
  const bool segments = BSX_DBG_ENV("BSX_NO_SEGMENTS") == nullptr && BSX_DBG_ENV("BSX_NO_FRAME_PROGRAM") == nullptr;
  if (!build_plan(c->graph, &c->plan, &err, !no_reuse, segments)) { report(nullptr, ondebug, caller_ctx, "error: unable to build GPU plan: %s\n", err.c_str()); return nullptr; }
  if (!capture_rois(c.get(), width, height, &c->roi, &c->in_roi)) {
    report(nullptr, ondebug, caller_ctx, "error: frame/model geometry yields an empty or out-of-range ROI\n");
    return nullptr;
  }
  c->no_mask_tile = BSX_DBG_ENV("BSX_NO_MASK_TILE") != nullptr;
  // the geometry classes: streams numbered class after class, one slice of the mask allocation each.  With more than one class, every class must be one the
  // geoms step takes — the rule bsx_step_batch_mixed applies per call (the fused tile route), applied here, before any device work
  for (int g = 0; g < n_geoms; g++) {
    bsx_ctx::Geom G;
    G.width = geoms[g].width; G.height = geoms[g].height; G.n_streams = geoms[g].n_streams;
    G.first = g ? c->geoms[g - 1].first + c->geoms[g - 1].n_streams : 0;
    G.mask_offset = c->mask_bytes;
    c->mask_bytes += (size_t)G.n_streams * G.width * G.height;
    if (!capture_rois(c.get(), (size_t)G.width, (size_t)G.height, &G.roi, &G.in_roi)) {
      report(nullptr, ondebug, caller_ctx, "error: bsx_new_geoms: geoms[%d] (%d x %d): frame/model geometry yields an empty or out-of-range ROI\n", g, G.width, G.height);
      return nullptr;
    }
    if (c->edge_roi) {
      // the opt-in rule, for any number of classes: rows of whole dwords and the tiled linear up-scale, with the tiles anchored where each of the two steps puts them
      const HostResizeTab up = make_resize_tab(G.in_roi.w, G.in_roi.h, G.roi.w, G.roi.h);
      G.shifted_tiles_fit = up.mode == 0 && mask_tile_fits(up.xofs.data(), up.yofs.data(), up.sw, up.sh, up.dw, up.dh, geom_edge_shift(G.roi));
      const bool tiles = up.mode == 0 && !c->no_mask_tile && G.roi.w >= 8 && G.shifted_tiles_fit && mask_tile_fits(up.xofs.data(), up.yofs.data(), up.sw, up.sh, up.dw, up.dh);
      if (G.width & 3) {
        report(nullptr, ondebug, caller_ctx, "error: bsx_new_geoms_ex: geoms[%d] (%d x %d): width %d is not a multiple of 4 (the edge-ROI flag frees roi.x and roi.w; a row "
               "must still be whole dwords)\n", g, G.width, G.height, G.width);
        return nullptr;
      }
      if (!tiles) {
        report(nullptr, ondebug, caller_ctx, "error: bsx_new_geoms_ex: geoms[%d] (%d x %d) is off the fused tile route: the mask up-scale %d x %d -> %d x %d must be a tiled "
               "linear one\n", g, G.width, G.height, G.in_roi.w, G.in_roi.h, G.roi.w, G.roi.h);
        return nullptr;
      }
    } else if (n_geoms > 1) {
      const HostResizeTab up = make_resize_tab(G.in_roi.w, G.in_roi.h, G.roi.w, G.roi.h);
      const bool tiles = up.mode == 0 && !c->no_mask_tile && mask_tile_fits(up.xofs.data(), up.yofs.data(), up.sw, up.sh, up.dw, up.dh);
      if ((G.width & 3) || (G.roi.x & 3) || (G.roi.w & 3) || !tiles) {
        report(nullptr, ondebug, caller_ctx, "error: bsx_new_geoms: geoms[%d] (%d x %d) is off the fused tile route: width %d, roi.x %d and roi.w %d must be multiples of 4 and "
               "the mask up-scale %d x %d -> %d x %d a tiled linear one\n", g, G.width, G.height, G.width, G.roi.x, G.roi.w, G.in_roi.w, G.in_roi.h, G.roi.w, G.roi.h);
        return nullptr;
      }
    }
    c->geoms.push_back(G);
  }
  c->no_mask_blend_fusion = BSX_DBG_ENV("BSX_NO_MASK_BLEND_FUSION") != nullptr;
  c->no_bgblur_fusion = BSX_DBG_ENV("BSX_NO_BGBLUR_FUSION") != nullptr;
  c->vcam_direct = BSX_DBG_ENV("BSX_VCAM_DIRECT") != nullptr;
  c->no_uniform_tiles = getenv("BSX_NO_UNIFORM_TILES") != nullptr;
  c->tail_generic = BSX_DBG_ENV("BSX_TAIL_GENERIC") != nullptr;
  c->keep_logits = BSX_DBG_ENV("BSX_KEEP_LOGITS") != nullptr;
  c->arena_poison = BSX_DBG_ENV("BSX_ARENA_POISON") != nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
    report(nullptr, ondebug, caller_ctx, "error: HIP device %d not available (%d visible)\n", device, ndev); return nullptr; }
  DeviceGuard guard(device);    // the caller's current device is restored on return
  if (init_device_state(c.get()) != BSX_OK) { bsx_ctx* raw = c.release(); bsx_delete(raw); return nullptr; }
  c->plan_text = c->plan.describe();
  {
    char line[256];
    for (size_t i = 0; i < c->plan.steps.size(); i++) {      // reduced-precision storage of the per-launch path: one line per fused pair whose output may leave as halves
      if (c->use_program || !c->d_weights16 || !ir_out16_planned(c->plan, c->plan.steps[i], c->f16_terms)) continue;
      const Step& dd = c->plan.steps[c->plan.steps[i].fuse_dw];
      snprintf(line, sizeof line, "f16 storage: steps %zu and %d (expand + depthwise) store t%d (%dx%dx%d per frame) as f16 at %ld pixels and more, step %d reads it as f16\n", i,
               c->plan.steps[i].fuse_dw, dd.out, dd.OH, dd.OW, dd.Cout, kOut16MinRows, c->plan.steps[i].fuse_dw + 1);
      c->plan_text += line;
    }
    snprintf(line, sizeof line, "frame program: %s, %zu micro-ops, LDS %d floats (%.1f KiB), %d tensors in LDS, %d in HBM\n",
             c->use_program ? "ON" : "off", c->plan.program.size(), c->plan.program_lds_floats, c->plan.program_lds_floats / 256.0,
             c->plan.program_lds_tensors, c->plan.program_global_tensors);
    c->plan_text += line;
    if (no_reuse) c->plan_text += "arena: every tensor in a slot of its own (debug switch)\n";
    if (c->arena_poison) c->plan_text += "arena: filled with NaN bytes in front of every network stage (debug switch)\n";
    if (c->use_program) c->plan_text += "program execution: " + c->kern.mid_note + "\n";
    if (c->use_program && c->plan.seg.on) {
      std::string seg = c->plan.seg_text;
      if (c->act16)                     // the storage width of what the segment kernels leave in the arena: "stores t33:f16 t41:f16"
        for (size_t at = seg.find(" stores t"); at != std::string::npos; at = seg.find(" stores t", at)) {
          for (at += 7; at + 2 < seg.size() && seg[at] == ' ' && seg[at + 1] == 't' && isdigit((unsigned char)seg[at + 2]); ) {
            for (at += 2; at < seg.size() && isdigit((unsigned char)seg[at]); at++) {}
            seg.insert(at, ":f16");
            at += 4;
          }
        }
      c->plan_text += seg;
    }
    if (c->use_program && c->plan.seg.on) c->plan_text += "segment execution: " + c->kern.seg_note + "\n";
    if (c->use_program && c->plan.seg.on && c->plan.seg.k3f.on && !c->kern.k3_frame)
      c->plan_text += "segment k3 execution: tiles and the gate launch (the per-frame form is part of the specialised module only)\n";
    if (c->use_program && c->kern.mid) c->plan_text += mid_barrier_line(c->plan, c->act16);
    for (size_t i = 0; i < c->plan.program_labels.size(); i++) {
      c->plan_text += "P" + std::to_string(i) + " " + c->plan.program_labels[i];
      if (i < c->plan.program_out_tensor.size()) {            // the tensor the op leaves behind, and where: the read-back entry serves the "hbm" ones only
        const int sp = c->plan.program[i].out.space;
        c->plan_text += " -> t" + std::to_string(c->plan.program_out_tensor[i]) + (sp == kLocLds ? " lds" : (program_op_elided(c.get(), (int)i) ? " elided" : (sp == kLocOutput ? " output" : " hbm")));
        if (sp == kLocGlobal && !program_op_elided(c.get(), (int)i) && debug_tensor_half(c.get(), c->plan.program_out_tensor[i])) c->plan_text += " f16";
      }
      c->plan_text += "\n";
    }
  }
  return c.release();
  } catch (const std::exception& e) {
    report(nullptr, ondebug, caller_ctx, "error: %s while creating the context\n", e.what());
    return nullptr;
  } catch (...) {
    report(nullptr, ondebug, caller_ctx, "error: unknown exception while creating the context\n");
    return nullptr;
  }
}

bsx_ctx* bsx_new(const char* model_path, size_t threads, size_t width, size_t height, int n_streams, int device, bsx_debug_fn ondebug,
                 bsx_stage_fn onprep, bsx_stage_fn oninfer, bsx_stage_fn onmask, void* caller_ctx) {
  if (!model_path || !width || !height || width > 0x7fffffffu || height > 0x7fffffffu || n_streams <= 0 || n_streams > 65535) {   // grid.z of the mask kernel carries the stream index
    report(nullptr, ondebug, caller_ctx, "error: bad arguments to bsx_new\n"); return nullptr; }
  const bsx_geometry one{(int)width, (int)height, n_streams};
  return new_ctx(model_path, threads, &one, 1, device, ondebug, onprep, oninfer, onmask, caller_ctx);
}

// the argument checks of bsx_new_geoms and bsx_new_geoms_ex (fn: the message prefix), then the context
static bsx_ctx* new_geoms_checked(const char* fn, const char* model_path, size_t threads, const bsx_geometry* geoms, int n_geoms, int device, unsigned geom_flags,
                                  bsx_debug_fn ondebug, bsx_stage_fn onprep, bsx_stage_fn oninfer, bsx_stage_fn onmask, void* caller_ctx) {
  if (!model_path || !geoms) { report(nullptr, ondebug, caller_ctx, "%s model_path or geoms is NULL\n", fn); return nullptr; }
  if (n_geoms < 1 || n_geoms > BSX_MAX_GEOMS) { report(nullptr, ondebug, caller_ctx, "%s n_geoms = %d is outside [1, %d]\n", fn, n_geoms, BSX_MAX_GEOMS); return nullptr; }
  long total = 0;
  for (int g = 0; g < n_geoms; g++) {
    if (geoms[g].width <= 0 || geoms[g].height <= 0) { report(nullptr, ondebug, caller_ctx, "%s geoms[%d]: size %d x %d is not positive\n", fn, g, geoms[g].width, geoms[g].height); return nullptr; }
    if (geoms[g].n_streams <= 0) { report(nullptr, ondebug, caller_ctx, "%s geoms[%d] (%d x %d): n_streams = %d is not positive\n", fn, g, geoms[g].width, geoms[g].height, geoms[g].n_streams); return nullptr; }
    for (int k = 0; k < g; k++)
      if (geoms[k].width == geoms[g].width && geoms[k].height == geoms[g].height) {
        report(nullptr, ondebug, caller_ctx, "%s geoms[%d] (%d x %d) repeats the size of geoms[%d]\n", fn, g, geoms[g].width, geoms[g].height, k); return nullptr; }
    total += geoms[g].n_streams;
    if (total > 65535) { report(nullptr, ondebug, caller_ctx, "%s geoms[%d] (%d x %d) brings the total to %ld streams, above 65535\n", fn, g, geoms[g].width, geoms[g].height, total); return nullptr; }
  }
  if (n_geoms > 1 && onmask) { report(nullptr, ondebug, caller_ctx, "%s an onmask callback needs a context of one geometry (%d given)\n", fn, n_geoms); return nullptr; }
  return new_ctx(model_path, threads, geoms, n_geoms, device, ondebug, onprep, oninfer, onmask, caller_ctx, geom_flags);
}

bsx_ctx* bsx_new_geoms(const char* model_path, size_t threads, const bsx_geometry* geoms, int n_geoms, int device, bsx_debug_fn ondebug, bsx_stage_fn onprep,
                       bsx_stage_fn oninfer, bsx_stage_fn onmask, void* caller_ctx) {
  return new_geoms_checked("error: bsx_new_geoms:", model_path, threads, geoms, n_geoms, device, 0, ondebug, onprep, oninfer, onmask, caller_ctx);
}

bsx_ctx* bsx_new_geoms_ex(const char* model_path, size_t threads, const bsx_geometry* geoms, int n_geoms, int device, unsigned flags, bsx_debug_fn ondebug,
                          bsx_stage_fn onprep, bsx_stage_fn oninfer, bsx_stage_fn onmask, void* caller_ctx) {
  if (flags == 0) return bsx_new_geoms(model_path, threads, geoms, n_geoms, device, ondebug, onprep, oninfer, onmask, caller_ctx);
  if (const unsigned unknown = flags & ~BSX_GEOMS_EDGE_ROI) {
    report(nullptr, ondebug, caller_ctx, "error: bsx_new_geoms_ex: flags 0x%x has the unknown bit 0x%x (known: 0x%x, the edge-ROI flag)\n", flags, unknown & (0u - unknown),
           BSX_GEOMS_EDGE_ROI);
    return nullptr;
  }
  return new_geoms_checked("error: bsx_new_geoms_ex:", model_path, threads, geoms, n_geoms, device, flags, ondebug, onprep, oninfer, onmask, caller_ctx);
}

void bsx_delete(bsx_ctx* c) {
  if (!c) return;
  DeviceGuard guard(c->device);
  if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
  for (auto& kv : c->host_graphs) if (kv.second) (void)hipGraphExecDestroy(kv.second);
  unload_specialised(&c->kern);
  void* ptrs[] = {c->d_arena, c->d_net_in, c->d_net_in_u8, c->d_net_out, c->d_weights, c->d_ofinal, c->d_masks, c->d_host_frame, c->d_bgr_scratch, c->d_bgr_scratch2, c->d_mask_scratch, c->d_bgblur_scratch, c->d_bgr_in_scratch, c->d_color_lut, c->tab_down.mem, c->tab_up.mem, c->d_program, c->d_weights16, c->d_tile_class};
  for (void* p : ptrs) if (p) (void)hipFree(p);
  for (auto& kv : c->bg_tabs) if (kv.second.mem) (void)hipFree(kv.second.mem);
  for (auto& kv : c->vcam_tabs) if (kv.second.d.mem) (void)hipFree(kv.second.d.mem);
  for (auto& kv : c->vg_geoms) { for (void* m : kv.second.mem) if (m) (void)hipFree(m); if (kv.second.d_rec) (void)hipFree(kv.second.d_rec); }
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  for (int k = 1; k < 4; k++) { if (c->lane_stream[k]) (void)hipStreamDestroy(c->lane_stream[k]); if (c->ev_join[k]) (void)hipEventDestroy(c->ev_join[k]); }
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  if (c->comp_stream) { (void)hipStreamSynchronize(c->comp_stream); (void)hipStreamDestroy(c->comp_stream); }
  if (c->ev_pdone) (void)hipEventDestroy(c->ev_pdone);
  if (c->ev_pcomp) (void)hipEventDestroy(c->ev_pcomp);
  for (hipEvent_t& e : c->ev_ids) if (e) (void)hipEventDestroy(e);
  if (c->d_ids) (void)hipFree(c->d_ids);
  if (c->h_ids) (void)hipHostFree(c->h_ids);
  if (c->d_mix) (void)hipFree(c->d_mix);
  if (c->h_mix) (void)hipHostFree(c->h_mix);
  for (bsx_ctx::DescRing* r : {&c->rsz_ring, &c->blur_ring, &c->blur_surf_ring, &c->rsz_surf_ring}) {
    if (r->d) (void)hipFree(r->d);
    if (r->h) (void)hipHostFree(r->h);
  }
  if (c->d_blur_coef) (void)hipFree(c->d_blur_coef);
  for (size_t g = 1; g < c->geoms.size(); g++) { if (c->geoms[g].tab_down.mem) (void)hipFree(c->geoms[g].tab_down.mem); if (c->geoms[g].tab_up.mem) (void)hipFree(c->geoms[g].tab_up.mem); }
  if (c->d_geom_classes) (void)hipFree(c->d_geom_classes);
  if (c->d_geom_classes_vg) (void)hipFree(c->d_geom_classes_vg);
  if (c->d_geom_tile_class) (void)hipFree(c->d_geom_tile_class);
  if (c->d_geo) (void)hipFree(c->d_geo);
  if (c->d_vo) (void)hipFree(c->d_vo);
  if (c->h_vo) (void)hipHostFree(c->h_vo);
  if (c->h_geo) (void)hipHostFree(c->h_geo);
  delete c;
}

int bsx_get_info(const bsx_ctx* c, bsx_info* o) {
  if (!c || !o) return BSX_EINVAL;
  memset(o, 0, sizeof *o);
  o->model_type = c->model_type; o->width = c->width; o->height = c->height; o->n_streams = c->n_streams;
  o->in_w = c->inW; o->in_h = c->inH; o->in_c = c->inC; o->out_w = c->outW; o->out_h = c->outH; o->out_c = c->outC;
  int r[4] = {c->roi.x, c->roi.y, c->roi.w, c->roi.h}, q[4] = {c->in_roi.x, c->in_roi.y, c->in_roi.w, c->in_roi.h};
  memcpy(o->roi, r, sizeof r); memcpy(o->in_roi, q, sizeof q);
  o->n_ops = c->graph.n_file_ops; o->n_steps = c->use_program ? (c->plan.seg.on ? 5 : 1) : (int)c->plan.steps.size(); o->device = c->device;
  o->norm_scale = c->norm_scale; o->norm_offset = c->norm_offset;
  o->nn_flops_per_frame = 2.0 * c->plan.macs_per_frame;
  o->act_bytes_per_stream = c->plan.arena_floats_per_stream * sizeof(float);
  return BSX_OK;
}

int bsx_reset(bsx_ctx* c, void* stream) {
  if (!c) return BSX_EINVAL;
  DeviceGuard guard(c->device);
  hipStream_t s = pick(c, stream);
  const size_t N = (size_t)c->n_streams;
  c->pend.active = false;                                          // a composite still pending in the two-deep pipeline is dropped with the state it belongs to
  BSX_HIP(c, hipMemsetAsync(c->d_ofinal, 0, N * c->outW * c->outH, s));
  BSX_HIP(c, hipMemsetAsync(c->d_masks, 255, c->mask_bytes, s));
  return BSX_OK;
}

uint8_t* bsx_masks_device(bsx_ctx* c) { return c ? c->d_masks : nullptr; }

int bsx_process_batch(bsx_ctx* c, const uint8_t* d_frames, int n, uint8_t* d_masks, void* stream) {
  if (!c || !d_frames || n <= 0 || n > c->n_streams) return BSX_EINVAL;
  if (const int rc = refuse_geoms(c, "bsx_process_batch")) return rc;
  if (const int rc = refuse_pending(c, "bsx_process_batch")) return rc;
  DeviceGuard guard(c->device);
  hipStream_t s = pick(c, stream);
  if (const int rc = process_impl(c, d_frames, n, 0, s)) return rc;
  if (d_masks) BSX_HIP(c, hipMemcpyAsync(d_masks, c->d_masks, (size_t)n * c->width * c->height, hipMemcpyDeviceToDevice, s));
  return BSX_OK;
}

int bsx_process_host(bsx_ctx* c, int stream_idx, const uint8_t* h_bgr, size_t bgr_stride, uint8_t* h_mask, size_t mask_stride) {
  if (!c || !h_bgr || !h_mask || stream_idx < 0 || stream_idx >= c->n_streams) return BSX_EINVAL;
  if (const int rc = refuse_geoms(c, "bsx_process_host")) return rc;
  if (bgr_stride < (size_t)c->width * 3 || mask_stride < (size_t)c->width) return BSX_ESIZE;
  if (const int rc = refuse_pending(c, "bsx_process_host")) return rc;
  DeviceGuard guard(c->device);
  hipStream_t s = c->own_stream;
  const size_t fbytes = (size_t)c->width * c->height * 3;
  if (!c->d_host_frame) BSX_HIP(c, hipMalloc(&c->d_host_frame, fbytes));
  BSX_HIP(c, hipMemcpy2DAsync(c->d_host_frame, (size_t)c->width * 3, h_bgr, bgr_stride, (size_t)c->width * 3, c->height, hipMemcpyHostToDevice, s));
  // the single frame runs against the temporal state of slot `stream_idx` (the context itself is never modified)
  int rc = BSX_OK;
  hipGraphExec_t exec = nullptr;
  if (c->graph_state >= 0 && !c->onprep && !c->oninfer && !c->onmask) {
    auto it = c->host_graphs.find(stream_idx);
    if (it != c->host_graphs.end()) exec = it->second;
    else if (c->host_graphs.size() < 64) {                          // capture this slot's launch chain (the kernels' arguments carry the slot's state pointers)
      hipGraph_t g = nullptr;
      bool ok = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) == hipSuccess;
      if (ok) {
        rc = process_impl(c, c->d_host_frame, 1, stream_idx, s);
        ok = hipStreamEndCapture(s, &g) == hipSuccess && rc == BSX_OK && g != nullptr;
      }
      if (ok) ok = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0) == hipSuccess;
      if (g) (void)hipGraphDestroy(g);
      if (ok) { c->host_graphs[stream_idx] = exec; c->graph_state = 1; }
      else { exec = nullptr; c->graph_state = -1; rc = BSX_OK; (void)hipGetLastError(); }      // nothing ran during the capture: fall through to the direct launches
    }
  }
  if (exec) BSX_HIP(c, hipGraphLaunch(exec, s));
  else rc = process_impl(c, c->d_host_frame, 1, stream_idx, s);
  if (rc) return rc;
  const uint8_t* my_mask = c->d_masks + (size_t)stream_idx * c->width * c->height;
  BSX_HIP(c, hipMemcpy2DAsync(h_mask, mask_stride, my_mask, (size_t)c->width, (size_t)c->width, c->height, hipMemcpyDeviceToHost, s));
  BSX_HIP(c, hipStreamSynchronize(s));
  return BSX_OK;
}

int bsx_composite_batch(bsx_ctx* c, const uint8_t* d_bg, size_t bg_frame_stride, const uint8_t* d_frames, const uint8_t* d_masks, uint8_t* d_out,
                        int n, void* stream) {
  if (!c || !d_bg || !d_frames || !d_out || n <= 0) return BSX_EINVAL;
  if (const int rc = refuse_geoms(c, "bsx_composite_batch")) return rc;
  if (!d_masks) { if (n > c->n_streams) return BSX_EINVAL; d_masks = c->d_masks; }
  DeviceGuard guard(c->device);
  bsx_roctx::Range range("bsx:blend");
  BSX_HIP(c, launch_blend(d_bg, bg_frame_stride, d_frames, d_masks, d_out, (size_t)c->width * c->height, n, pick(c, stream)));
  return BSX_OK;
}

int bsx_step_batch(bsx_ctx* c, const uint8_t* d_frames, const uint8_t* d_bg, size_t bg_frame_stride, uint8_t* d_out, int n, void* stream) {
  return step_call(c, "bsx_step_batch", Entry::Step, StepReq{d_frames, d_bg, bg_frame_stride, d_out, 0, 0, n, 0u, (hipStream_t)stream, nullptr});
}
int bsx_step_batch_yuyv(bsx_ctx* c, const uint8_t* d_frames, const uint8_t* d_bg, size_t bg_frame_stride, uint8_t* d_out_yuyv, int n, void* stream) {
  return step_call(c, "bsx_step_batch_yuyv", Entry::Step, StepReq{d_frames, d_bg, bg_frame_stride, d_out_yuyv, 0, 0, n, BSX_STEP_YUYV, (hipStream_t)stream, nullptr});
}
int bsx_step_batch_ex(bsx_ctx* c, const uint8_t* d_frames, const uint8_t* d_bg, size_t bg_frame_stride, uint8_t* d_out, int n, void* stream, unsigned flags) {
  return step_call(c, "bsx_step_batch_ex", Entry::Step, StepReq{d_frames, d_bg, bg_frame_stride, d_out, 0, 0, n, flags, (hipStream_t)stream, nullptr});
}
// ids (host): frame i's temporal state and persistent mask are slot ids[i]; everything else stays indexed by position i
int bsx_step_batch_streams(bsx_ctx* c, const int* ids, const uint8_t* d_frames, const uint8_t* d_bg, size_t bg_frame_stride, uint8_t* d_out, int n, void* stream,
                           unsigned flags) {
  return step_call(c, "bsx_step_batch_streams", Entry::Streams, StepReq{d_frames, d_bg, bg_frame_stride, d_out, 0, 0, n, flags, (hipStream_t)stream, nullptr}, ids);
}

// settings (host): position i's background, flip, blur and filter switch; flags: the batch's layout bits; ids: NULL = frame i is stream i, else as above
int bsx_step_batch_mixed(bsx_ctx* c, const int* ids, const uint8_t* d_frames, const bsx_stream_setting* settings, uint8_t* d_out, int n, void* stream,
                         unsigned flags) {
  return step_call(c, "bsx_step_batch_mixed", Entry::Mixed, StepReq{d_frames, nullptr, 0, d_out, 0, 0, n, flags, (hipStream_t)stream, nullptr}, ids, settings);
}

int bsx_geom_count(const bsx_ctx* c) { return c ? (int)c->geoms.size() : BSX_EINVAL; }

int bsx_get_geom_info(const bsx_ctx* c, int g, bsx_geom_info* o) {
  if (!c || !o || g < 0 || g >= (int)c->geoms.size()) return BSX_EINVAL;
  const bsx_ctx::Geom& G = c->geoms[(size_t)g];
  memset(o, 0, sizeof *o);
  o->width = G.width; o->height = G.height; o->n_streams = G.n_streams; o->first_stream = G.first;
  int r[4] = {G.roi.x, G.roi.y, G.roi.w, G.roi.h}, q[4] = {G.in_roi.x, G.in_roi.y, G.in_roi.w, G.in_roi.h};
  memcpy(o->roi, r, sizeof r); memcpy(o->in_roi, q, sizeof q);
  o->mask_offset = G.mask_offset;
  return BSX_OK;
}

// The five multi-geometry steps (bsx.h): each builds its request for geoms_call.  ids (host): position i is stream ids[i], whose class decides the geometry of items[i]
int bsx_step_batch_geoms(bsx_ctx* c, const int* ids, const bsx_geom_item* items, int n, void* stream, unsigned flags) {
  GeomsRequest q{};
  q.kind = GeomsKind::Geoms; q.ids = ids; q.n = n; q.items = items; q.flags = flags;
  return geoms_call(c, q, stream);
}
// ... with every d_out at (out_w, out_h)
int bsx_step_batch_vcam_geoms(bsx_ctx* c, const int* ids, const bsx_geom_item* items, int n, int out_w, int out_h, void* stream, unsigned flags) {
  GeomsRequest q{};
  q.kind = GeomsKind::VcamGeoms; q.ids = ids; q.n = n; q.items = items; q.out_w = out_w; q.out_h = out_h; q.flags = flags;
  return geoms_call(c, q, stream);
}
// ... with several outputs per position, each of its own size
int bsx_step_batch_vcam_geoms_outs(bsx_ctx* c, const int* ids, const bsx_geom_item* items, int n, const bsx_vcam_out* outs, int m, void* stream, unsigned flags) {
  GeomsRequest q{};
  q.kind = GeomsKind::VcamOuts; q.ids = ids; q.n = n; q.items = items; q.outs = outs; q.m = m; q.flags = flags;
  return geoms_call(c, q, stream);
}
// ... with every record an NV12 surface
int bsx_step_batch_vcam_geoms_outs_nv12(bsx_ctx* c, const int* ids, const bsx_geom_item* items, int n, const bsx_vcam_out_nv12* outs, int m, void* stream, unsigned flags) {
  GeomsRequest q{};
  q.kind = GeomsKind::VcamOutsNv12; q.ids = ids; q.n = n; q.items = items; q.outs_nv12 = outs; q.m = m; q.flags = flags;
  return geoms_call(c, q, stream);
}
// ... with every frame an NV12 surface too
int bsx_step_batch_surfaces(bsx_ctx* c, const int* ids, const bsx_surface_item* items, int n, const bsx_vcam_out_nv12* outs, int m, void* stream, unsigned flags) {
  GeomsRequest q{};
  q.kind = GeomsKind::Surfaces; q.ids = ids; q.n = n; q.surfaces = items; q.outs_nv12 = outs; q.m = m; q.flags = flags;
  return geoms_call(c, q, stream);
}

int bsx_reset_streams(bsx_ctx* c, const int* ids, int n, void* stream) {
  if (!c) return BSX_EINVAL;
  if (const int rc = ids_check(c, "bsx_reset_streams", ids, n)) return rc;
  if (const int rc = refuse_pending(c, "bsx_reset_streams")) return rc;
  if (n == 0) return BSX_OK;
  DeviceGuard guard(c->device);
  hipStream_t s = pick(c, stream);
  const int* d_ids = nullptr;
  int entry = 0;
  if (c->geoms.size() <= 1) {
    if (const int rc = ids_stage(c, ids, n, s, &d_ids, &entry)) return rc;
    const hipError_t e = launch_reset_slots(c->d_ofinal, (size_t)c->outW * c->outH, c->d_masks, (size_t)c->width * c->height, d_ids, n, s);
    int rc = BSX_OK;
    if (e != hipSuccess) { report(c, c->ondebug, c->caller_ctx, "error: HIP %s while resetting streams\n", hipGetErrorString(e)); rc = BSX_EDEVICE; }
    return ids_release(c, entry, s, rc);
  }
  // several classes: the ids ordered by class, one launch per class present — a slot's mask has its class's size and lies in its class's slice (masks of slot s of
  // class g: d_masks + mask_offset + (s - first) * bytes, i.e. slot-indexed from the slice's base moved back by `first` slots)
  c->geo_ids.assign(ids, ids + n);
  std::stable_sort(c->geo_ids.begin(), c->geo_ids.end(), [&](int a, int b) { return c->geom_of(a) < c->geom_of(b); });
  if (const int rc = ids_stage(c, c->geo_ids.data(), n, s, &d_ids, &entry)) return rc;
  int rc = BSX_OK;
  for (int j = 0; j < n && rc == BSX_OK;) {
    const bsx_ctx::Geom& G = c->geoms[(size_t)c->geom_of(c->geo_ids[(size_t)j])];
    int e2 = j;
    while (e2 < n && c->geo_ids[(size_t)e2] < G.first + G.n_streams) e2++;
    const size_t mb = (size_t)G.width * G.height;
    uint8_t* const base = reinterpret_cast<uint8_t*>(reinterpret_cast<uintptr_t>(c->d_masks) + G.mask_offset - (size_t)G.first * mb);
    const hipError_t e = launch_reset_slots(c->d_ofinal, (size_t)c->outW * c->outH, base, mb, d_ids + j, e2 - j, s);
    if (e != hipSuccess) { report(c, c->ondebug, c->caller_ctx, "error: HIP %s while resetting streams\n", hipGetErrorString(e)); rc = BSX_EDEVICE; }
    j = e2;
  }
  return ids_release(c, entry, s, rc);
}

// ---- the main loop at the virtual camera's geometry (--vg, app/deepseg.cc:634-681): blend → flip → resize → YUYV pack with the resize folded in -----------------
int bsx_step_batch_vcam_mixed(bsx_ctx* c, const int* ids, const uint8_t* d_frames, const bsx_stream_setting* settings, uint8_t* d_out, int out_w, int out_h, int n,
                              void* stream, unsigned flags) {
  return step_call(c, "bsx_step_batch_vcam_mixed", Entry::VcamMixed, StepReq{d_frames, nullptr, 0, d_out, out_w, out_h, n, flags, (hipStream_t)stream, nullptr}, ids,
                   settings);
}

int bsx_step_batch_vcam(bsx_ctx* c, const uint8_t* d_frames, const uint8_t* d_bg, size_t bg_frame_stride, uint8_t* d_out, int out_w, int out_h, int n, void* stream,
                        unsigned flags) {
  return step_call(c, "bsx_step_batch_vcam", Entry::Vcam, StepReq{d_frames, d_bg, bg_frame_stride, d_out, out_w, out_h, n, flags, (hipStream_t)stream, nullptr});
}

int bsx_step_batch_pipelined(bsx_ctx* c, const uint8_t* d_frames, const uint8_t* d_bg, size_t bg_frame_stride, uint8_t* d_out, int n, void* stream, unsigned flags) {
  if (!c) return BSX_EINVAL;
  if (const int rc = refuse_geoms(c, "bsx_step_batch_pipelined")) return rc;
  hipStream_t s = pick(c, stream);
  if (!d_frames) {                                                  // flush: the composite of the last batch, on the caller's stream
    DeviceGuard guard(c->device);
    if (!c->pend.active) return BSX_OK;
    BSX_HIP(c, hipStreamWaitEvent(s, c->ev_pdone, 0));               // the pending batch's network may have run on another stream than this call's
    const int rc = composite_pending(c, s, false);
    c->pend.active = false;
    return rc;
  }
  StepReq r = StepReq{d_frames, d_bg, bg_frame_stride, d_out, c->width, c->height, n, flags, s, nullptr};
  if (const int rc = check_step(c, "bsx_step_batch_pipelined", r, Entry::Pipelined)) return rc;
  DeviceGuard guard(c->device);
  int rc = pipelined_objects(c);
  if (rc) return rc;
  bool forked = false;
  if (c->pend.active) {
    BSX_HIP(c, hipStreamWaitEvent(c->comp_stream, c->ev_pdone, 0)); // behind the network of the pending batch, whatever stream the call that enqueued it was given
    BSX_HIP(c, hipStreamWaitEvent(s, c->ev_pdone, 0));              // this call's network reuses the arena of the previous one: same order if the caller changed streams
    rc = composite_pending(c, c->comp_stream, true);
    // forked work is ALWAYS joined, also after an error: the caller's stream must not be left with work in flight on a stream it cannot see
    if (hipEventRecord(c->ev_pcomp, c->comp_stream) != hipSuccess) rc = rc ? rc : BSX_EDEVICE;
    c->pend.active = false;
    forked = true;
    if (!rc) c->wait_before_state = c->ev_pcomp;
  }
  if (!rc) rc = enqueue_masks(c, d_frames, n, s, r.yin(), 0, nullptr);
  if (forked && (c->wait_before_state || rc)) {                     // fence not consumed (error on the way): join here
    c->wait_before_state = nullptr;
    if (hipStreamWaitEvent(s, c->ev_pcomp, 0) != hipSuccess) rc = rc ? rc : BSX_EDEVICE;
  }
  if (rc) return rc;
  BSX_HIP(c, hipEventRecord(c->ev_pdone, s));
  c->pend.active = true; c->pend.frames = d_frames; c->pend.bg = d_bg; c->pend.bg_stride = bg_frame_stride; c->pend.out = d_out; c->pend.n = n; c->pend.flags = flags;
  return BSX_OK;
}

int bsx_resize_bgr(bsx_ctx* c, const uint8_t* d_src, int sw, int sh, uint8_t* d_dst, int dw, int dh, int n, void* stream) {
  if (!c || !d_src || !d_dst || sw <= 0 || sh <= 0 || dw <= 0 || dh <= 0 || n <= 0) return BSX_EINVAL;
  DeviceGuard guard(c->device);
  const DevResizeTab* t = nullptr;
  if (const int rc = bg_tab(c, sw, sh, dw, dh, &t)) return rc;
  BSX_HIP(c, launch_resize_bgr(d_src, d_dst, t->tab, n, pick(c, stream)));
  return BSX_OK;
}

// n images, each of its own size, to dw x dh in ONE launch: checked on the host, the descriptors through the staging ring, the tables from bg_tabs
int bsx_resize_bgr_batch(bsx_ctx* c, const bsx_resize_item* items, int n, int dw, int dh, void* stream) {
  if (!c) return BSX_EINVAL;
  const int planned = resize_bgr_batch_plan(items, n, c->n_streams, dw, dh, &c->pic_plan);
  const DevResizeTab* t = nullptr;
  return picture_batch_call<ResizeBatchDesc>(c, "bsx_resize_bgr_batch", planned, &c->rsz_ring, false, "resizing a batch", stream,
    [&](int i, ResizeBatchDesc* d) {
      const bsx_resize_item& it = items[i];
      if (const int rc = bg_tab(c, it.sw, it.sh, dw, dh, &t)) return rc;
      *d = ResizeBatchDesc{it.d_src, it.d_dst, t->tab.xofs, t->tab.xa, t->tab.yofs, t->tab.ya, t->tab.sw, t->tab.sh, t->tab.mode, 0};
      return (int)BSX_OK;
    },
    [&](const ResizeBatchDesc* d, const PictureGrid&, hipStream_t s) { return launch_resize_bgr_batch(d, n, dw, dh, s); });
}

int bsx_flip_bgr(bsx_ctx* c, const uint8_t* d_src, uint8_t* d_dst, int w, int h, int n, int code, void* stream) {
  if (!c || !d_src || !d_dst || d_src == d_dst || w <= 0 || h <= 0 || n <= 0) return BSX_EINVAL;
  DeviceGuard guard(c->device);
  BSX_HIP(c, launch_flip_bgr(d_src, d_dst, w, h, code, n, pick(c, stream)));
  return BSX_OK;
}

int bsx_gaussian_blur_bgr(bsx_ctx* c, const uint8_t* d_src, uint8_t* d_dst, int w, int h, int n, int ksize, void* stream) {
  if (!c || !d_src || !d_dst || d_src == d_dst || w <= 0 || h <= 0 || n <= 0 || ksize < 1 || ksize > 31 || !(ksize & 1)) return BSX_EINVAL;
  DeviceGuard guard(c->device);
  BSX_HIP(c, launch_gauss_blur(d_src, d_dst, w, h, ksize, n, pick(c, stream)));
  return BSX_OK;
}

// n images, each of its own size, blur size and pixel format, blurred in ONE launch: checked on the host, the descriptors ordered by size through the staging ring,
// the ragged grid's spans by value
int bsx_gaussian_blur_bgr_batch(bsx_ctx* c, const bsx_blur_item* items, int n, void* stream) {
  if (!c) return BSX_EINVAL;
  const int planned = blur_bgr_batch_plan(items, n, c->n_streams, &c->pic_plan);
  return picture_batch_call<BlurDesc>(c, "bsx_gaussian_blur_bgr_batch", planned, &c->blur_ring, true, "blurring a batch", stream,
    [&](int i, BlurDesc* d) {
      const bsx_blur_item& it = items[i];
      *d = BlurDesc{it.d_src, it.d_dst, it.w, it.h, it.ksize, it.flags & kGeomYuyvIn};
      return (int)BSX_OK;
    },
    [&](const BlurDesc* d, const PictureGrid& g, hipStream_t s) { return launch_blur_batch(d, c->d_blur_coef, g.spans, g.cols, s); });
}

// n NV12 surfaces, each of its own size, pitches and blur size, blurred into BGR images in ONE launch: planned and checked on the host, the descriptors ordered by size
// through the staging ring, the ragged grid's spans by value
int bsx_gaussian_blur_surfaces_batch(bsx_ctx* c, const bsx_blur_surface_item* items, int n, void* stream) {
  if (!c) return BSX_EINVAL;
  const int planned = blur_surfaces_plan(items, n, c->n_streams, &c->pic_plan);
  return picture_batch_call<BlurSurfDesc>(c, "bsx_gaussian_blur_surfaces_batch", planned, &c->blur_surf_ring, true, "blurring a batch of surfaces", stream,
    [&](int i, BlurSurfDesc* d) {
      const bsx_blur_surface_item& it = items[i];
      *d = BlurSurfDesc{it.d_y, it.d_uv, it.d_dst, it.pitch_y, it.pitch_uv, it.w, it.h, it.ksize, 0u};
      return (int)BSX_OK;
    },
    [&](const BlurSurfDesc* d, const PictureGrid& g, hipStream_t s) { return launch_blur_surfaces(d, c->d_blur_coef, g.spans, g.cols, s); });
}

// n NV12 surfaces, each of its own size and pitches, resized to BGR images of their own sizes in ONE launch: planned and checked on the host, the descriptors ordered by
// destination size through the staging ring, the ragged grid's spans and the classes' sizes by value
int bsx_resize_surfaces_batch(bsx_ctx* c, const bsx_resize_surface_item* items, int n, void* stream) {
  if (!c) return BSX_EINVAL;
  const int planned = resize_surfaces_plan(items, n, c->n_streams, &c->pic_plan);
  const DevResizeTab* t = nullptr;
  return picture_batch_call<ResizeSurfDesc>(c, "bsx_resize_surfaces_batch", planned, &c->rsz_surf_ring, false, "resizing a batch of surfaces", stream,
    [&](int i, ResizeSurfDesc* d) {
      const bsx_resize_surface_item& it = items[i];
      if (const int rc = bg_tab(c, it.sw, it.sh, it.dw, it.dh, &t)) return rc;
      *d = ResizeSurfDesc{it.d_y, it.d_uv, it.d_dst, t->tab.xofs, t->tab.xa, t->tab.yofs, t->tab.ya, it.pitch_y, it.pitch_uv, it.sw, it.sh, t->tab.mode, 0};
      return (int)BSX_OK;
    },
    [&](const ResizeSurfDesc* d, const PictureGrid& g, hipStream_t s) { return launch_resize_surfaces(d, g.spans, g.sizes, s); });
}

int bsx_bgr_to_yuyv(bsx_ctx* c, const uint8_t* d_bgr, uint8_t* d_yuyv, int w, int h, int n, void* stream) {
  if (!c || !d_bgr || !d_yuyv || w <= 0 || h <= 0 || n <= 0) return BSX_EINVAL;
  DeviceGuard guard(c->device);
  BSX_HIP(c, launch_bgr_to_yuyv(d_bgr, d_yuyv, w, h, n, pick(c, stream)));
  return BSX_OK;
}

int bsx_bgr_to_nv12(bsx_ctx* c, const uint8_t* d_bgr, int w, int h, int n, uint8_t* d_y, int pitch_y, uint8_t* d_uv, int pitch_uv, void* stream) {
  const char* fn = "bsx_bgr_to_nv12";
  if (!c) return BSX_EINVAL;
  if (!d_bgr || !d_y || !d_uv) return refuse(c, fn, "d_bgr %p, d_y %p or d_uv %p is NULL", (const void*)d_bgr, (const void*)d_y, (const void*)d_uv);
  if (w <= 0 || h <= 0 || n <= 0) return refuse(c, fn, "w = %d, h = %d and n = %d must be positive", w, h, n);
  if ((w | h) & 1) return refuse(c, fn, "NV12 needs an even width and height (%d x %d)", w, h);
  if (pitch_y < w || (pitch_y & 3)) return refuse(c, fn, "pitch_y = %d must be a multiple of 4 and at least w = %d", pitch_y, w);
  if (pitch_uv < w || (pitch_uv & 3)) return refuse(c, fn, "pitch_uv = %d must be a multiple of 4 and at least w = %d", pitch_uv, w);
  if ((uintptr_t)d_y & 3) return refuse(c, fn, "d_y %p is not 4-byte aligned", (const void*)d_y);
  if ((uintptr_t)d_uv & 3) return refuse(c, fn, "d_uv %p is not 4-byte aligned", (const void*)d_uv);
  DeviceGuard guard(c->device);
  BSX_HIP(c, launch_bgr_to_nv12(d_bgr, w, h, n, d_y, pitch_y, d_uv, pitch_uv, pick(c, stream)));
  return BSX_OK;
}

int bsx_nv12_to_bgr(bsx_ctx* c, const uint8_t* d_y, int pitch_y, const uint8_t* d_uv, int pitch_uv, int w, int h, int n, uint8_t* d_bgr, void* stream) {
  const char* fn = "bsx_nv12_to_bgr";
  if (!c) return BSX_EINVAL;
  if (!d_y || !d_uv || !d_bgr) return refuse(c, fn, "d_y %p, d_uv %p or d_bgr %p is NULL", (const void*)d_y, (const void*)d_uv, (const void*)d_bgr);
  if (w <= 0 || h <= 0 || n <= 0) return refuse(c, fn, "w = %d, h = %d and n = %d must be positive", w, h, n);
  if ((w | h) & 1) return refuse(c, fn, "NV12 needs an even width and height (%d x %d)", w, h);
  if (pitch_y < w || (pitch_y & 3)) return refuse(c, fn, "pitch_y = %d must be a multiple of 4 and at least w = %d", pitch_y, w);
  if (pitch_uv < w || (pitch_uv & 3)) return refuse(c, fn, "pitch_uv = %d must be a multiple of 4 and at least w = %d", pitch_uv, w);
  if ((uintptr_t)d_y & 3) return refuse(c, fn, "d_y %p is not 4-byte aligned", (const void*)d_y);
  if ((uintptr_t)d_uv & 3) return refuse(c, fn, "d_uv %p is not 4-byte aligned", (const void*)d_uv);
  DeviceGuard guard(c->device);
  BSX_HIP(c, launch_nv12_to_bgr(d_y, pitch_y, d_uv, pitch_uv, w, h, n, d_bgr, pick(c, stream)));
  return BSX_OK;
}

int bsx_yuyv_to_bgr(bsx_ctx* c, const uint8_t* d_yuyv, uint8_t* d_bgr, int w, int h, int n, void* stream) {
  if (!c || !d_yuyv || !d_bgr || w <= 0 || h <= 0 || n <= 0 || (((long)w * h) & 1)) return BSX_EINVAL;
  DeviceGuard guard(c->device);
  BSX_HIP(c, launch_yuyv_to_bgr(d_yuyv, d_bgr, w, h, n, pick(c, stream)));
  return BSX_OK;
}

int bsx_debug_buffer(bsx_ctx* c, int which, void** d_ptr, size_t* bytes) {
  if (!c || !d_ptr || !bytes) return BSX_EINVAL;
  const size_t N = (size_t)c->n_streams;
  switch (which) {
    case 0: *d_ptr = c->tensor_ptr(c->plan.input); *bytes = N * c->inW * c->inH * c->inC * 4; break;
    case 1: *d_ptr = c->tensor_ptr(c->plan.output); *bytes = N * c->outW * c->outH * c->outC * 4; break;
    case 2: *d_ptr = c->d_ofinal; *bytes = N * c->outW * c->outH; break;
    case 3: *d_ptr = c->d_masks; *bytes = c->mask_bytes; break;
    case 4:                                                       // what the step's prep writes where the stem has a byte path (in_u8); the f32 form stays unwritten there
      if (!c->in_u8) return refuse(c, "bsx_debug_buffer", "which = 4: this context's stem reads the f32 network input, the 8-bit form is never written");
      *d_ptr = c->d_net_in_u8; *bytes = N * c->inW * c->inH * sizeof(uint32_t); break;
    default: return BSX_EINVAL;
  }
  return BSX_OK;
}

int bsx_debug_run_stage(bsx_ctx* c, int stage, const uint8_t* d_frames, int n, void* stream) {
  if (!c || n <= 0 || n > c->n_streams) return BSX_EINVAL;
  if (const int rc = refuse_geoms(c, "bsx_debug_run_stage")) return rc;
  if (stage >= 1 && stage <= 3) { if (const int rc = refuse_pending(c, "bsx_debug_run_stage")) return rc; }
  DeviceGuard guard(c->device);
  hipStream_t s = pick(c, stream);
  switch (stage) {
    case 0: if (!d_frames) return BSX_EINVAL; return run_prep(c, d_frames, n, s, true);
    case 1: return run_infer(c, n, s);
    case 2: return run_decode(c, n, s);
    case 3: return run_mask(c, n, s);
    case 4:                                                       // stage 0 on raw YUYV 4:2:2 frames (BSX_STEP_YUYV_IN's prep): the f32 network input, for the stage tests
      if (!d_frames || !prep_yuyv_fusable(c->width, c->roi, c->tab_down.tab)) return BSX_EINVAL;
      return run_prep(c, d_frames, n, s, true, true);
    default: return BSX_EINVAL;
  }
}

int bsx_profile_batch(bsx_ctx* c, const uint8_t* d_frames, const uint8_t* d_bg, size_t bg_stride, uint8_t* d_out, int n, int iters,
                      bsx_launch_stat* out, int cap, void* stream) {
  if (!c || !d_frames || !d_bg || !d_out || !out || n <= 0 || n > c->n_streams || iters <= 0) return BSX_EINVAL;
  if (const int rc = refuse_geoms(c, "bsx_profile_batch")) return rc;
  if (const int rc = refuse_pending(c, "bsx_profile_batch")) return rc;
  DeviceGuard guard(c->device);
  hipStream_t s = pick(c, stream);
  const bool seg = c->use_program && c->plan.seg.on;
  const bool fused_decode = infer_decodes(c);
  const bool atail = argmax_tail(c);
  const int n_net = c->use_program ? (seg ? (c->plan.seg.tail.pre_gate_off >= 0 && !k3_frame_runs(c) ? 6 : 5) : 1) : (int)c->plan.steps.size();
  const bool fuse_tail = tile_fusable(c, StepReq{d_frames, d_bg, bg_stride, d_out, c->width, c->height, n, 0u, s, nullptr});
  const int L = 1 + n_net + (fused_decode ? 0 : 1) + (fuse_tail ? 1 : 2) + (fuse_tail ? 1 : 0);   // + a stand-alone blend launch when the step's tail is fused
  if (cap < L) return BSX_EINVAL;
  // ONE event between consecutive launches (L + 1 events, not 2 L): the per-launch figures add up to the pass and carry one event's cost each instead of two
  LaunchTimer t{std::vector<hipEvent_t>((size_t)L + 1, nullptr)};
  for (auto& e : t.ev) BSX_HIP(c, hipEventCreate(&e));
  std::vector<double> sum(L, 0.0);
  const double N = n, px = (double)c->width * c->height;
  for (int it = 0; it < iters; it++) {
    t.k = 0;
    BSX_HIP(c, hipEventRecord(t.ev[0], s));
    // the step's own launch sequence (bsx_step_batch on the same buffers), an event behind each launch
    if (const int rc = enqueue_masks(c, d_frames, n, s, false, 0, nullptr, &t)) return rc;
    if (fuse_tail) {
      BSX_LAUNCH(c, &t, s, launch_mask_blend(c->d_ofinal, c->outW, c->outH, c->in_roi, c->tab_up.tab, c->d_masks, c->width, c->height, c->roi, d_bg, bg_stride,
                                             d_frames, d_out, n, s));
    } else if (const int rc = run_mask(c, n, s, 0, nullptr, &t)) return rc;
    // not part of a fused step: the plain alpha-blend kernel (bsx_composite_batch) on the same buffers, for its own roofline line
    BSX_LAUNCH(c, &t, s, launch_blend(d_bg, bg_stride, d_frames, c->d_masks, d_out, (size_t)c->width * c->height, n, s));
    BSX_HIP(c, hipStreamSynchronize(s));
    if (t.k != L) { c->last_error = "error: bsx_profile_batch: the step made fewer launches than the profile counts\n"; return BSX_EDEVICE; }
    for (int j = 0; j < L; j++) { float ms = 0; BSX_HIP(c, hipEventElapsedTime(&ms, t.ev[j], t.ev[j + 1])); sum[j] += ms; }
  }
  auto put = [&](int j, const std::string& name, double bytes, double flops) {
    memset(&out[j], 0, sizeof out[j]);
    snprintf(out[j].name, sizeof out[j].name, "%s", name.c_str());
    out[j].avg_ms = sum[j] / iters; out[j].bytes = bytes; out[j].flops = flops;
  };
  int j = 0;
  const double canvas = (double)c->inW * c->inH;
  // prep_resize: reads the TOUCHED source pixels of the ROI — a bilinear tap pair per destination column / row, i.e. at most 2 x 2 source
  // pixels per canvas pixel of in_roi (a 5x down-scale touches 16 % of the ROI)
  const double touched = (double)std::min(c->roi.w, 2 * c->in_roi.w) * (double)std::min(c->roi.h, 2 * c->in_roi.h);
  put(j++, "prep", N * (3.0 * touched + (c->in_u8 ? 4.0 : 12.0) * canvas), 0);       // touched source pixels in, the network input out
  if (seg) {
    // algorithmic bytes of each segment = the tensors it must read once + write once (f32); flops from the fused steps it covers
    const std::vector<Step>& S = c->plan.steps;
    const int NS = (int)S.size();
    auto macs = [&](int a, int b) { double m = 0; for (int i = a; i <= b; i++) m += S[i].macs; return m; };
    const SegPlan& sp = c->plan.seg;
    const double eA = 16.0 * sp.head.H1 * sp.head.W1, eb0 = 16.0 * sp.head.H2 * sp.head.W2, ec0 = (double)sp.k2.dw.C * sp.k2.H3 * sp.k2.W3;
    const double elo2 = 16.0 * sp.k3.HL * sp.k3.WL, elo = 16.0 * sp.k3.H2 * sp.k3.W2;
    const double ein = (double)c->inW * c->inH * c->inC, eout = (double)c->outW * c->outH * c->outC;
    put(j++, "seg_head", N * ((c->in_u8 ? 4.0 * c->inW * c->inH : 4.0 * ein) + 4.0 * (eA + eb0)), N * 2.0 * macs(0, 2));
    put(j++, "seg_k2", N * 4.0 * (eb0 + eb0 + ec0), N * 2.0 * macs(3, 8));
    put(j++, "frame_program", N * 4.0 * (ec0 + elo2) + 4.0 * c->plan.weights.size(), N * 2.0 * macs(9, NS - 11));
    const double egate = 16.0 * (sp.tail.gate.part[0].n + sp.tail.gate.part[1].n) + 16.0, fgate = 2.0 * macs(NS - 5, NS - 4);      // the tail's gate, once per frame
    if (k3_frame_runs(c)) put(j++, "seg_k3", N * 4.0 * (eb0 + elo2 + elo + egate), N * (2.0 * macs(NS - 10, NS - 8) + fgate));      // the per-frame form: the gate's work is this launch's
    else {
      put(j++, "seg_k3", N * 4.0 * (eb0 + elo2 + elo), N * 2.0 * macs(NS - 10, NS - 8));
      if (sp.tail.pre_gate_off >= 0) put(j++, "seg_gate", N * 4.0 * egate, 0);
    }
    put(j++, fused_decode ? "seg_tail+decode" : "seg_tail", N * (4.0 * (eA + elo) + (fused_decode ? 2.0 * c->outW * c->outH : 4.0 * eout)), N * 2.0 * macs(NS - 7, NS - 1));
  } else if (c->use_program) {
    // algorithmic bytes of the fused network = its input tensor + its output tensor + the weights once
    double io = (double)c->inW * c->inH * c->inC + (double)c->outW * c->outH * c->outC;
    put(j++, "frame_program", N * io * 4.0 + 4.0 * c->plan.weights.size(), N * 2.0 * c->plan.macs_per_frame);
  } else
  for (const Step& st : c->plan.steps) {
    double in = (double)st.H * st.W * st.Cin, o = (double)st.OH * st.OW * st.Cout, b = 0;
    switch (st.kind) {
      case StepKind::Eltwise: b = in + o + (st.elt == kEltUnary ? 0 : (st.bcast1 ? st.Cin : in)) + (st.elt == kEltMulAdd ? in : 0); break;
      case StepKind::Concat: b = 2 * o; break;
      case StepKind::Gap: b = in + st.Cin; break;
      default: b = in + o + (st.residual >= 0 ? o : 0) + (st.in_scale >= 0 ? st.Cin : 0); break;
    }
    const bool is_tail = atail && &st == &c->plan.steps.back();
    const bool ir_on = c->d_weights16 && c->f16_terms > 0;
    const bool h0 = c->plan.steps[0].fuse_head0;
    const bool h0_member = h0 && (&st == &c->plan.steps[1] || &st == &c->plan.steps[2]);
    if (h0_member || (st.fused_away && !(h0 && &st <= &c->plan.steps[2]) && ir_on)) { put(j++, st.label + " (inside the launch before)", 0, 0); continue; }   // no-op slot of a fused group
    if (st.chain_mid >= 0 && chain3_on(c->plan, st.chain_mid, n, c->d_weights16, c->f16_terms)) { put(j++, st.label + " (inside the chained launch)", 0, 0); continue; }
    if (st.chain_first >= 0 && chain3_on(c->plan, (int)(&st - c->plan.steps.data()), n, c->d_weights16, c->f16_terms)) {      // three 1x1 convolutions: reads the first one's input, writes the last one's output
      const Step& ca = c->plan.steps[st.chain_first];
      const Step& cc = c->plan.steps[st.chain_last];
      put(j++, ca.label + "+" + st.label + "+" + cc.label, N * 4.0 * ((double)ca.H * ca.W * ca.Cin + (double)cc.OH * cc.OW * cc.Cout), N * 2.0 * (ca.macs + st.macs + cc.macs));
      continue;
    }
    if (st.fuse_head0 && h0) {                                   // stem + depthwise + 1x1: reads the network input, writes the 1x1's output
      const Step& d1 = c->plan.steps[1];
      const Step& p2 = c->plan.steps[2];
      put(j++, st.label + "+" + d1.label + "+" + p2.label, N * ((c->in_u8 ? 4.0 * st.H * st.W : 4.0 * in) + 4.0 * (double)p2.OH * p2.OW * p2.Cout), N * 2.0 * (st.macs + d1.macs + p2.macs));
      continue;
    }
    if (st.fuse_dw >= 0 && ir_on) {                              // expand + depthwise in one launch: reads the expand's input, writes the depthwise's output
      const Step& dd = c->plan.steps[st.fuse_dw];
      put(j++, st.label + "+" + dd.label, N * 4.0 * (in + (double)dd.OH * dd.OW * dd.Cout), N * 2.0 * (st.macs + dd.macs));
      continue;
    }
    put(j++, is_tail ? st.label + "+argmax" : st.label, is_tail ? N * (4.0 * in + 2.0 * st.OH * st.OW) : N * b * 4.0, N * 2.0 * st.macs);
  }
  if (!fused_decode) put(j++, "decode_iir", N * ((double)c->outW * c->outH * c->outC * 4.0 + 2.0 * c->outW * c->outH), 0);
  if (fuse_tail) {
    // fused: model-res mask in, full-res mask out (1 B/px), bg + frame in (6 B/px), composite out (3 B/px)
    put(j++, "mask_blend", N * ((double)c->in_roi.w * c->in_roi.h + 10.0 * px), 0);
    put(j++, "blend(standalone)", N * 10.0 * px, 0);
  } else {
    put(j++, "mask_upscale_blur", N * ((double)c->in_roi.w * c->in_roi.h + (double)c->roi.w * c->roi.h), 0);
    put(j++, "blend", N * 10.0 * px, 0);
  }
  return j;
}

int bsx_debug_mask_tile_stats(bsx_ctx* c, int n, long* out4) {
  if (!c || !out4 || n <= 0 || n > c->n_streams) return BSX_EINVAL;
  if (const int rc = refuse_geoms(c, "bsx_debug_mask_tile_stats")) return rc;
  DeviceGuard guard(c->device);
  out4[0] = (long)c->tiles_per_frame * n; out4[1] = out4[2] = 0; out4[3] = out4[0];
  if (!c->d_tile_class) return BSX_OK;                          // generic kernel / shortcut off: every tile is general
  // the classifier the launches themselves run, on the current temporal state
  BSX_HIP(c, launch_tile_class(c->d_ofinal, c->outW, c->outH, c->in_roi, c->tab_up.tab, c->roi, n, nullptr));
  std::vector<uint8_t> cls((size_t)out4[0]);
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(cls.data(), c->d_tile_class, cls.size(), hipMemcpyDeviceToHost) != hipSuccess) return BSX_EDEVICE;
  out4[3] = 0;
  for (uint8_t v : cls) out4[v == 1 ? 1 : (v == 2 ? 2 : 3)]++;
  return BSX_OK;
}

int bsx_debug_gauss_coeffs(int ksize, int shift, uint32_t* c4, uint32_t* c2) {
  return (c4 && c2 && gauss_coeff_words(ksize, shift, c4, c2)) ? BSX_OK : BSX_EINVAL;
}

int bsx_debug_program_timeline(bsx_ctx* c, int n, unsigned long long* ticks, int cap, void* stream) {
  if (!c || !ticks || n <= 0 || n > c->n_streams) return BSX_EINVAL;
  DeviceGuard guard(c->device);
  if (!c->use_program) return 0;
  const int L = (int)c->plan.program.size();
  if (cap < L + 1 || L + 1 > 256) return BSX_EINVAL;
  unsigned long long* d = nullptr;
  const size_t kTl = 1024 + 64 * 16 * 4;       // coarse stamps [0,256), sub-phase accumulators [256,512), fine per-wave stamps [1024, ..)
  BSX_HIP(c, hipMalloc(&d, kTl * sizeof(unsigned long long)));
  BSX_HIP(c, hipMemset(d, 0, kTl * sizeof(unsigned long long)));
  hipStream_t s = pick(c, stream);
  BSX_HIP(c, launch_program(c, n, s, d));
  BSX_HIP(c, hipStreamSynchronize(s));
  BSX_HIP(c, hipMemcpy(ticks, d, std::min((size_t)cap, kTl) * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  (void)hipFree(d);
  return L;
}

int bsx_model_describe(const char* model_path, char* buf, size_t cap) {
  if (!model_path || !buf || !cap) return BSX_EINVAL;
  std::string err, out;
  int rc = BSX_OK;
  try {
  Graph g; Plan p;
  if (!load_tflite(model_path, &g, &err) || !build_plan(g, &p, &err)) { out = err; rc = BSX_EMODEL; }
  else {
    char head[256];
    snprintf(head, sizeof head, "ops=%d nodes=%d steps=%d macs=%.0f arena_floats=%zu\n", g.n_file_ops, (int)g.nodes.size(), (int)p.steps.size(),
             p.macs_per_frame, p.arena_floats_per_stream);
    out = head + p.describe();
    snprintf(head, sizeof head, "program micro-ops=%zu lds_floats=%d lds_tensors=%d hbm_tensors=%d arena_bytes_per_frame=%ld placement_policy=%u lds_blocks=%zu lds_check=%s\n", p.program.size(),
             p.program_lds_floats, p.program_lds_tensors, p.program_global_tensors, p.program_arena_bytes, p.program_policy, p.program_blocks.size(), p.program_check.c_str());
    out += head;
    for (size_t i = 0; i < p.program_labels.size(); i++)
      out += "P" + std::to_string(i) + " " + p.program_labels[i] + (i < p.program_out_tensor.size() ? " -> t" + std::to_string(p.program_out_tensor[i]) : std::string()) + "\n";
    if (p.seg.on) out += p.seg_text;
    if (!p.program.empty()) out += mid_barrier_line(p, false);
    if (BSX_DBG_ENV("BSX_PLAN_BLOCKS"))           // debugging: the LDS reservations of the program (float offset, length, first / last step, owner)
      for (const auto& b : p.program_blocks) { snprintf(head, sizeof head, "block off=%d len=%d steps=[%d,%d] %s\n", b.off, b.len, b.from, b.until, b.what.c_str()); out += head; }
  }
  } catch (const std::exception& e) { out = std::string("exception while reading the model: ") + e.what(); rc = BSX_EMODEL; }
  catch (...) { out = "unknown exception while reading the model"; rc = BSX_EMODEL; }
  snprintf(buf, cap, "%s", out.c_str());
  return rc;
}

long bsx_model_kernel_source(const char* model_path, char* buf, size_t cap) {
  if (!model_path || !buf || !cap) return BSX_EINVAL;
  try {
    Graph g; Plan p;
    std::string err;
    if (!load_tflite(model_path, &g, &err) || !build_plan(g, &p, &err)) { snprintf(buf, cap, "%s", err.c_str()); return BSX_EMODEL; }
    if (p.program.empty()) { snprintf(buf, cap, "no program"); return 0; }
    // the source of the kernel a context would RUN (the form build_specialised picks: compiles, no GPU needed); a compiler failure still shows the source, a graph
    // without a body shows why
    const SpecialisedCode m = build_specialised(p, kernel_variant(p), "gfx950", kBuildMid).mid;
    snprintf(buf, cap, "%s", (m.source.empty() ? m.why : m.source).c_str());
    return (long)m.source.size();
  } catch (...) { snprintf(buf, cap, "exception while reading the model"); return BSX_EMODEL; }
}

long bsx_model_seg_source(const char* model_path, char* buf, size_t cap) {
  if (!model_path || !buf || !cap) return BSX_EINVAL;
  try {
    Graph g; Plan p;
    std::string err;
    if (!load_tflite(model_path, &g, &err) || !build_plan(g, &p, &err)) { snprintf(buf, cap, "%s", err.c_str()); return BSX_EMODEL; }
    const SpecialisedCode sc = build_specialised(p, kernel_variant(p), "gfx950", kBuildSeg).seg;
    snprintf(buf, cap, "%s", (sc.source.empty() ? sc.why : sc.source).c_str());
    return (long)sc.source.size();
  } catch (...) { snprintf(buf, cap, "exception while reading the model"); return BSX_EMODEL; }
}

int bsx_model_precompile(const char* model_path, const char* arch, char* msg, size_t cap) {
  if (!model_path || !msg || !cap) return BSX_EINVAL;
  try {
    Graph g; Plan p;
    std::string err;
    if (!load_tflite(model_path, &g, &err) || !build_plan(g, &p, &err)) { snprintf(msg, cap, "%s", err.c_str()); return BSX_EMODEL; }
    if (p.program.empty()) { snprintf(msg, cap, "interpreted (no program)"); return BSX_OK; }
    // the variant a context created under the same environment would ask for
    const SpecialisedBuild b = build_specialised(p, kernel_variant(p), arch ? arch : "gfx950");
    const std::string& e = b.mid.fallback;
    if (b.mid.code.empty()) { snprintf(msg, cap, "%s", e.c_str()); return e.compare(0, 19, "interpreted (hipRTC") == 0 ? BSX_EMODEL : BSX_OK; }
    std::string seg_msg;
    if (p.seg.on) {
      if (!b.seg.code.empty()) {
        long worst = 0;
        for (const char* k : {"bsx_seg_head", "bsx_seg_k2", "bsx_seg_k3", "bsx_seg_tail"}) worst = std::max(worst, code_object_scratch_bytes(b.seg.code, k));
        if (b.seg_k3_frame) worst = std::max(worst, code_object_scratch_bytes(b.seg.code, "bsx_seg_k3f"));
        char sm[256];
        snprintf(sm, sizeof sm, "; segment kernels %s (%zu bytes of source, %zu bytes of code object, %ld B of scratch)", b.seg.cached ? "cached" : "compiled", b.seg.source.size(),
                 b.seg.code.size(), worst);
        seg_msg = sm;
      } else {
        seg_msg = "; segment kernels: " + b.seg.fallback;
        if (b.seg.fallback.find("hipRTC:") != std::string::npos) { snprintf(msg, cap, "%s", seg_msg.c_str()); return BSX_EMODEL; }
      }
    }
    snprintf(msg, cap, "%s (%zu bytes of source, %zu bytes of code object, %ld B of scratch%s, cache %s)%s", b.mid.cached ? "cached" : "compiled", b.mid.source.size(),
             b.mid.code.size(), b.scratch, b.opaque_tid ? ", lane indices re-derived per op" : "", rtc_cache_dir().c_str(), seg_msg.c_str());
    return BSX_OK;
  } catch (...) { snprintf(msg, cap, "exception while reading the model"); return BSX_EMODEL; }
}

const char* bsx_plan_describe(bsx_ctx* c) { return c ? c->plan_text.c_str() : ""; }

// An arena offset alone does not mean that the tensor exists: the planner gives every step output one before it decides what stays in LDS, what a fused launch keeps
// in registers and what the generated kernel elides.  Returns why the path that executes this context never writes tensor t to the arena (nullptr: it does) — from
// the plan and from the choices the launchers made for the last network stage (the same predicates: program_op_elided, chain3_on, the ir_on rule of launch_step).
static const char* debug_tensor_unstored(const bsx_ctx* c, int t) {
  const Plan& p = c->plan;
  if (t == p.input) return nullptr;
  if (t == p.output) return c->last_net_logits ? nullptr : "the last network stage decoded inside its final kernel and wrote no logits";
  if (c->use_program) {
    if (p.seg.on && std::find(p.seg_stored.begin(), p.seg_stored.end(), t) != p.seg_stored.end()) return nullptr;
    if (p.seg.on && std::find(p.seg_partials.begin(), p.seg_partials.end(), t) != p.seg_partials.end()) return nullptr;      // (synthetic: past the file's tensors)
    for (size_t i = 0; i < p.program.size() && i < p.program_out_tensor.size(); i++) {
      if (p.program_out_tensor[i] != t) continue;
      if (p.program[i].out.space == kLocLds) return "the frame program keeps it in LDS";
      if (p.program[i].out.space != kLocGlobal) return "the frame program writes it to a buffer of its own";
      if (program_op_elided(c, (int)i)) return "the specialised middle kernel computes it chunk by chunk inside the depthwise that reads it";
      return nullptr;
    }
    return p.seg.on ? "it lives inside a segment kernel or a fused micro-op (LDS / registers only)" : "it lives inside a fused micro-op (LDS / registers only)";
  }
  const int NS = (int)p.steps.size();
  const int n = c->last_net_n > 0 ? c->last_net_n : c->n_streams;
  const bool ir_on = c->d_weights16 && c->f16_terms > 0;                      // launch_step: when the expand + depthwise pairs run as one kernel
  for (int j = 0; j < NS; j++) {
    const Step& st = p.steps[j];
    if (st.out != t) continue;
    if (p.steps[0].fuse_head0 && j < 2) return "the fused head kernel (stem + depthwise + 1x1) keeps it in LDS";
    if (st.fuse_dw >= 0 && ir_on) return "the fused expand + depthwise kernel keeps it in LDS";
    if (st.chain_first >= 0 && chain3_on(p, j, n, c->d_weights16, c->f16_terms)) return "the chained 1x1 kernel keeps it in registers";
    if (st.chain_mid >= 0 && j < st.chain_mid && chain3_on(p, st.chain_mid, n, c->d_weights16, c->f16_terms)) return "the chained 1x1 kernel keeps it in registers";
    return nullptr;
  }
  return "no step of this plan writes it";
}

static long debug_tensor_at(bsx_ctx* c, int t, int stream_idx, float* h_out, long cap) {
  if (!c) return BSX_EINVAL;
  if (t < 0 || t >= (int)c->plan.tensor_off.size() || t >= (int)c->plan.tensor_elems.size() || stream_idx < 0 || stream_idx >= c->n_streams || (h_out && cap < 0)) { c->last_error = "bsx_debug_tensor: tensor or stream index out of range"; return BSX_EINVAL; }
  if (c->plan.tensor_off[t] < 0) { c->last_error = "bsx_debug_tensor: tensor " + std::to_string(t) + " has no place in the arena (a constant, or fused away by the planner)"; return BSX_EINVAL; }
  if (const char* why = debug_tensor_unstored(c, t)) { c->last_error = "bsx_debug_tensor: tensor " + std::to_string(t) + " is never written to the arena on this path: " + why; return BSX_EINVAL; }
  DeviceGuard guard(c->device);
  const long n = c->plan.tensor_elems[t];              // (the plan's count: a rewrite's synthetic tensor — the 1x1 convolution moved below its resize — has no entry in the file's graph)
  if (!h_out) return n;
  // network input / output and the per-launch arena are batch-major (stream i at + i * elems); the per-frame program's arena is frame-major
  const float* p = (t == c->plan.input || t == c->plan.output || !c->use_program) ? c->tensor_ptr(t) + (size_t)stream_idx * (size_t)n
                                                                                 : c->tensor_ptr(t) + (size_t)stream_idx * c->plan.arena_floats_per_stream;
  if (hipDeviceSynchronize() != hipSuccess) return BSX_EDEVICE;
  const size_t take = (size_t)std::min(n, cap);
  if (debug_tensor_half(c, t)) {       // packed halves: stream i's start at half i * elems of a batch-major tensor, at the frame's own arena slice of a frame-major one
    const bool batch_major = !c->use_program;
    const _Float16* ph = reinterpret_cast<const _Float16*>(batch_major ? c->tensor_ptr(t) : p) + (batch_major ? (size_t)stream_idx * (size_t)n : 0);
    std::vector<_Float16> h(take);
    if (take && hipMemcpy(h.data(), ph, sizeof(_Float16) * take, hipMemcpyDeviceToHost) != hipSuccess) return BSX_EDEVICE;
    for (size_t i = 0; i < take; i++) h_out[i] = (float)h[i];
    return n;
  }
  if (hipMemcpy(h_out, p, sizeof(float) * take, hipMemcpyDeviceToHost) != hipSuccess) return BSX_EDEVICE;
  return n;
}

long bsx_debug_tensor_of(bsx_ctx* c, int t, int stream_idx, float* h_out, long cap) { return debug_tensor_at(c, t, stream_idx, h_out, cap); }
long bsx_debug_tensor(bsx_ctx* c, int t, float* h_out, long cap) { return debug_tensor_at(c, t, 0, h_out, cap); }

}  // extern "C"
