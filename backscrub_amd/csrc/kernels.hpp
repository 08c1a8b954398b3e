// kernels.hpp — launch interface of the hand-written gfx950 kernels (kernels_nn.hip,
// kernels_img.hip).  Host-only declarations; everything takes an explicit hipStream_t.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "plan.hpp"
#include "segments.hpp"

namespace bsx {

// ---- network -------------------------------------------------------------------------
// Executes one fused step for `n` streams.  `arena` holds every activation tensor at
// arena + plan.tensor_off[t] * n_cap (frame i of tensor t at + i * elems(t)).
// The network input / output tensors live in their own batch-major buffers (net_in / net_out).
// weights16 / f16_terms: the split-f16 MFMA form of the large pointwise convolutions (Step::w16_off, plan.weights16):
// 3 = hi/lo split of both operands (f32-grade results, the default), 1 = plain f16 inputs (IoU-gated fast mode), 0 = f32 MFMA
// f16_terms: low nibble = MFMA terms (0: f32 MFMA kernels, 1: plain f16 operands, 3: split f16); bit 4 (with 1 term only) = the fused expand+depthwise
// kernels store their output as f16 and the project GEMM that consumes it reads f16 (opt-in reduced-precision storage, BSX_F16_GEMM=fast16)
hipError_t launch_step(const Step& st, const Plan& plan, float* arena, float* net_in, float* net_out, const float* weights, int n, int n_cap,
                       hipStream_t s, const uint16_t* weights16 = nullptr, int f16_terms = 0, const uint32_t* net_in_u8 = nullptr, float in_scale = 0.f, float in_offset = 0.f);
// net_in_u8: the network input as 8-bit pixels (prep_fused_k<2>) — taken by the fused DeepLab head (dl_head0_k<true>), which normalises on load
inline bool head0_u8_ok(const Plan& plan) {
  if (plan.steps.empty() || !plan.steps[0].fuse_head0) return false;
  const Step& st = plan.steps[0];
  return st.in0 == plan.input && (long)(2 * (head0_band_rows(st.W, st.OW) + 2) + 1) * st.W <= 4 * 3 * 512;
}

// Does the chain of three 1x1 convolutions around step `mid` (Step::chain_first / chain_last) run as ONE launch for n streams?  Asked by the three steps'
// launches and by the profile's slot labels: split-f16 MFMA mode, and enough pixels for the GEMM forms (below that the three steps run on their own).
inline bool chain3_on(const Plan& plan, int mid, int n, const uint16_t* weights16, int f16_terms) {
  if (mid < 0 || mid >= (int)plan.steps.size() || plan.steps[mid].chain_first < 0) return false;
  const Step& b = plan.steps[mid];
  const long M = (long)n * b.OH * b.OW;                 // (the kernel indexes its input with 32-bit element offsets: past 2^31 elements the three steps run on their own)
  return weights16 && (f16_terms & 15) == 3 && M >= 8192 && M * plan.steps[b.chain_first].Cin < (1l << 31);
}

// Reduced-precision storage (f16_terms bit 4, BSX_F16_GEMM=fast16): is the output of the fused expand + depthwise pair that starts at step `expand` stored as packed
// halves ([n][OH*OW][C], at the tensor's own arena place) for n streams?  `expand` is the pair's first step, a step of `plan`.  Only when the depthwise output's single reader is a 1x1 convolution that will take the
// f16-input GEMM (Step::in_from_fused_dw, same row rule on both sides).  Asked by the pair's launch and by the read-back entry; ir_out16_planned is the part
// that does not depend on the batch (what the plan text announces).
constexpr long kOut16MinRows = 8192;
inline bool ir_out16_planned(const Plan& plan, const Step& expand, int f16_terms) {
  if (!(f16_terms & 16)) return false;
  const int dw = expand.fuse_dw;
  return dw >= 0 && (size_t)dw + 1 < plan.steps.size() && plan.steps[dw + 1].in_from_fused_dw && plan.steps[dw + 1].in0 == plan.steps[dw].out;
}
inline bool ir_out16(const Plan& plan, const Step& expand, int n, const uint16_t* weights16, int f16_terms, bool no_gemm) {
  if (!weights16 || no_gemm || !ir_out16_planned(plan, expand, f16_terms)) return false;
  const Step& dws = plan.steps[expand.fuse_dw];
  return (long)n * dws.OH * dws.OW >= kOut16MinRows;
}

// DeepLab tail: the graph's final RESIZE_BILINEAR fused with the 21-way argmax + temporal IIR (the full-resolution logits never exist)
bool resize_argmax_fusable(const Step& st);
// generic = the scalar first-maximum scan (what more than 24 classes take; tests force it for the 21-class graph)
hipError_t launch_resize_argmax_iir(const Step& st, const float* lowres_logits, uint8_t* ofinal, int n, hipStream_t s, bool generic = false, const int* slot_of = nullptr);

// Whole-network per-frame program (kernels_frame.hip): one 1024-lane workgroup per stream.
hipError_t frame_program_prepare(int lds_floats);
hipError_t launch_frame_program(const MicroOp* d_ops, int n_ops, int lds_floats, float* arena, long per_frame_floats, float* net_in, float* net_out,
                                const float* weights, int n, hipStream_t s, unsigned long long* timeline = nullptr);

// Spatially-parallel segment kernels around the per-frame program (kernels_seg.hip, segments.hpp)
hipError_t seg_prepare();
hipError_t nn_prepare();          // dynamic-LDS limits of the fused per-launch kernels (kernels_nn.hip), for the current device
// fn: the graph-specialised kernel (specialised.hpp) or nullptr for the ahead-of-time instance; grid, block, dynamic LDS and arguments are the same either way
hipError_t launch_seg_head(hipFunction_t fn, const SegHead& d, float* arena, long per_frame, const void* net_in, const float* weights, int n, hipStream_t s, bool h16, bool u8,
                           float in_scale, float in_offset);
hipError_t launch_seg_k2(hipFunction_t fn, const SegK2& d, float* arena, long per_frame, const float* weights, int n, hipStream_t s, bool h16);
hipError_t launch_seg_k3(hipFunction_t fn, const SegK3& d, float* arena, long per_frame, const float* weights, int n, hipStream_t s, bool h16);
hipError_t launch_seg_k3_frame(hipFunction_t fn, const SegK3F& L, float* arena, long per_frame, const float* weights, int n, hipStream_t s);
hipError_t launch_seg_gate(const SegGate& gt, float* arena, long per_frame, const float* weights, long long out_off, int n, hipStream_t s);
// logits = true: write the network output tensor (debug / stage tests; ahead of time only); false: decode + temporal IIR straight into `ofinal`
hipError_t launch_seg_tail(hipFunction_t fn, const SegTail& d, float* arena, long per_frame, float* net_out, uint8_t* ofinal, const float* weights, bool logits, int n,
                           hipStream_t s, bool h16, const int* slot_of);

// ---- image path ----------------------------------------------------------------------
// slot_of (every launch below that reads or writes per-stream state: the model-resolution temporal state `ofinal` and the persistent full-frame masks):
// nullptr = frame i of the batch owns state slot i (the dense form); else a DEVICE array of n stream ids — frame i's state is slot slot_of[i], while frames,
// backgrounds, outputs and scratch stay indexed by the frame's position.  Read once per workgroup (a scalar load: the frame index is workgroup-uniform).
// Fixed-point bilinear tables of cv::resize(INTER_LINEAR, 8u) for one (src,dst) size pair
// (device arrays; built on the host with the same float/double arithmetic OpenCV uses).
struct ResizeTab {
  const int* xofs = nullptr;     // [dw]  source column (already clamped)
  const short* xa = nullptr;     // [2*dw] horizontal coefficients (a0,a1), sum 2048
  const int* yofs = nullptr;     // [dh]  source row before clamping
  const short* ya = nullptr;     // [2*dh] vertical coefficients (b0,b1)
  int sw = 0, sh = 0, dw = 0, dh = 0;
  int mode = 0;                  // 0 linear, 1 copy (same size), 2 INTER_AREA 2x2 (both scales exactly 2)
  int tile_ok = 0;               // mask_tile_fits(): every mask tile's source block fits the LDS staging area
  // mask up-scale table only: device scratch of one byte per (stream, mask tile), written by tile_class_k right before the tile kernel reads it (1 = the tile's
  // whole source block is 0xFF, 2 = 0x00, 0 = anything else).  nullptr (BSX_NO_UNIFORM_TILES at bsx_new: A/B timing, parity tests) = every tile on the general path
  uint8_t* tile_class = nullptr;
};
bool mask_tile_fits(const int* xofs, const int* yofs, int sw, int sh, int dw, int dh, int shift = 0);      // shift: the first tile column starts `shift` columns left of the ROI (geom_edge_shift)
int mask_tile_width();             // the mask tile kernel's tile geometry (kernels_img.hip: kTW x kTH)
int mask_tile_height();
// classify the mask tiles of n streams into tab.tile_class (see ResizeTab); launch_mask_upscale_blur / launch_mask_blend run it themselves
struct Rect4;
hipError_t launch_tile_class(const uint8_t* ofinal, int outW, int outH, const Rect4& in_roi, const ResizeTab& tab, const Rect4& roi, int n, hipStream_t s,
                             const int* slot_of = nullptr);

struct Rect4 { int x, y, w, h; };
inline bool roi_is_frame(int W, int H, const Rect4& roi) { return roi.x == 0 && roi.y == 0 && roi.w == W && roi.h == H; }      // nothing outside the ROI to fill

// ---- launch rule of the kernels whose workgroups are the tiles of n independent frames (mfma_tile.hpp: xcd_frame_tile), one statement for every launcher ----
// BSX_XCD_TILES (debug build, A/B timing; read once per process): 0 = plain frame-major workgroup order everywhere; 2 = the one-XCD-per-frame order also where it
// measured slower (the fused DeepLab head's bands); unset = 1.
int xcd_tiles_mode();
inline int xcd_frames(int n) { return xcd_tiles_mode() ? n : 0; }      // the kernels' n_frames argument: 0 tells xcd_frame_tile to keep the plain order
// The mask tile launches (mask_tile_k, mask_upscale_blur_k) of n frames: tiles per ROI row / column, the flat grid and nf, the kernels' n_frames argument.
struct MaskTileGrid {
  int ntx, nty, nf;
  bool ok;                       // false: 2^31 workgroups or more — the launcher refuses
  dim3 grid(int rows, int n) const { return dim3((unsigned)(ntx * rows) * (unsigned)n); }      // `rows` of the nty tile rows of each frame
};
MaskTileGrid mask_tile_grid(int W, const Rect4& roi, int n);

struct BilateralParams {
  float space_w[13];
  int off_y[13], off_x[13];
  const float* color_lut;        // [768] device
  float scale, offset;
};

constexpr int kCanvasPad = 2;        // radius of the bilateral filter: the halo of prep_fused_k's tiles (BORDER_REFLECT_101)
bool bilateral_taps_match(const BilateralParams& bp);   // host table order == the kernel's hard-wired 13 taps
// frame ROI ↓ → model canvas → bilateral(5,100,100) → convertTo: ONE kernel, no canvas in memory.  libbackscrub.cc:285-302
// input (f32 [n][inH][inW][3]) and / or input_u8 (R|G<<8|B<<16 [n][inH][inW]): whichever is non-null is written
// yuyv_in: `frames` is YUYV 4:2:2 (2 B/px; BSX_STEP_YUYV_IN) — only where prep_yuyv_fusable() holds
hipError_t launch_prep_fused(const uint8_t* frames, int W, int H, Rect4 roi, float* input, uint32_t* input_u8, int inW, int inH, Rect4 in_roi, ResizeTab tab,
                             BilateralParams bp, int n, hipStream_t s, bool yuyv_in = false);
bool prep_yuyv_fusable(int W, Rect4 roi, const ResizeTab& tab);
// decode + temporal IIR on the model-resolution mask.  libbackscrub.cc:317-357
hipError_t launch_decode(int model_type, const float* logits, uint8_t* ofinal, int npix, int nch, int n, hipStream_t s, const int* slot_of = nullptr);
// ofinal(in_roi) ↑ roi size, 5x5 box blur (REFLECT_101 on the ROI), write into mask(roi).  libbackscrub.cc:367-371
hipError_t launch_mask_upscale_blur(const uint8_t* ofinal, int outW, int outH, Rect4 in_roi, ResizeTab tab, uint8_t* mask, int W, int H,
                                    Rect4 roi, int n, hipStream_t s, const int* slot_of = nullptr);
// mask upscale + blur AND alpha blend of the same tile in one launch (W, roi.x, roi.w multiples of 4, 4-byte aligned images;
// pixels outside the ROI — mask 255 forever — get the background copied)
bool mask_blend_fusable(int W, int H, Rect4 roi, const uint8_t* bg, size_t bg_stride, const uint8_t* frames, const uint8_t* out);
hipError_t launch_mask_blend(const uint8_t* ofinal, int outW, int outH, Rect4 in_roi, ResizeTab tab, uint8_t* mask, int W, int H, Rect4 roi,
                             const uint8_t* bg, size_t bg_stride, const uint8_t* frames, uint8_t* out, int n, hipStream_t s, int yuyv = 0, int lds_pad = 0,
                             const int* slot_of = nullptr);
// bsx_step_batch_mixed: one 16-byte descriptor per position of the batch, read by the mixed instantiations of the mask tile kernels and by outside_roi_mixed_k
// with one uniform load per workgroup.  bg: the position's background (4-byte aligned BGR, any number of positions may share one; unread when the filter is
// off); flags: kMixFlipH / kMixFlipV (the same bits as the tile kernels' flag word) | kMixFilterOff.
constexpr unsigned kMixFlipH = 2u, kMixFlipV = 4u, kMixFilterOff = 32u;
struct alignas(16) MixDesc { const uint8_t* bg; unsigned flags; unsigned pad; };
static_assert(sizeof(MixDesc) == 16, "one 16-byte uniform load per workgroup");
// launch_mask_blend with the background and the flip of each position taken from desc[i] (a DEVICE array of n descriptors) and a filter-off position composited
// from its frame; `flags`: the batch's bits only (bit 0 = YUYV out, bit 3 = no mask store, bit 4 = YUYV frames).  Same geometry as launch_mask_blend.
hipError_t launch_mask_blend_mixed(const uint8_t* ofinal, int outW, int outH, Rect4 in_roi, ResizeTab tab, uint8_t* mask, int W, int H, Rect4 roi,
                                   const MixDesc* desc, const uint8_t* frames, uint8_t* out, int n, hipStream_t s, int flags, const int* slot_of = nullptr);
// ---- bsx_step_batch_geoms: streams of several capture sizes ("geometry classes") in ONE prep launch, ONE network pass, ONE tile-class and ONE tile launch ------
// The two ends of the pipeline that see the capture size read it per position.  Three pieces, each as cheap as its rate of change allows:
//   GeomClass   one constant record per class, uploaded once: capture size, both ROIs, both resize tables, the mask tiling;
//   GeomDesc    one record per position of a call, staged through the context's ring, ORDERED BY CLASS: the position's own frame / output / background / persistent
//               mask pointers, its MixDesc flags, the format of its frame (kGeomYuyvIn) and its state slot;
//   GeomSpans   by value in the kernel arguments: per class the first position and the first workgroup of its segment of the (ragged) grid, and the workgroups
//               one position takes.  A workgroup finds its class with compares on SGPRs, then position = pos[g] + local / per[g] and item = local % per[g] — no load
//               in front of the tile-class byte but the kernel arguments themselves, exactly as in the mixed step; class record and descriptor are two independent
//               uniform loads next to it.  (A binary search through a device prefix array would put a chain of dependent loads there, a per-workgroup table would
//               stage a word per tile per call.)
constexpr int kMaxGeoms = 8;
constexpr unsigned kGeomYuyvIn = 64u;      // GeomDesc::flags: the position's frame is YUYV 4:2:2 (BSX_STREAM_YUYV_IN) — read by the *_fmt launchers' kernels only
struct alignas(16) GeomClass {
  int W, H;
  int ntx, nty;                  // mask tiles per ROI row / column (kTW x kTH)
  Rect4 roi, in_roi;
  ResizeTab down, up;            // ROI -> model canvas (prep), model output -> ROI (mask); up.tile_class is unused (the call's scratch travels as an argument)
};
struct alignas(16) GeomDesc {
  const uint8_t* frame;          // [H][W][3] BGR of the position's class, or [H][W][2] YUYV (Y0 U Y1 V) with kGeomYuyvIn
  uint8_t* out;                  // [H][W][3], or [H][W][2] with the batch's YUYV bit
  const uint8_t* bg;             // the position's background (unread with kMixFilterOff)
  uint8_t* mask;                 // the stream's persistent mask [H][W]
  unsigned flags;                // kMixFlipH | kMixFlipV | kMixFilterOff | kGeomYuyvIn
  int slot;                      // the stream id: ofinal slot
  int pad[2];
};
static_assert(sizeof(GeomDesc) == 48, "three 16-byte uniform loads per workgroup");
struct GeomSpans {
  int pos[kMaxGeoms + 1];        // class g owns positions [pos[g], pos[g + 1]) of the call (empty for a class the call does not touch; entries past the last class = n)
  int wg[kMaxGeoms + 1];         // ... and workgroups [wg[g], wg[g + 1]) of the grid
  int per[kMaxGeoms];            // workgroups per position of class g
};
// frame ROI -> model canvas -> bilateral -> network input of position i at input / input_u8 + i (launch_prep_fused with the geometry of each position's class)
hipError_t launch_prep_geoms(const GeomClass* classes, const GeomDesc* desc, const GeomSpans& spans, float* input, uint32_t* input_u8, int inW, int inH, BilateralParams bp,
                             int n, hipStream_t s);
// launch_mask_blend_mixed with the geometry, buffers and settings of each position: [one outside-ROI launch,] one tile-class launch (tile_class != nullptr), one tile
// launch.  tiles / outside: the ragged grids (per = mask tiles / outside-ROI workgroups of one position, 0 = none); tile_class: one byte per workgroup of `tiles`;
// `flags`: the batch's bits (bit 0 = YUYV out, bit 3 = no mask store).  Every class must satisfy geom_class_fusable.
bool geom_class_fusable(int W, const Rect4& roi, const ResizeTab& up);
int geom_outside_blocks(int W, int H, const Rect4& roi);      // outside-ROI workgroups of one position (0: the ROI is the frame)
bool geom_class_xcd(int W, const Rect4& roi);                // the class's mask tiles of one frame on one XCD (launch_mask_blend's shared_lines rule): bit g of xcd_mask
hipError_t launch_mask_blend_geoms(const GeomClass* classes, const GeomDesc* desc, const GeomSpans& tiles, unsigned xcd_mask, const GeomSpans& outside, const uint8_t* ofinal,
                                   int outW, int outH, uint8_t* tile_class, int n, hipStream_t s, int flags);
// bsx_step_batch_vcam_geoms: the geoms step whose outputs all have the virtual camera's size (out_w x out_h) — [one tile-class launch,] ONE masks-only tile launch
// (the persistent masks, as launch_mask_blend_geoms writes them) and ONE resize pass that reads each position's frame, background and mask taps and writes its d_out:
// the capture-size composite is never stored.  vg: one record per class (a DEVICE array, built once per output size): the capture size, the capture -> output table
// (always linear: the copy and the 2x2 area mode expanded to one) and whether the class takes the per-tap form (!vcam_tile_fits, or the debug switch).
// `flags`: bit 0 = YUYV pack; every d_out 4-byte aligned.
struct alignas(16) VgClass { int W, H, direct, pad; ResizeTab tab; };
hipError_t launch_vcam_geoms(const GeomClass* classes, const VgClass* vg, const GeomDesc* desc, const GeomSpans& tiles, unsigned xcd_mask, const uint8_t* ofinal, int outW,
                             int outH, uint8_t* tile_class, int out_w, int out_h, int n, hipStream_t s, unsigned flags);
// The three launchers above for a call in which at least one position's frame is YUYV 4:2:2 (kGeomYuyvIn in its descriptor): the same launch sequences with
// the kernels that read a frame replaced by forms that choose, per workgroup and on a scalar, between the BGR and the YUYV inclusion of the same bodies — the
// per-position forms of prep_fused_k<OUT, true, true>, mask_tile_k<true, true, false, false, true>, outside_roi_mixed_k's bit 4 and vg_mixed_k<DIRECT, true>.
// Every YUYV position's class must satisfy prep_yuyv_fusable (checked by the caller); a call of BGR positions takes the launchers above, whose code is unchanged.
hipError_t launch_prep_geoms_fmt(const GeomClass* classes, const GeomDesc* desc, const GeomSpans& spans, float* input, uint32_t* input_u8, int inW, int inH,
                                 BilateralParams bp, int n, hipStream_t s);
hipError_t launch_mask_blend_geoms_fmt(const GeomClass* classes, const GeomDesc* desc, const GeomSpans& tiles, unsigned xcd_mask, const GeomSpans& outside,
                                       const uint8_t* ofinal, int outW, int outH, uint8_t* tile_class, int n, hipStream_t s, int flags);
hipError_t launch_vcam_geoms_fmt(const GeomClass* classes, const VgClass* vg, const GeomDesc* desc, const GeomSpans& tiles, unsigned xcd_mask, const uint8_t* ofinal,
                                 int outW, int outH, uint8_t* tile_class, int out_w, int out_h, int n, hipStream_t s, unsigned flags);
// bsx_step_batch_vcam_geoms_outs: launch_vcam_geoms' [tile-class launch and] masks-only tile launch over the call's positions, then ONE resize pass whose ragged grid
// ranges over OUTPUT RECORDS of different sizes instead of positions of one size.  The records are ordered by (class of their item, output size); each such pair
// that occurs is a group:
//   VgOutGroup  one record per group of the call (a DEVICE array, staged per call): the VgClass of (class, size), the tiles per output row and the option bits of
//               the body (bit 0 = YUYV pack, bit 4 = whole-dword stores: launch_vcam_geoms' rule, per size);
//   odesc       one GeomDesc per output record, in group order: the descriptor of the record's position with `out` replaced by the record's buffer;
//   OutSpans    by value in the kernel arguments: per group its first workgroup, its first record and the workgroups of one record (64 x 32 output tiles).  A
//               workgroup finds its group with compares on SGPRs as geom_span does, then record = rec[g] + local / per[g] and tile = local % per[g]: nothing is
//               loaded ahead of the group record and the descriptor, two independent uniform loads.  Entries past the last group: wg = the grid's size.
// outs.wg[kMaxOutGroups] == 0 (no record): the masks-only step.  fmt: some position's frame is YUYV (launch_vcam_geoms_fmt's kernels and rules).
constexpr int kMaxOutGroups = 32;
struct alignas(16) VgOutGroup { VgClass c; int ntx, opt, pad[2]; };
struct OutSpans { int wg[kMaxOutGroups + 1]; int rec[kMaxOutGroups]; int per[kMaxOutGroups]; int ng; };
// ONE launcher for the three forms of the call: nrec NULL — the records are BGR / YUYV; nrec — NV12 records (below); srec with nrec — NV12 frames too (further below).
struct VgNv12Rec;
struct VgSurfRec;
hipError_t launch_vcam_geoms_outs(const GeomClass* classes, const VgOutGroup* groups, const GeomDesc* odesc, const VgNv12Rec* nrec, const VgSurfRec* srec,
                                  const OutSpans& outs, const GeomDesc* desc, const GeomSpans& tiles, unsigned xcd_mask, const uint8_t* ofinal, int outW, int outH,
                                  uint8_t* tile_class, int n, hipStream_t s, bool fmt);
// bsx_step_batch_vcam_geoms_outs_nv12: launch_vcam_geoms_outs with every record written as NV12 — a Y plane (odesc's `out`) and an interleaved UV plane of half the
// rows, each with a row pitch in bytes (multiples of 4, >= out_w; out_w and out_h even; both planes 4-byte aligned).  nrec: one VgNv12Rec per output record, in group
// order like odesc, a DEVICE array staged with it: the kernel reads record r's planes and pitches with the workgroup-uniform index it reads odesc[r] with.  The
// groups' option bits are not read.  The same three launches; the resize pass is vg_outs_nv12_k (vg_outs_nv12_fmt_k with fmt).
struct alignas(16) VgNv12Rec { uint8_t* uv; int pitch_y, pitch_uv; };
// bsx_step_batch_surfaces: launch_prep_geoms and launch_vcam_geoms_outs with NV12 records for positions whose frames are all NV12 SURFACES — desc[i].frame is position i's Y
// plane ([H] rows of pitch_y bytes), srec[i] its interleaved UV plane ([H / 2] rows of pitch_uv bytes) and the two pitches (multiples of 4, >= W; both planes 4-byte
// aligned; W and H even).  srec: a DEVICE array staged behind the call's descriptors, read with one 16-byte uniform load; an OUTPUT record's descriptor names its
// position (the index into srec) in pad[0].  Pixel (x, y) of the frame is Y[y][x] with the chroma pair UV[y >> 1][x & ~1 ..], converted with cv::COLOR_YUV2BGR_YUYV's
// integers: the BGR frame is launch_yuyv_to_bgr of the 4:2:2 image whose row y repeats chroma row y >> 1.  No load touches a byte at or past W of a row.  Every class
// of the call must satisfy prep_nv12_fusable (the proper INTER_LINEAR down-scale table, W and H even, W >= 4); the prep kernel is prep_geoms_nv12_k, the resize pass
// vg_outs_nv12in_k, tile_class_geoms_k and mask_geoms_k are those of every other form.
struct alignas(16) VgSurfRec { const uint8_t* uv; int pitch_y, pitch_uv; };
bool prep_nv12_fusable(int W, int H, const ResizeTab& tab);
hipError_t launch_prep_geoms_nv12(const GeomClass* classes, const GeomDesc* desc, const VgSurfRec* srec, const GeomSpans& spans, float* input, uint32_t* input_u8, int inW,
                                  int inH, BilateralParams bp, int n, hipStream_t s);
// ---- classes off the 4-pixel grid (bsx_new_geoms_ex with BSX_GEOMS_EDGE_ROI): W % 4 == 0, roi.x and roi.w free ----------------------------------------------------
// The composite moves in 4-pixel groups of three aligned dwords, so the groups are anchored to the FRAME: with s = roi.x & 3 (geom_edge_shift) tile column tbx of a
// class starts at ROI-relative column 128 tbx - s, and a class has ceil((s + roi.w) / 128) tile columns (geom_tile_cols: GeomClass::ntx, the spans and the tile-class
// scratch all count those).  The tile launch owns every group that intersects the ROI — a straddling group's pixels outside the ROI have mask 255 by definition: their
// composite is the background (the frame with the filter off) and their mask bytes are not stored — the outside-ROI launch the groups wholly outside.  A class on the
// grid (s = 0, roi.w % 4 == 0) is the same record either way.  launch_mask_blend_geoms_edge is launch_mask_blend_geoms_fmt's launch sequence with kernels of its own
// that take every class in this form and every position in its own format; a call that touches no such class takes the launchers above.  The vcam launchers need no
// such form (their tile kernel stores masks only, bytewise at ragged edges): they are given class records whose ntx counts ROI-anchored columns.
constexpr int geom_edge_shift(const Rect4& roi) { return roi.x & 3; }      // (constexpr: host and device code both call it)
int geom_tile_cols(const Rect4& roi, bool edge);             // tile columns of one frame: ROI-anchored, or frame-anchored for the edge launcher
inline bool geom_class_on_grid(const Rect4& roi) { return (roi.x & 3) == 0 && (roi.w & 3) == 0; }
bool geom_class_edge_fusable(int W, const Rect4& roi, const ResizeTab& up, bool shifted_tiles_fit);      // shifted_tiles_fit: mask_tile_fits(.., geom_edge_shift(roi)) of `up`
hipError_t launch_mask_blend_geoms_edge(const GeomClass* classes, const GeomDesc* desc, const GeomSpans& tiles, unsigned xcd_mask, const GeomSpans& outside,
                                        const uint8_t* ofinal, int outW, int outH, uint8_t* tile_class, int n, hipStream_t s, int flags);
// alpha blend.  deepseg.cc:108-134
hipError_t launch_blend(const uint8_t* bg, size_t bg_stride, const uint8_t* frames, const uint8_t* masks, uint8_t* out, size_t npix,
                        int n, hipStream_t s, const int* slot_of = nullptr);
// generic BGR resize (background → frame size).  background.cc:186,190
hipError_t launch_resize_bgr(const uint8_t* src, uint8_t* dst, ResizeTab tab, int n, hipStream_t s);
// n resizes to ONE output size in ONE launch (bsx_resize_bgr_batch): block row i of the grid reads desc[i] (a DEVICE array, one uniform load per workgroup) —
// its source, its destination (dw x dh x 3 bytes, any alignment: a 4-byte aligned one with dw % 4 == 0 is stored as dwords) and the table of (sw x sh -> dw x dh),
// whose mode (ResizeTab::mode) may differ from one descriptor to the next.  The integers of launch_resize_bgr.
struct alignas(16) ResizeBatchDesc {
  const uint8_t* src; uint8_t* dst;
  const int* xofs; const short* xa; const int* yofs; const short* ya;     // ResizeTab's tables (null in modes 1 and 2)
  int sw, sh, mode, pad;
};
static_assert(sizeof(ResizeBatchDesc) == 64, "four 16-byte uniform loads per workgroup");
hipError_t launch_resize_bgr_batch(const ResizeBatchDesc* desc, int n, int dw, int dh, hipStream_t s);
// BGR → YUYV.  deepseg.cc:87-106
hipError_t launch_bgr_to_yuyv(const uint8_t* bgr, uint8_t* yuyv, int w, int h, int n, hipStream_t s);
// BGR → NV12: n tight [h][w][3] images into pitched planes, image i's at y + i * pitch_y * h and uv + i * pitch_uv * (h / 2).  w, h even; pitches multiples of 4,
// >= w; planes 4-byte aligned.  Y and chroma are launch_bgr_to_yuyv's bytes, the chroma averaged (truncating) over each pair of rows: UV[r][2c] is the mean of byte 1
// of the 4:2:2 words (2r, c) and (2r + 1, c), UV[r][2c + 1] that of byte 3.  Bytes [w, pitch) of a row are not written.
hipError_t launch_bgr_to_nv12(const uint8_t* bgr, int w, int h, int n, uint8_t* y, int pitch_y, uint8_t* uv, int pitch_uv, hipStream_t s);
// NV12 → BGR: launch_bgr_to_nv12's layout read back — n pitched surfaces into tight [h][w][3] images.  The bytes of launch_yuyv_to_bgr applied to the 4:2:2 image
// Q[y][c] = (Y[y][2c], UV[y / 2][2c], Y[y][2c + 1], UV[y / 2][2c + 1]).  Bytes [w, pitch) of a row are not read.  bgr: any alignment.
hipError_t launch_nv12_to_bgr(const uint8_t* y, int pitch_y, const uint8_t* uv, int pitch_uv, int w, int h, int n, uint8_t* bgr, hipStream_t s);
// YUYV → BGR ingest.  deepseg.cc:553 (CAP_PROP_CONVERT_RGB), :725
hipError_t launch_yuyv_to_bgr(const uint8_t* yuyv, uint8_t* bgr, int w, int h, int n, hipStream_t s);
// cv::flip of the composited frame (code as cv::flip: 0 vertical, >0 horizontal, <0 both).  deepseg.cc:667-673
hipError_t launch_flip_bgr(const uint8_t* src, uint8_t* dst, int w, int h, int code, int n, hipStream_t s);
// cv::GaussianBlur(Size(ksize, ksize), sigma 0) of packed BGR u8 images (dst != src), ksize odd <= 31.  deepseg.cc:657-658 (-p bgblur:N)
// positions (DEVICE array of n, nullable): image i of the launch is image positions[i] of src and of dst (bsx_step_batch_mixed: the positions of one blur size)
hipError_t launch_gauss_blur(const uint8_t* src, uint8_t* dst, int w, int h, int ksize, int n, hipStream_t s, const int* positions = nullptr);
bool gauss_coeff_words(int ksize, int shift, uint32_t* c4 /* [4][9] */, uint32_t* c2 /* [2][17] */);   // host: the tables launch_gauss_* pass to the kernel
// blur + alpha blend of the frames over their own blur (deepseg.cc:652-661 without -b), the blurred image never stored; fusable = 4-byte aligned images, w % 4 == 0
bool gauss_blend_fusable(const uint8_t* frames, const uint8_t* masks, const uint8_t* out, int w, int ksize);
hipError_t launch_gauss_blend(const uint8_t* frames, const uint8_t* masks, uint8_t* out, int w, int h, int ksize, int n, hipStream_t s, const int* slot_of = nullptr);
// n blurs in ONE launch (bsx_gaussian_blur_bgr_batch): position i reads desc[i] (a DEVICE array ORDERED BY IMAGE SIZE, two 16-byte uniform loads per workgroup) —
// its source (w x h BGR of any alignment, or with kGeomYuyvIn 4-byte aligned YUYV 4:2:2 of an even width), its destination (w x h BGR, any alignment: a 4-byte
// aligned one with w % 4 == 0 is stored as dwords) and its blur size (odd, 1 .. 31; 1 = the image itself, converted for a YUYV source).  spans: the ragged grid —
// per size class the first position, the first workgroup and the 64 x 16 tiles of one image (blur_tiles).  coef: the DEVICE copy of blur_coef_table's records.
// The integers of launch_gauss_blur (after launch_yuyv_to_bgr for a YUYV source).
struct alignas(16) BlurDesc { const uint8_t* src; uint8_t* dst; int w, h, ksize; unsigned flags; };
static_assert(sizeof(BlurDesc) == 32, "two 16-byte uniform loads per workgroup");
struct GaussCoef;
size_t blur_coef_table_bytes();                                   // host: the size of the table, and its records (every odd ksize of 1 .. 31 x both staging paths)
void blur_coef_table(GaussCoef* tab);
inline long blur_tiles(int w, int h) { return (long)((w + 63) / 64) * (long)((h + 15) / 16); }
struct BlurTileCols { int ntx[kMaxGeoms]; };                      // by value next to the spans: tiles per image row of class g (blur_tile_cols of its width)
inline int blur_tile_cols(int w) { return (w + 63) / 64; }
hipError_t launch_blur_batch(const BlurDesc* desc, const GaussCoef* coef, const GeomSpans& spans, const BlurTileCols& cols, hipStream_t s);
// launch_blur_batch for NV12 surfaces (bsx_gaussian_blur_surfaces_batch): position i reads desc[i] (a DEVICE array ORDERED BY SURFACE SIZE, three 16-byte uniform loads
// per workgroup) — its Y plane ([h] rows of pitch_y bytes) and interleaved UV plane ([h / 2] rows of pitch_uv bytes; both planes 4-byte aligned, the pitches multiples
// of 4 and >= w, w and h even, every plane below 2^31 bytes: offsets into a plane are 32-bit), its destination (w x h BGR, any alignment: a 4-byte aligned one with
// w % 4 == 0 is stored as dwords) and its blur size (odd, 1 .. 31; 1 = the conversion alone).  spans, cols and coef as above — the same table.  The integers of
// launch_nv12_to_bgr, then those of launch_gauss_blur; no load touches a byte at or past w of a row.
struct alignas(16) BlurSurfDesc { const uint8_t* y; const uint8_t* uv; uint8_t* dst; int pitch_y, pitch_uv; int w, h, ksize; unsigned flags; };
static_assert(sizeof(BlurSurfDesc) == 48, "three 16-byte uniform loads per workgroup");
hipError_t launch_blur_surfaces(const BlurSurfDesc* desc, const GaussCoef* coef, const GeomSpans& spans, const BlurTileCols& cols, hipStream_t s);
// launch_resize_bgr_batch for NV12 surfaces, every position with an output size of its own (bsx_resize_surfaces_batch): position i reads desc[i] (a DEVICE array ORDERED
// BY DESTINATION SIZE, five 16-byte uniform loads per workgroup) — its Y plane ([sh] rows of pitch_y bytes) and interleaved UV plane ([sh / 2] rows of pitch_uv
// bytes; both planes 4-byte aligned, the pitches multiples of 4 and >= sw, sw and sh even, every plane below 2^31 bytes: offsets into a plane are 32-bit), its
// destination (dw x dh BGR of its class, dw * dh * 3 < 2^31, any alignment: a 4-byte aligned one with dw % 4 == 0 is stored as dwords) and the table of (sw x sh ->
// dw x dh), whose mode may differ from one descriptor to the next.  spans: the ragged grid over destination-size classes, per[g] = resize_surf_blocks of the class;
// sizes: the classes' (dw, dh), by value next to the spans.  The integers of launch_nv12_to_bgr, then those of launch_resize_bgr; no load touches a byte at or past
// sw of a row.
struct alignas(16) ResizeSurfDesc {
  const uint8_t* y; const uint8_t* uv;
  uint8_t* dst; const int* xofs;
  const short* xa; const int* yofs;                                       // ResizeTab's tables (null in modes 1 and 2)
  const short* ya; int pitch_y, pitch_uv;
  int sw, sh, mode, pad;
};
static_assert(sizeof(ResizeSurfDesc) == 80, "five 16-byte uniform loads per workgroup");
struct ResizeDstSizes { int dw[kMaxGeoms], dh[kMaxGeoms]; };
inline long resize_surf_blocks(int dw, int dh) { return (((long)dw + 3) / 4 * (long)dh + 255) / 256; }
hipError_t launch_resize_surfaces(const ResizeSurfDesc* desc, const GeomSpans& spans, const ResizeDstSizes& sizes, hipStream_t s);
// composite at the virtual camera's geometry: alpha blend → cv::flip (flags bits 1-2) → cv::resize to (tab.dw, tab.dh) → [YUYV pack (bit 0)] in one pass over
// frames, background and the persistent masks (deepseg.cc:634-681).  `tab`: a linear table from the capture size (the 2x2 area mode expanded to one);
// direct = !vcam_tile_fits(tab): every tap blended where it is read instead of the footprint staged in LDS.  yuyv_in: `frames` is YUYV 4:2:2
bool vcam_tile_fits(const int* xofs, const int* yofs, int sw, int sh, int dw, int dh);
hipError_t launch_vcam_blend_resize(const uint8_t* frames, bool yuyv_in, const uint8_t* bg, size_t bg_stride, const uint8_t* masks, uint8_t* out, int W, int H,
                                    ResizeTab tab, bool direct, int n, hipStream_t s, unsigned flags);
// the same pass with every position's own settings (bsx_step_batch_vcam_mixed): desc[i] (device) gives position i's background, flip bits and filter switch, its
// mask is slot slot_of[i]'s (device; NULL: slot i).  flags: bit 0 (YUYV pack) only — the flips are the descriptors'.  Any background alignment (byte form per stream)
hipError_t launch_vg_mixed(const uint8_t* frames, bool yuyv_in, const MixDesc* desc, const uint8_t* masks, const int* slot_of, uint8_t* out, int W, int H,
                           ResizeTab tab, bool direct, int n, hipStream_t s, unsigned flags);
// bsx_reset_streams: state slots ids[0..n) (a device array) back to their initial values, ofinal -> 0 and mask -> 255 (what bsx_reset does for every slot)
hipError_t launch_reset_slots(uint8_t* ofinal, size_t ofinal_bytes, uint8_t* masks, size_t mask_bytes, const int* ids, int n, hipStream_t s);
// fill
hipError_t launch_fill_u8(uint8_t* p, uint8_t v, size_t bytes, hipStream_t s);

}  // namespace bsx
