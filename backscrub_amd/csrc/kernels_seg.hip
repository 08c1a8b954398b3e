// kernels_seg.hip — the spatially-parallel segment kernels of the Meet / MLKit networks (segments.hpp).
//
// Every kernel: grid = (tiles per frame, frames), 256 lanes = 4 waves per workgroup, several workgroups per CU.  A workgroup
// owns one tile of its segment's OUTPUT pixels and recomputes the halo its depthwise 3x3 needs; intermediate tensors of the
// tile live in LDS as [pixel][16] rows whose four channel quads are permuted per column (swz_a / swz_b / swz_l below: conflict-free
// for every access pattern used here — MFMA epilogue stores, MFMA operand reads, stride-1 and stride-2 depthwise taps), never in HBM.
//
// 1x1 convolutions and the 3x3 stem run on v_mfma_f32_16x16x4_f32 — exact f32 FMA chains, so the results stay within
// float rounding of the reference order (measured against the oracle: < 1e-5 relative on the logits).  Operand maps as
// in kernels_frame.hip, operands swapped: A lane (li, g) = w[k][channel li]; B lane = x[pixel li][k = 4g..4g+3]; D lane = channels 4g..4g+3 of pixel li —
// 4 consecutive channels of ONE pixel (acc_quad): 16-byte stores everywhere.
//
// Reference operators covered (file:line into /root/reference): Interpreter::Invoke() lib/libbackscrub.cc:307 — CONV_2D,
// DEPTHWISE_CONV_2D, RESIZE_BILINEAR (half-pixel), MUL/ADD gates, AVERAGE_POOL_2D (as partial sums), FULLY_CONNECTED /
// 1x1 gate convs; Convolution2DTransposeBias lib/transpose_conv_bias.cc:37-114; decode + IIR lib/libbackscrub.cc:317-357.
// TWO ways into this file (round 6):
//   * hipcc, ahead of time: every kernel a template instantiation that takes its segment descriptor as a kernel argument — any graph of the family, also what runs when
//     hipRTC is unavailable and what the stage tests' logits variant uses;
//   * hipRTC, when a context is created (gen_seg.cpp: this text + segments.hpp + mfma_tile.hpp flattened by build.py into seg_rtc_src.inc, with BSX_SEG_RTC, the
//     template arguments and the four descriptors of THE LOADED GRAPH as compile-time constants in front): extern "C" kernels bsx_seg_head / _k2 / _k3 / _tail in which
//     every geometry value, weight offset and activation kind is a constant — loops get their trip counts, index arithmetic its strength reduction, dead activation
//     branches disappear.  tools/seg_probe.sh measured that form first (profiles/r06o: head 39.7 -> 36.1 us, k2 40.2 -> 34.6, tail 44.7 -> 41.6, step -3.7 % at configs[1]).
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#endif
#ifndef BSX_SEG_RTC               // (the flattened translation unit of gen_seg.cpp carries segments.hpp and mfma_tile.hpp in front of this text and needs nothing else)
#include "debug_switches.hpp"

#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "kernels.hpp"
#include "mfma_tile.hpp"
#include "segments.hpp"
#endif

// Where the kernels get their descriptor `d` from: the kernel argument (ahead-of-time build), the generator's constants (BSX_SEG_RTC: kSegHEAD ... in front of this text),
// or — tools/seg_probe.sh, the ahead-of-time experiment that preceded the hipRTC form — a dumped file of constants (-DBSX_SEG_PROBE=\"file\": one model only, never shipped).
#if defined(BSX_SEG_RTC)
#define BSX_SEG_D(T, NAME) constexpr T d = kSeg##NAME; (void)d_rt
#elif defined(BSX_SEG_PROBE)
#define BSX_SEG_D(T, NAME) constexpr T d = kProbe##NAME; (void)d_rt
#else
#define BSX_SEG_D(T, NAME) const T& d = d_rt
#endif

namespace bsx {
#ifdef BSX_SEG_RTC
namespace segrtc {               // (named: an extern "C" kernel inside an unnamed namespace would have internal linkage)
BSX_SEG_CONSTANTS                // constexpr SegHead kSegHEAD = ...; kSegK2; kSegK3; kSegTAIL  (gen_seg.cpp)
// the template arguments of the one variant this graph / mode needs
constexpr bool STEM_HSWISH = BSX_SEG_HS != 0, H16 = BSX_SEG_H16 != 0, U8IN = BSX_SEG_U8 != 0, LOGITS = false, SIGMOID = BSX_SEG_SIG != 0;
constexpr int CO = BSX_SEG_CO;
#else
namespace {
#endif
#ifdef BSX_SEG_PROBE
#include BSX_SEG_PROBE
#endif

extern __shared__ __attribute__((aligned(16))) float seg_smem[];

constexpr int kScrGate = 0;      // [0,16) gate vector, [16,48) means, [48,80) hidden
constexpr int kScrRed = 96;      // [96, 96 + 2*256) partial-sum meeting points (two sets of 16 slots x 16 channels)
constexpr int kScrFloats = kSegScratchFloats;  // tiles start here

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
// Activation tensors that cross a kernel boundary (A, b0, B, c0, lo2, lo — SURVEY Appendix B.1) are f32 by default; H16 = the 16-bit activation
// STORAGE mode (BSX_ACT16=1, what SetAllowFp16PrecisionForFp32 permits: /root/reference/lib/libbackscrub.cc:225): the same tensor at the same
// arena offset as packed halves (round to nearest even on store), all arithmetic still f32.  `idx` = element index inside the tensor.
typedef _Float16 h4s __attribute__((ext_vector_type(4)));
template <bool H16> __device__ __forceinline__ float4 ldg4(const float* base, unsigned idx) {
  if (H16) { const h4s h = *reinterpret_cast<const h4s*>(reinterpret_cast<const _Float16*>(base) + idx); return make_float4((float)h.x, (float)h.y, (float)h.z, (float)h.w); }
  return *reinterpret_cast<const float4*>(base + idx);
}
template <bool H16> __device__ __forceinline__ void stg4(float* base, unsigned idx, float4 v) {
  if (H16) *reinterpret_cast<h4s*>(reinterpret_cast<_Float16*>(base) + idx) = h4s{(_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w};
  else *reinterpret_cast<float4*>(base + idx) = v;
}
// What every reader of a half-stored tensor gets back.  A kernel that goes on computing with a value it also stores (the head's 1x1 behind A, k2's behind B, every
// pooled partial sum) uses the STORED value in the 16-bit storage mode: its own arithmetic, the next kernel and the gate's pooled mean then all see one tensor —
// the one in the arena — and each stored tensor can be checked against the tensors it was computed from (tests/test_gpu_layers_reduced.py).  This is part of what
// the mode DEFINES: its results are those of a network whose stored activations are halves, not of the f32 network with halves on the side.
template <bool H16> __device__ __forceinline__ float4 as_stored(float4 v) {
  if (H16) return make_float4((float)(_Float16)v.x, (float)(_Float16)v.y, (float)(_Float16)v.z, (float)(_Float16)v.w);
  return v;
}
// ---- LDS tile layouts (bank model: MI355X_MICROARCH.md §LDS; evaluated for every access pattern of this file by tests/test_lds_layouts.py) ----------------------------
// A tile pixel is 16 floats = four 16-byte channel quads.  Stored densely ([pixel][16], quad q at +4q) the MFMA epilogue's ds_write_b128 — 8 consecutive lanes = 8
// consecutive pixels, ONE quad — touches two of the eight 16-byte slots of its 128-byte window (4-way conflict: 32 LDS cycles for an instruction that costs 13), the MFMA
// operand read (ds_read_b128, 16-lane groups of 8 pixels x 2 quads) is 2-way, and so is every tap of a STRIDE-2 depthwise (even columns only: half of the banks).
// SQ counters of round 4: 55 % (k2), 41 % (head), 40 % (tail) of the LDS-active cycles were conflict cycles.  Three layouts remove all of them:
//   swz_a — stride-1 tiles (k2's B, k3 / tail's z and t): quad q of column x lives at quad position q ^ swz_a(x).  The 8 pixels of an epilogue store then cover all 8
//           slots, the 16 (pixel, quad) pairs of an operand read all 16; the stride-1 depthwise (4 quads of one pixel per lane quad) is conflict-free under any permutation.
//   swz_b — tiles a STRIDE-2 depthwise reads (head's x, k2's x): columns de-interleaved — a row is [even columns | odd columns] — so a tap is a stride-1 read of one plane,
//           and quad position q ^ swz_b(x) (bit 1 = the plane) keeps the epilogue store (lanes alternate planes) on 8 distinct slots.
//   swz_l — the staged low-resolution window (k3 / tail): stride 16 floats instead of 20 (the padding halved nothing: every tap read was 2-way) with a period-16 swizzle under
//           which the 2x up-sampling taps (two neighbouring lanes share a source pixel) are conflict-free for every window alignment: 20 % less LDS for the window as well.
// Written as single-expression functions so that the test evaluates the kernels' own source.
__device__ __forceinline__ int swz_a(int x) { return (x >> 1) & 3; }
__device__ __forceinline__ int swz_b(int x) { return ((x >> 2) & 1) | ((x & 1) << 1); }
__device__ __forceinline__ int swz_l(int x) { return (((x >> 2) & 1) << 1) ^ ((x >> 3) & 1); }
// float offset of quad q of column x inside a tile row: stride-1 layout / de-interleaved layout (half = (row width + 1) / 2 columns in the even plane)
__device__ __forceinline__ int col_a(int x, int q) { return x * 16 + 4 * (q ^ swz_a(x)); }
__device__ __forceinline__ int col_b(int x, int q, int half) { return ((x & 1) * half + (x >> 1)) * 16 + 4 * (q ^ swz_b(x)); }
__device__ __forceinline__ int col_l(int x, int q) { return x * kSegLoStride + 4 * (q ^ swz_l(x)); }

__device__ __forceinline__ float4 f4zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 f4add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 f4fma(float4 a, float4 b, float4 c) { return make_float4(fmaf(a.x, b.x, c.x), fmaf(a.y, b.y, c.y), fmaf(a.z, b.z, c.z), fmaf(a.w, b.w, c.w)); }

// Activations.  none / relu / relu6 are ONE branch-free v_med3_f32 with kernel-uniform bounds (the first version switched on the
// activation code per element: a dozen scalar branches per MFMA tile were most of its SALU stream and of its stalls); hard-swish
// (stems) and the logistic (MLKit's output) are compile-time variants of the kernels that need them.  Same arithmetic forms as the
// per-frame program (hardware exp2 / rcp).
struct Clamp { float lo, hi; };
__device__ __forceinline__ Clamp clamp_of(int act) {               // planner guarantees act in {none, relu, relu6} wherever this is used
  Clamp c;
  c.lo = act == kActNone ? -__builtin_huge_valf() : 0.f;
  c.hi = act == kActRelu6 ? 6.f : __builtin_huge_valf();
  return c;
}
__device__ __forceinline__ float4 clamp4(float4 v, Clamp c) {
  return make_float4(__builtin_amdgcn_fmed3f(v.x, c.lo, c.hi), __builtin_amdgcn_fmed3f(v.y, c.lo, c.hi), __builtin_amdgcn_fmed3f(v.z, c.lo, c.hi),
                     __builtin_amdgcn_fmed3f(v.w, c.lo, c.hi));
}
__device__ __forceinline__ float hswish1(float v) { return v * __builtin_amdgcn_fmed3f(v + 3.f, 0.f, 6.f) * 0.16666667163372040f; }
__device__ __forceinline__ float4 hswish4(float4 v) { return make_float4(hswish1(v.x), hswish1(v.y), hswish1(v.z), hswish1(v.w)); }
__device__ __forceinline__ float sigmoid1(float v) { return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(v * -1.44269504088896341f)); }
// gate prologue only (a handful of lanes, once per workgroup)
__device__ __forceinline__ float sg_act(float v, int act) {
  if (act == kActNone) return v;
  if (act == kActSigmoid) return sigmoid1(v);
  if (act == kActHswish) return hswish1(v);
  if (act == kActRelu) return fmaxf(v, 0.f);
  return __builtin_amdgcn_fmed3f(v, 0.f, 6.f);
}

// The weights are the A operand of every MFMA here (rows = output channels) and the activations the B operand (columns = pixels): the accumulator of lane
// (li, g) is then D[channels 4g..4g+3][pixel li] — four consecutive channels of ONE pixel, the 16-byte unit every store, bias and residual in these kernels
// works in — without the 4x4 transpose inside lane quads (12 selects + 4 DPP moves per tile) the pixel-major operand order needed.  Same products, same
// accumulation order over k: bit-identical values.
__device__ __forceinline__ float4 acc_quad(const f4acc acc) { return make_float4(acc[0], acc[1], acc[2], acc[3]); }
// one 16-pixel x 16-channel tile of a 1x1 convolution with Cin = 16: 4 MFMAs
__device__ __forceinline__ f4acc mma16(const float4 a, const float (&wr)[4]) {
  f4acc acc = {0.f, 0.f, 0.f, 0.f};
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[0], a.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[1], a.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[2], a.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[3], a.w, acc, 0, 0, 0);
  return acc;
}
// B-operand registers of the [16][cout_pad] block at output channels n0..n0+15: lane (li, g) holds w[4g + r][n0 + li]
__device__ __forceinline__ void load_wtile(float (&wr)[4], const float* __restrict__ w, const SegConvW& c, int n0, int li, int g) {
#pragma unroll
  for (int r = 0; r < 4; r++) wr[r] = (w + c.w_off)[(unsigned)((4 * g + r) * c.cout_pad + n0 + li)];
}

// ---- gate prologue: means from partial sums → FC → [FC] → s_gate[0..C) ---------------------------------------------------
// All 256 lanes call it.  GAP(a | b) (concatenated) or GAP(a) + GAP(b) (MLKit's GAP(skip + up)).  ONE cooperative memory round
// trip stages the partial sums and both FC weight blocks in LDS (`stage`, <= kGateStageFloats floats, may alias a tile region that
// is not live yet); everything after runs from LDS: a per-workgroup serial chain of dependent global loads here was most of the
// first version's run time.
// `publish` runs in front of the FIRST barrier, behind the requests of the prologue's own loads: LDS stores of the caller (k2's staged weights) that every later phase
// may read, without a barrier of their own and without a memory round trip in front of the prologue's.
constexpr int kGateStageFloats = kSegGateStageFloats;
struct NoPublish { __device__ __forceinline__ void operator()() const {} };
template <class Publish = NoPublish>
__device__ __forceinline__ void seg_gate(const SegGate& gt, const float* __restrict__ fa, const float* __restrict__ w, float* scr, float* stage, Publish publish = Publish()) {
  if (gt.timing_skip) { if (threadIdx.x < 16) scr[kScrGate + threadIdx.x] = 0.5f; publish(); __syncthreads(); return; }      // upper bound of what hoisting the gate out could buy
  const int tid = threadIdx.x;
#define BSX_GATE_SCR scr
#define BSX_GATE_STAGE stage
#define BSX_GATE_SRC(k) fa + gt.part[k].off
#define BSX_GATE_K k
#define BSX_GATE_FC_LANE true
#define BSX_GATE_FC_CAPTURE &
#define BSX_GATE_PART 1
#include "seg_gate.inc"
  for (int k = 0; k < gt.n_parts; k++)
#define BSX_GATE_PART 2
#include "seg_gate.inc"
#define BSX_GATE_PART 3
#include "seg_gate.inc"
  publish();
  __syncthreads();
#define BSX_GATE_PART 4
#include "seg_gate.inc"
}

// ---- per-tile partial sums of a 16-channel tensor → partials[tile][16] -------------------------------------------------------
// Lanes hold float4 partial sums of their channel quad.  MODE 0: MFMA-epilogue lanes (lane (g, li): channel quad g, the 16 lanes of
// the row differ in pixel); MODE 1: depthwise lanes (lane = 4 * pixel + quad inside a 16-lane DPP row).  DPP row shifts leave
// the partial float4s of a wave; they meet in s_red[16 slots][16 channels] and the first 16 lanes of the workgroup finish the sum.
template <int SHR>
__device__ __forceinline__ float dpp_row_shr(float v) {        // lane i <- lane i - SHR inside its row of 16 (0 where there is none)
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x110 + SHR, 0xf, 0xf, true));
}
template <int MODE>
__device__ __forceinline__ void wave_reduce16(float4 v, float* s_red, int wave, int lane) {
  if (MODE == 0) {                                                   // MFMA-epilogue lanes: row g of 16 lanes = 16 pixels of channel quad g
    v.x += dpp_row_shr<1>(v.x); v.y += dpp_row_shr<1>(v.y); v.z += dpp_row_shr<1>(v.z); v.w += dpp_row_shr<1>(v.w);
    v.x += dpp_row_shr<2>(v.x); v.y += dpp_row_shr<2>(v.y); v.z += dpp_row_shr<2>(v.z); v.w += dpp_row_shr<2>(v.w);
    v.x += dpp_row_shr<4>(v.x); v.y += dpp_row_shr<4>(v.y); v.z += dpp_row_shr<4>(v.z); v.w += dpp_row_shr<4>(v.w);
    v.x += dpp_row_shr<8>(v.x); v.y += dpp_row_shr<8>(v.y); v.z += dpp_row_shr<8>(v.z); v.w += dpp_row_shr<8>(v.w);
    const int li = lane & 15;                                        // lane 15 of the row holds its sum → slot 4 * wave; lanes 12..14 zero the wave's other three slots
    if (li >= 12) st4(s_red + (wave * 4 + (15 - li)) * 16 + 4 * (lane >> 4), li == 15 ? v : f4zero());
  } else {
    v.x += dpp_row_shr<4>(v.x); v.y += dpp_row_shr<4>(v.y); v.z += dpp_row_shr<4>(v.z); v.w += dpp_row_shr<4>(v.w);
    v.x += dpp_row_shr<8>(v.x); v.y += dpp_row_shr<8>(v.y); v.z += dpp_row_shr<8>(v.z); v.w += dpp_row_shr<8>(v.w);
    if ((lane & 12) == 12) st4(s_red + (wave * 4 + (lane >> 4)) * 16 + 4 * (lane & 3), v);     // slot (wave, row), channels 4 * quad
  }
}
// s += channel c of a tile's 16 slots, in slot order.  (A macro: as a function it moved the code of k3's per-frame form — tools/isa_same.py.)
#define BSX_SLOTS_SUM16(s, s_red, c) _Pragma("unroll") for (int j = 0; j < 16; j++) s += (s_red)[j * 16 + (c)]
__device__ __forceinline__ void store_partials(const float* s_red, float* dst /* 16 floats */) {   // after a barrier
  if (threadIdx.x < 16) {
    float s = 0.f;
    BSX_SLOTS_SUM16(s, s_red, threadIdx.x);
    dst[threadIdx.x] = s;
  }
}

// ---- bilinear up-sampling (RESIZE_BILINEAR) as per-axis tables: index pair + fraction, TFLite's clamping ----------------------
__device__ __forceinline__ void up_axis(int o, float scale, bool half_pixel, int in_size, int* lo, int* hi, float* frac) {
  const float v = half_pixel ? __fadd_rn(__fmul_rn((float)o + 0.5f, scale), -0.5f) : __fmul_rn((float)o, scale);
  const float fl = floorf(v);
  *lo = max((int)fl, 0);
  *hi = min((int)ceilf(v), in_size - 1);
  *frac = v - (float)*lo;
}
__device__ __forceinline__ float up_scale(int in, int out, bool align) { return (align && out > 1) ? (float)(in - 1) / (float)(out - 1) : (float)in / (float)out; }

// sum over the four lanes of a quad of p[quad]: a 4x4 "reduce-scatter" in 3 DPP exchanges (cf. quad_transpose)
__device__ __forceinline__ float quad_reduce_scatter(float p0, float p1, float p2, float p3, int quad) {
  const bool b0 = quad & 1, b1 = quad & 2;
  const float klo = (b0 ? p1 : p0) + dpp_quad(b0 ? p0 : p1, 1);     // positions {b0, 2 + b0} stay on this lane
  const float khi = (b0 ? p3 : p2) + dpp_quad(b0 ? p2 : p3, 1);
  return (b1 ? khi : klo) + dpp_quad(b1 ? klo : khi, 2);
}

// depthwise 3x3 (stride S) at pixel (py, px) of a [rows][RW][16] LDS tile, channel quad `q`; packed FMAs (v_pk_fma_f32)
typedef float f4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f4v ldv(const float* p) { return *reinterpret_cast<const f4v*>(p); }
__device__ __forceinline__ f4v tov(float4 a) { f4v r = {a.x, a.y, a.z, a.w}; return r; }
__device__ __forceinline__ float4 tof4(f4v a) { return make_float4(a.x, a.y, a.z, a.w); }
// `co[fx]` = float offset of the lane's quad at column S * px + fx of a tile row (col_a / col_b: the layout's swizzle is folded into the three per-lane constants),
// `row0` = the tile row of tap fy = 0, RWF = floats per tile row
__device__ __forceinline__ f4v dw3x3(const float* __restrict__ zt, int RWF, int row0, const int (&co)[3], const f4v (&wd)[9]) {
  f4v acc = {0.f, 0.f, 0.f, 0.f};
  const float* base = zt + row0 * RWF;
#pragma unroll
  for (int fy = 0; fy < 3; fy++)
#pragma unroll
    for (int fx = 0; fx < 3; fx++) acc = __builtin_elementwise_fma(ldv(base + fy * RWF + co[fx]), wd[fy * 3 + fx], acc);
  return acc;
}

// decode of one model-resolution pixel (lib/libbackscrub.cc:333-357) — same arithmetic as decode_k / decode_meet4_k (kernels_img.hip)
__device__ __forceinline__ uint32_t seg_meet_val(float l0, float l1) {
  const float d = l1 - l0;
  if (fabsf(l0) <= 80.f && fabsf(l1) <= 80.f && fabsf(d) >= 1e-4f) return d > 0.f ? 0u : 255u;
  const float e0 = (float)exp((double)l0), e1 = (float)exp((double)l1);
  const float s = __fadd_rn(e0, e1);
  return __fdiv_rn(e0, s) < __fdiv_rn(e1, s) ? 0u : 255u;
}

__device__ __forceinline__ int wave_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// MFMA phases walk ROW-ALIGNED tiles: tile t = (row t / ctiles, 16 columns 16 * (t % ctiles) ..) of a [rows][RW = 16 * ctiles][16]
// LDS tile.  The row is wave-uniform (scalar index math, scalar in-image tests), the column of a lane is 16 * ct + its fixed lane
// offset: no per-pixel divisions, which were most of the VALU work of the first (linear-index) version of these kernels.
struct RowTile { int row, ct; };
__device__ __forceinline__ RowTile row_tile(int t, int ctiles, unsigned m_ct) {
  RowTile r;
  r.row = (int)(((unsigned)t * m_ct) >> 16);           // t / ctiles for t < 4096 (m_ct = ceil(65536 / ctiles))
  r.ct = t - r.row * ctiles;
  return r;
}

// ==================================================================================================================================
// head: stem conv3x3/s2 (3 → 16) → 1x1 (16 → 16) → depthwise 3x3/s2; writes A (skip of the last decoder level), b0, and the
// pooled partial sums of both.  Tile = TR (<= 4) x TC (<= 15) pixels of b0.
// ==================================================================================================================================
// U8IN: the network input arrives as the filtered 8-bit pixels (R | G<<8 | B<<16 per pixel, prep_fused_k<2>) and is normalised here with the
// same two roundings convertTo applies (libbackscrub.cc:302): fadd(fmul(float(q), scale), offset) — bit-identical to reading the f32 tensor.
#ifdef BSX_SEG_RTC
extern "C" __global__ __launch_bounds__(kSegThreads) void bsx_seg_head(
#else
template <bool STEM_HSWISH, bool H16, bool U8IN>
__global__ __launch_bounds__(kSegThreads) void seg_head_k(
#endif
    const SegHead d_rt, float* __restrict__ arena, long per_frame, const float* __restrict__ net_in,
                                                          const float* __restrict__ w, float in_scale, float in_offset, int n_frames) {
  BSX_SEG_D(SegHead, HEAD);
  unsigned f_, t_;
  xcd_frame_tile((unsigned)(d.tiles_y * d.tiles_x), (unsigned)n_frames, &f_, &t_);
  const int f = (int)f_, ty = (int)t_ / d.tiles_x, tx = (int)t_ - ty * d.tiles_x;
  const int r0 = ty * d.TR, c0 = tx * d.TC;
  const int AR = 2 * d.TR + 1, AC = 2 * d.TC + 1, ar0 = 2 * r0 - d.dw_pt, ac0 = 2 * c0 - d.dw_pl, RW = d.rw, ctiles = RW >> 4;
  const int IR = 2 * AR + 1, IC = 2 * AC + 1, ir0 = 2 * ar0 - d.stem_pt, ic0 = 2 * ac0 - d.stem_pl, rowf = IC * 3;
  float* fa = arena + (size_t)f * (size_t)per_frame;
  float* in_t = seg_smem;                                           // [IR][IC * 3]; no scratch block in front: the head has no gate prologue, and its partial-sum meeting
                                                                    // points (s_red, 512 floats) reuse this window once the stem is done with it — 2.5 KB that put the 4 x 14 tile's
                                                                    // workgroup exactly ON the 32 KB line (5 per CU only if the allocator wastes nothing)
  float* a_t = in_t + max(512, (IR * rowf + 3) & ~3);                      // x = act(pw(stem)) [AR][AC][16]: rows of AC pixels, not of RW = 16 ceil(AC / 16) — the MFMA tiles
                                                                    // round the COMPUTE up to 16 pixels, the storage need not (5 workgroups per CU instead of 4 at a 4 x 13 tile)
  float* A_out = fa + d.a_off;                                      // uniform bases + 32-bit lane offsets (global_load/store saddr forms)
  float* b0_out = fa + d.b0_off;
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6), li = lane & 15, g = lane >> 4, cq4 = 4 * g;

  // 1. input tile (zero outside the image: SAME padding of the stem): wave = rows, lane = row elements; every load of the lane is
  //    in flight before its first LDS store
  if (d.dbg_skip & 8) { /* timing: no input tile */ } else
  if (U8IN) {                                                       // lane = pixel of the row (IC <= 63): one dword = three input values
    // (addresses clamped into the image and the load unconditional: under `if (inside)` every row became an exec-masked region with its own s_waitcnt vmcnt(0) and
    //  a dozen register copies to merge the paths — five serialised memory round trips where this has five loads in flight; outside pixels are zeroed below.
    //  Measured: seg_head 55.5 -> 51.5 us lite, 249 -> 226 mlkit / HD.  The same rewrite of the k2 / k3 / tail prefetches, whose loads were already in flight,
    //  measured 1-3 % slower — more loads issued — and was not kept: profiles/r03aj)
    const uint32_t* src = reinterpret_cast<const uint32_t*>(net_in) + (size_t)f * (size_t)(d.H0 * d.W0);
    const bool colok = lane < IC && ic0 + lane >= 0 && ic0 + lane < d.W0;
    const int gxc = min(max(ic0 + lane, 0), d.W0 - 1);
    uint32_t v[5];
    bool ok[5];
#pragma unroll
    for (int j = 0; j < 5; j++) {
      const int row = wave + 4 * j, gy = ir0 + row;
      ok[j] = row < IR && gy >= 0 && gy < d.H0 && colok;
      v[j] = src[(unsigned)(min(max(gy, 0), d.H0 - 1) * d.W0 + gxc)];
    }
#pragma unroll
    for (int j = 0; j < 5; j++) {
      const int row = wave + 4 * j;
      if (row < IR && lane < IC) {
        float* o = in_t + row * rowf + 3 * lane;
        o[0] = ok[j] ? __fadd_rn(__fmul_rn((float)(v[j] & 255u), in_scale), in_offset) : 0.f;
        o[1] = ok[j] ? __fadd_rn(__fmul_rn((float)((v[j] >> 8) & 255u), in_scale), in_offset) : 0.f;
        o[2] = ok[j] ? __fadd_rn(__fmul_rn((float)((v[j] >> 16) & 255u), in_scale), in_offset) : 0.f;
      }
    }
  } else {
    const float* src = net_in + (size_t)f * (size_t)(d.H0 * d.W0 * 3);
    const int lo_rem = max(0, -ic0) * 3, hi_rem = min(IC, d.W0 - ic0) * 3;
    float v[5][3];
#pragma unroll
    for (int j = 0; j < 5; j++) {
      const int row = wave + 4 * j, gy = ir0 + row;
      const bool rowok = row < IR && gy >= 0 && gy < d.H0;
#pragma unroll
      for (int e3 = 0; e3 < 3; e3++) {
        const int e = lane + 64 * e3;
        v[j][e3] = 0.f;
        if (rowok && e >= lo_rem && e < hi_rem) v[j][e3] = src[(unsigned)((gy * d.W0 + ic0) * 3 + e)];
      }
    }
#pragma unroll
    for (int j = 0; j < 5; j++) {
      const int row = wave + 4 * j;
#pragma unroll
      for (int e3 = 0; e3 < 3; e3++) { const int e = lane + 64 * e3; if (row < IR && e < rowf) in_t[row * rowf + e] = v[j][e3]; }
    }
  }
  // stem operand tables of this lane: k = 4s + g over the im2col axis (fy, fx, ci), 27 valid entries
  int koff[7];
  float ws[7];
#pragma unroll
  for (int s = 0; s < 7; s++) {
    const int k = 4 * s + g;
    const bool valid = k < 27;
    const int fy = k / 9, r9 = k - 9 * fy, fx = r9 / 3, ci = r9 - 3 * fx;
    koff[s] = valid ? fy * rowf + fx * 3 + ci : 0;
    ws[s] = valid ? (w + d.stem.w_off)[(unsigned)(k * d.stem.cout_pad + li)] : 0.f;
  }
  const float4 bias_s = ld4(w + d.stem.b_off + cq4);
  const Clamp cl_stem = clamp_of(d.stem.act), cl_pw = clamp_of(d.pw.act), cl_dw = clamp_of(d.dw.act);
  const int ntile = AR * ctiles;
  const int xe = li;                                        // column of the pixel this lane owns after the quad transpose
  __syncthreads();

  // 2 + 3. stem on the A region and x = act(pw(A)) on the same pixels, two tiles per iteration (their MFMA chains interleave).  With the weights as the MFMA's A
  //    operand the stem's accumulator lane (li, g) holds channels 4 g .. 4 g + 3 of pixel li — EXACTLY the B operand the 1x1's four MFMAs want from that lane: the
  //    activated stem output goes from the accumulator registers straight into them (round 4).  Until then it made a round trip through an LDS tile of its own
  //    ([AR][RW][16]: 18 KB written, a barrier, 18 KB read) and the 1x1 was a second loop over the tiles; the same values enter the same instructions, so the results
  //    are the same bits.  x lands where that tile was (a_t's region: in_t is still being read by the other waves' stem tiles); zero outside the image = SAME padding
  //    of the depthwise.
  float* x_f = a_t;                                                 // DENSE [AR][AC][16] rows: the de-interleaved, swizzled form (col_b) removes this tile's bank conflicts as it does in
                                                                    // k2 — and measured 4-5 % SLOWER here on all three networks (profiles/r05b: 44.4 -> 46.5 us lite, 389 -> 409 us segm_full / HD):
                                                                    // the head is bound by VALU issue, and the odd row width AC makes the swizzled address arithmetic per tile, not per lane
  float wr[4];
  load_wtile(wr, w, d.pw, 0, li, g);
  const float4 bias_p = ld4(w + d.pw.b_off + cq4);
  float4 sumA = f4zero();
  auto stem_pw_epilogue = [&](const f4acc acc, const RowTile rt) {
    float4 v = acc_quad(acc);
    const int x2 = 16 * rt.ct + xe, gy = ar0 + rt.row, gx = ac0 + x2;
    v = f4add(v, bias_s);
    v = as_stored<H16>(STEM_HSWISH ? hswish4(v) : clamp4(v, cl_stem));
    // (lanes past the tile's last column hold the stem of column AC - 1, as the clamped read of the two-loop form did; their results are dropped below)
    f4acc pa = {0.f, 0.f, 0.f, 0.f};
    if (!(d.dbg_skip & 2)) {
      pa = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[0], v.x, pa, 0, 0, 0);
      pa = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[1], v.y, pa, 0, 0, 0);
      pa = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[2], v.z, pa, 0, 0, 0);
      pa = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[3], v.w, pa, 0, 0, 0);
    }
    if (x2 < AC) {
      const bool row_owned = gy >= max(2 * r0, 0) && gy < min(2 * r0 + 2 * d.TR, d.H1);          // scalar
      if (row_owned && gx >= 2 * c0 && gx < min(2 * c0 + 2 * d.TC, d.W1)) {                      // each A pixel is stored by exactly one tile
        stg4<H16>(A_out, (unsigned)((gy * d.W1 + gx) * 16 + cq4), v);
        sumA = f4add(sumA, v);
      }
      float4 xv = acc_quad(pa);
      const bool inside = gy >= 0 && gy < d.H1 && gx >= 0 && gx < d.W1;
      xv = inside ? clamp4(f4add(xv, bias_p), cl_pw) : f4zero();
      st4(x_f + (rt.row * AC + x2) * 16 + cq4, xv);
    }
  };
  for (int t = wave; t < ntile && !(d.dbg_skip & 1); t += 8) {
    const bool two = t + 4 < ntile;                                  // scalar
    const RowTile r0t = row_tile(t, ctiles, d.m_ct), r1t = row_tile(two ? t + 4 : t, ctiles, d.m_ct);
    const float* base0 = in_t + (2 * r0t.row) * rowf + 6 * min(16 * r0t.ct + li, AC - 1);
    const float* base1 = in_t + (2 * r1t.row) * rowf + 6 * min(16 * r1t.ct + li, AC - 1);
    float av0[7], av1[7];
#pragma unroll
    for (int s7 = 0; s7 < 7; s7++) { av0[s7] = base0[koff[s7]]; av1[s7] = base1[koff[s7]]; }
    f4acc acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s7 = 0; s7 < 7; s7++) {
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ws[s7], av0[s7], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ws[s7], av1[s7], acc1, 0, 0, 0);
    }
    stem_pw_epilogue(acc0, r0t);
    if (two) stem_pw_epilogue(acc1, r1t);
  }
  const int quad = lane & 3, px = lane >> 2;                        // depthwise lanes: (pixel of the row, channel quad)
  f4v wd[9];
#pragma unroll
  for (int k = 0; k < 9; k++) wd[k] = ldv(w + d.dw.w_off + k * 16 + 4 * quad);
  const f4v bias_d = ldv(w + d.dw.b_off + 4 * quad);
  const int cox[3] = {(2 * px) * 16 + 4 * quad, (2 * px + 1) * 16 + 4 * quad, (2 * px + 2) * 16 + 4 * quad};
  __syncthreads();

  // 4. depthwise 3x3 / stride 2 → b0: one tile row per wave iteration
  float4 sumB = f4zero();
  for (int py = wave; py < d.TR && !(d.dbg_skip & 4); py += 4) {
    if (r0 + py >= d.H2) break;
    if (px < d.TC && c0 + px < d.W2) {
      const float4 v = as_stored<H16>(clamp4(tof4(dw3x3(x_f, AC * 16, 2 * py, cox, wd) + bias_d), cl_dw));
      stg4<H16>(b0_out, (unsigned)(((r0 + py) * d.W2 + c0 + px) * 16 + 4 * quad), v);
      sumB = f4add(sumB, v);
    }
  }
  float* s_red = in_t;                                              // (every wave is past the stem — the barrier in front of the depthwise — so the window is free)
  wave_reduce16<0>(sumA, s_red, wave, lane);
  wave_reduce16<1>(sumB, s_red + 256, wave, lane);
  __syncthreads();
  store_partials(s_red, fa + d.part_a_off + (long)t_ * 16);
  store_partials(s_red + 256, fa + d.part_b0_off + (long)t_ * 16);
}

// ==================================================================================================================================
// k2: s = gate(GAP(b0)); B = pw_a(b0 * s) (skip of decoder level 2); x = act(pw_b(B)); c0 = act(dw3x3/s2(x)).  Tile = TR x TC of c0.
// The expanded tensor x (72 channels) exists only 16 channels at a time, in LDS.
// ==================================================================================================================================
#ifdef BSX_SEG_RTC
extern "C" __global__ __launch_bounds__(kSegThreads) __attribute__((amdgpu_waves_per_eu(kSegK2Waves, kSegK2Waves))) void bsx_seg_k2(
#else
template <bool H16>
__global__ __launch_bounds__(kSegThreads) __attribute__((amdgpu_waves_per_eu(kSegK2Waves, kSegK2Waves))) void seg_k2_k(
#endif
    const SegK2 d_rt, float* __restrict__ arena, long per_frame, const float* __restrict__ w, int n_frames) {
  BSX_SEG_D(SegK2, K2);
  unsigned f_, t_;
  xcd_frame_tile((unsigned)(d.tiles_y * d.tiles_x), (unsigned)n_frames, &f_, &t_);
  const int f = (int)f_, ty = (int)t_ / d.tiles_x, tx = (int)t_ - ty * d.tiles_x;
  const int r0 = ty * d.TR, c0 = tx * d.TC;
  const int BR = 2 * d.TR + 1, BC = 2 * d.TC + 1, br0 = 2 * r0 - d.dw_pt, bc0 = 2 * c0 - d.dw_pl, RW = d.rw, ctiles = RW >> 4;
  float* fa = arena + (size_t)f * (size_t)per_frame;
  float* B_t = seg_smem + kScrFloats;                               // [BR][RW][16]
  float* x_t = B_t + BR * RW * 16;
#ifdef BSX_SEG_RTC
  // the staged weights lie behind both tiles and behind the gate's staging area, and end where the launch's dynamic LDS (lds_floats) ends
  static_assert(d.wst.form == 0 || (d.wst.off >= kScrFloats + 2 * BR * RW * 16 && d.wst.off >= kScrFloats + kGateStageFloats && d.wst.off + d.wst.floats == d.lds_floats),
                "k2: staged weights outside the planned LDS");
#endif
  const float* b0_in = fa + d.b0_off;
  float* B_out = fa + d.B_off;
  float* c0_out = fa + d.c0_off;
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6), li = lane & 15, g = lane >> 4, cq4 = 4 * g;
  const int ntile = BR * ctiles, xe = li;
  const int la = col_a(li, g), lb = col_b(li, g, RW >> 1);          // this lane's quad at column 16 ct + li of a B_t / x_t row = (16 | 8) ct columns further + these (the swizzles have period <= 16)
  // all of this wave's b0 operands are requested before the gate prologue (one memory round trip for the whole workgroup)
  constexpr int kB0 = 6;                                            // planner: ceil(BR * ctiles / 4) <= 6
  float4 b0v[kB0];
#pragma unroll
  for (int j = 0; j < kB0; j++) {
    const int t = wave + 4 * j;
    b0v[j] = f4zero();
    if (t < ntile) {
      const RowTile rt = row_tile(t, ctiles, d.m_ct);
      const int gy = br0 + rt.row, gx = bc0 + 16 * rt.ct + li;
      if (gy >= 0 && gy < d.H2 && gx >= 0 && gx < d.W2) b0v[j] = ldg4<H16>(b0_in, (unsigned)((gy * d.W2 + gx) * 16 + 4 * g));
    }
  }
  // ... and with them the weights the later phases need (SegStage, plan.cpp).  form >= 1: pw_a's tile + bias wait in registers across the gate, where the kernel is far
  // below its register step, and pw_b's tile + bias of channel group 0 go to LDS; form 2: the depthwise weights + biases of all groups too — 16-byte pieces through
  // registers, stored in front of the gate's first barrier.  The expand loop below then never waits for HBM / L2 in front of a use: it was one dependent round trip per
  // channel group for the 1x1 tile (1-2 us each at this occupancy), one for the depthwise weights behind it, and one for pw_a behind the gate.  Same floats into the
  // same instructions: bit-identical to form 0.
  // (The graph-specialised build only: the ahead-of-time instance — descriptor as a kernel argument, what runs where hipRTC is unavailable — sits at 78 of its 80
  // registers and spills 20-44 bytes with any staged form, whose LDS addresses it cannot fold into instruction offsets; it reads its weights from global memory
  // whatever the plan's form and leaves the block unused.)
#ifdef BSX_SEG_RTC
  constexpr SegStage st = d.wst;
#else
  const SegStage st{};
#endif
  float* sw = seg_smem + st.off;
  // one group's pw_b tile + bias as 68 pieces: lanes 0..63 = (row tid & 15, columns 4 * (tid >> 4) ..), lanes 64..67 the bias
  auto pwb_fetch = [&](int grp) {
    float4 v = f4zero();
    if (tid < 64) v = ld4(w + d.pw_b.w_off + (unsigned)((tid & 15) * d.pw_b.cout_pad + 16 * grp + 4 * (tid >> 4)));
    else if (tid < 68) v = ld4(w + d.pw_b.b_off + 16 * grp + 4 * (tid - 64));
    return v;
  };
  auto pwb_store = [&](int buf, float4 v) {
    float* dst = sw + buf * st.buf_floats;
    if (tid < 64) st4(dst + (tid & 15) * st.stride + 4 * (tid >> 4), v);
    else if (tid < 68) st4(dst + st.bias_off + 4 * (tid - 64), v);
  };
  float wr[4];
  float4 bias_a, sf[3];
  if (st.form >= 1) {
    load_wtile(wr, w, d.pw_a, 0, li, g);
    bias_a = ld4(w + d.pw_a.b_off + cq4);
    sf[0] = pwb_fetch(0);
    if (st.form >= 2) {
      if (4 * tid < 9 * d.dw.C) sf[1] = ld4(w + d.dw.w_off + 4 * tid);
      if (4 * tid < d.dw.C) sf[2] = ld4(w + d.dw.b_off + 4 * tid);
    }
  }
  seg_gate(d.gate, fa, w, seg_smem, B_t, [&] {
    if (st.form >= 1) {
      pwb_store(0, sf[0]);
      if (st.form >= 2) {
        if (4 * tid < 9 * d.dw.C) st4(sw + st.dw_off + 4 * tid, sf[1]);
        if (4 * tid < d.dw.C) st4(sw + st.dwb_off + 4 * tid, sf[2]);
      }
    }
  });
  const float4 sv = ld4(seg_smem + kScrGate + 4 * g);
  if (st.form == 0) {
    load_wtile(wr, w, d.pw_a, 0, li, g);
    bias_a = ld4(w + d.pw_a.b_off + cq4);
  }
  const Clamp cl_a = clamp_of(d.pw_a.act), cl_b = clamp_of(d.pw_b.act), cl_dw = clamp_of(d.dw.act);

  // 1. B on the region the depthwise needs
  float4 sumB = f4zero();
#pragma unroll
  for (int j = 0; j < kB0; j++) {
    const int t = wave + 4 * j;
    if (t >= ntile) break;
    const RowTile rt = row_tile(t, ctiles, d.m_ct);
    float4 a = b0v[j];
    a = make_float4(__fmul_rn(a.x, sv.x), __fmul_rn(a.y, sv.y), __fmul_rn(a.z, sv.z), __fmul_rn(a.w, sv.w));
    const f4acc acc = mma16(a, wr);
    float4 v = acc_quad(acc);
    const int x2 = 16 * rt.ct + xe, hy = br0 + rt.row, hx = bc0 + x2;
    if (x2 < BC) {
      v = as_stored<H16>(clamp4(f4add(v, bias_a), cl_a));
      st4(B_t + (rt.row * RW + 16 * rt.ct) * 16 + la, v);
      const bool row_owned = hy >= max(2 * r0, 0) && hy < min(2 * r0 + 2 * d.TR, d.H2);
      if (row_owned && hx >= 2 * c0 && hx < min(2 * c0 + 2 * d.TC, d.W2)) {
        stg4<H16>(B_out, (unsigned)((hy * d.W2 + hx) * 16 + cq4), v);
        sumB = f4add(sumB, v);
      }
    }
  }
  float* s_red = seg_smem + kScrRed;
  wave_reduce16<0>(sumB, s_red, wave, lane);
  __syncthreads();
  store_partials(s_red, fa + d.part_B_off + (long)t_ * 16);

  // 2. 16 expanded channels at a time: x = act(pw_b(B)) → depthwise 3x3/s2 → c0
  //    (requesting group g + 1's 1x1 tile while group g runs — 8 more registers, 5 instead of 6 waves per SIMD or 16 B of scratch at a cap of 6 — measured SLOWER:
  //     45.4 → 51.3 us at 256 VGA streams, 170 → 187 us for mlkit / HD, profiles/r03af)
  const int C = d.dw.C, ngrp = (C + 15) >> 4, quad = lane & 3, px = lane >> 2;
  const int cox[3] = {col_b(2 * px, quad, RW >> 1), col_b(2 * px + 1, quad, RW >> 1), col_b(2 * px + 2, quad, RW >> 1)};   // x_t: de-interleaved columns (swz_b)
  for (int grp = 0; grp < ngrp && !(d.dbg_skip & 2); grp++) {
    float4 bias_b, nxt;
    if (st.form >= 1) {                                             // staged rows: stride = 4 (mod 8), conflict-free (tests/test_k2_staging.py)
      const float* tb = sw + (grp & 1) * st.buf_floats;
#pragma unroll
      for (int r = 0; r < 4; r++) wr[r] = tb[(4 * g + r) * st.stride + li];
      bias_b = ld4(tb + st.bias_off + cq4);
      if (grp + 1 < ngrp) nxt = pwb_fetch(grp + 1);                 // lands during this group's work; stored in front of the group's last barrier
    } else {
      load_wtile(wr, w, d.pw_b, 16 * grp, li, g);
      bias_b = ld4(w + d.pw_b.b_off + 16 * grp + cq4);
    }
    for (int t = wave; t < ntile; t += 4) {
      const RowTile rt = row_tile(t, ctiles, d.m_ct);
      // (columns >= BC of the row hold nothing: their lanes feed MFMA columns whose results are dropped below — a column of D depends on the same column of B only)
      const f4acc acc = mma16(ld4(B_t + (rt.row * RW + 16 * rt.ct) * 16 + la), wr);
      float4 v = acc_quad(acc);
      const int x2 = 16 * rt.ct + xe, hy = br0 + rt.row, hx = bc0 + x2;
      if (x2 < BC) {
        const bool inside = hy >= 0 && hy < d.H2 && hx >= 0 && hx < d.W2;
        v = inside ? clamp4(f4add(v, bias_b), cl_b) : f4zero();
        st4(x_t + (rt.row * RW + 8 * rt.ct) * 16 + lb, v);
      }
    }
    const int ch = 16 * grp + 4 * quad;
    f4v wd[9];
    f4v bias_d = {0.f, 0.f, 0.f, 0.f};
    if (ch < C && st.form < 2) {
#pragma unroll
      for (int k = 0; k < 9; k++) wd[k] = ldv(w + d.dw.w_off + (unsigned)(k * C + ch));
      bias_d = ldv(w + d.dw.b_off + ch);
    } else if (ch < C) {
#pragma unroll
      for (int k = 0; k < 9; k++) wd[k] = ldv(sw + st.dw_off + k * C + ch);
      bias_d = ldv(sw + st.dwb_off + ch);
    }
    __syncthreads();
    if (ch < C && px < d.TC && c0 + px < d.W3)
      for (int py = wave; py < d.TR && r0 + py < d.H3; py += 4) {
        const float4 v = clamp4(tof4(dw3x3(x_t, RW * 16, 2 * py, cox, wd) + bias_d), cl_dw);
        stg4<H16>(c0_out, (unsigned)(((r0 + py) * d.W3 + c0 + px) * C + ch), v);
      }
    if (st.form >= 1 && grp + 1 < ngrp) pwb_store((grp + 1) & 1, nxt);        // (that buffer was last read a group ago: two barriers back)
    __syncthreads();
  }
}

// z = act(pw(skip * g + up(lo))) on the (TR+2) x (TC+2 <= 16) halo region of a tile, zero outside the image — shared by k3 and the
// tail.  One MFMA tile = one region row (16 columns): the row's interpolation pair is scalar, the column's a per-lane constant;
// up = a*w00 + b*w10 + c*w01 + d*w11 with w = products of the two axis fractions (differs from the reference association
// ((a*(1-dy))*(1-dx) + ...) by float rounding only).
// Memory: at 3-4 workgroups per CU a dependent global load costs 1-2 us, so EVERYTHING the phase reads is requested in the first
// instructions of the kernel (gated_prefetch): the lane's skip operand of each of its <= kGatedRows rows into registers, the
// low-resolution rows/columns the tile interpolates from into LDS (l_t, [LR][LC][20]); the compute part then never touches HBM.
constexpr int kGatedRows = 5;           // region rows per wave: (TR + 2 + 3) / 4 <= 5  →  TR <= 18
constexpr int kLoStride = kSegLoStride; // floats per staged low-resolution pixel (16: dense, swizzled by swz_l)
struct GatedPre { float4 s[kGatedRows]; int ly0, lx0, LC; };
template <bool H16>
__device__ __forceinline__ GatedPre gated_prefetch(const float* __restrict__ skip, const float* __restrict__ lo, int H, int W, int HL, int WL, bool half_pixel,
                                                   float hs, float wsc, int r0, int c0, int ZH, int ZC, float* l_t) {
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6), li = lane & 15, g = lane >> 4;
  GatedPre pre;
  const int ix = c0 - 1 + li;
  const bool col_in = li < ZC && ix >= 0 && ix < W;
#pragma unroll
  for (int j = 0; j < kGatedRows; j++) {
    const int zy = wave + 4 * j, iy = r0 - 1 + zy;
    pre.s[j] = f4zero();
    if (zy < ZH && iy >= 0 && iy < H && col_in) pre.s[j] = ldg4<H16>(skip, (unsigned)((iy * W + ix) * 16 + 4 * g));
  }
  // low-resolution window: rows y0(first image row of the region) .. y1(last), columns likewise (monotone maps).  hs / wsc: the two up-sampling scales — launch constants the
  // planner computes (SegK3 / SegTail::hs, ::ws: the same IEEE single-precision quotients); computed here they were four correctly-rounded divisions (both `align` forms of
  // each axis) of ~11 instructions in front of the prefetch's first address, and four more in gated_compute
  int ly0, ly1, lx0, lx1, t0, t1;
  float fr;
  up_axis(max(r0 - 1, 0), hs, half_pixel, HL, &ly0, &t1, &fr);
  up_axis(min(r0 - 2 + ZH, H - 1), hs, half_pixel, HL, &t0, &ly1, &fr);
  up_axis(max(c0 - 1, 0), wsc, half_pixel, WL, &lx0, &t1, &fr);
  up_axis(min(c0 - 2 + ZC, W - 1), wsc, half_pixel, WL, &t0, &lx1, &fr);
  const int LR = ly1 - ly0 + 1, LC = lx1 - lx0 + 1;                 // planner: LR <= 12, LC * 4 <= 64
  pre.ly0 = ly0; pre.lx0 = lx0; pre.LC = LC;
  float4 v[3];
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const int ly = wave + 4 * j;
    v[j] = f4zero();
    if (ly < LR && lane < LC * 4) v[j] = ldg4<H16>(lo, (unsigned)(((ly0 + ly) * WL + lx0 + (lane >> 2)) * 16 + 4 * (lane & 3)));
  }
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const int ly = wave + 4 * j;
    if (ly < LR && lane < LC * 4) st4(l_t + ly * LC * kLoStride + col_l(lane >> 2, lane & 3), v[j]);
  }
  return pre;
}
__device__ __forceinline__ void gated_compute(const GatedPre& pre, const float* l_t, int H, int W, int HL, int WL, bool half_pixel, float hs, float wsc, const float* s_gate,
                                              const SegConvW& pw, const float* __restrict__ w, int r0, int c0, int ZH, int ZC, float* z_t) {
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6), li = lane & 15, g = lane >> 4, cq4 = 4 * g;
  float wr[4];
  load_wtile(wr, w, pw, 0, li, g);
  const float4 bias = ld4(w + pw.b_off + cq4);
  const float4 gv = ld4(s_gate + 4 * g);
  const Clamp cl = clamp_of(pw.act);
  // column constants of this lane: operand and epilogue side are the same pixel li
  const int ix = c0 - 1 + li;
  int x0, x1;
  float dx;
  up_axis(min(max(ix, 0), W - 1), wsc, half_pixel, WL, &x0, &x1, &dx);
  const int xo0 = col_l(x0 - pre.lx0, g), xo1 = col_l(x1 - pre.lx0, g);
  const int xe = li;
  const bool ecol_in = xe < ZC && ix >= 0 && ix < W;
#pragma unroll
  for (int j = 0; j < kGatedRows; j++) {
    const int zy = wave + 4 * j, iy = r0 - 1 + zy;
    if (zy >= ZH) break;
#define BSX_GR_LO_ROW(y) (l_t + ((y) - pre.ly0) * pre.LC * kLoStride)
#define BSX_GR_SKIP pre.s[j]
#define BSX_GR_STORE(v) if (xe < ZC) st4(z_t + zy * 256 + col_a(xe, g), v)
#include "seg_gated_row.inc"
  }
}

// ==================================================================================================================================
// k3 (decoder level 2): z = act(pw1(B * g + up(lo2))); t = z + act(dw3x3(z)); lo = pw2(t).  Tile = TR x TC (<= 14) at the B resolution.
// ==================================================================================================================================
#ifdef BSX_SEG_RTC
extern "C" __global__ __launch_bounds__(kSegThreads) void bsx_seg_k3(
#else
template <bool H16>
__global__ __launch_bounds__(kSegThreads) void seg_k3_k(
#endif
    const SegK3 d_rt, float* __restrict__ arena, long per_frame, const float* __restrict__ w, int n_frames) {
  BSX_SEG_D(SegK3, K3);
  unsigned f_, t_;
  xcd_frame_tile((unsigned)(d.tiles_y * d.tiles_x), (unsigned)n_frames, &f_, &t_);
  const int f = (int)f_, ty = (int)t_ / d.tiles_x, tx = (int)t_ - ty * d.tiles_x;
  const int r0 = ty * d.TR, c0 = tx * d.TC, ZH = d.TR + 2, ZC = d.TC + 2;
  float* fa = arena + (size_t)f * (size_t)per_frame;
  float* z_t = seg_smem + kScrFloats;                               // [ZH][16][16]
  float* l_t = z_t + ZH * 256;                                      // staged window of lo2
  float* lo_out = fa + d.lo_off;
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6), li = lane & 15, g = lane >> 4, cq4 = 4 * g;
  const GatedPre pre = gated_prefetch<H16>(fa + d.skip_off, fa + d.lo2_off, d.H2, d.W2, d.HL, d.WL, d.half_pixel != 0, d.hs, d.ws, r0, c0, ZH, ZC, l_t);
  if (tid < 16) seg_smem[kScrGate + tid] = fa[d.g_off + tid];
  __syncthreads();
  gated_compute(pre, l_t, d.H2, d.W2, d.HL, d.WL, d.half_pixel != 0, d.hs, d.ws, seg_smem + kScrGate, d.pw1, w, r0, c0, ZH, ZC, z_t);
  // The depthwise runs on the MFMA's own lanes — lane (li, g) = (pixel of the row, channel quad) — so t = z + act(dw(z)) of the lane IS the B operand of pw2's four
  // MFMAs (round 5).  Until then the depthwise used (pixel = lane >> 2, quad = lane & 3) lanes and t made a round trip through an LDS tile of its own ([TR][16][16]:
  // 12 KB, a barrier): k3 34.8 -> 22.8 KiB per workgroup at a 12 x 14 tile.  Same values into the same instructions: bit-identical.  Under swz_a the (li, g) lanes read
  // z_t without bank conflicts, exactly like an MFMA operand read.  Lanes 14, 15 (TC <= 14) repeat lane 13's columns; their results are dropped.
  const int pc = min(li, 13);
  const int coz[3] = {col_a(pc, g), col_a(pc + 1, g), col_a(pc + 2, g)};
  f4v wd[9];
#pragma unroll
  for (int k = 0; k < 9; k++) wd[k] = ldv(w + d.dw.w_off + k * 16 + cq4);
  const f4v bias_d = ldv(w + d.dw.b_off + cq4);
  const Clamp cl_dw = clamp_of(d.dw.act), cl_2 = clamp_of(d.pw2.act);
  float wr[4];
  load_wtile(wr, w, d.pw2, 0, li, g);
  const float4 bias2 = ld4(w + d.pw2.b_off + cq4);
  __syncthreads();
  float4 sum = f4zero();
#define BSX_K3R_FIRST wave
#define BSX_K3R_Z z_t
#define BSX_K3R_ZRW 256
#define BSX_K3R_ZROW(py) (py)
#include "seg_k3_rows.inc"
  float* s_red = seg_smem + kScrRed;
  wave_reduce16<0>(sum, s_red, wave, lane);
  __syncthreads();
  store_partials(s_red, fa + d.part_lo_off + (long)t_ * 16);
}

// ==================================================================================================================================
// k3, per-frame form (segments.hpp: SegK3F): blockIdx.x = frame, 1024 lanes = 16 waves, one workgroup per CU — the whole of seg_k3_k's frame and seg_gate_k's work in
// one dependent chain instead of tiles_y * tiles_x chains in one and a half rounds plus a launch.  Each phase is the tile form's own text, included with this form's operands:
//   phase A  seg_gated_row.inc (gated_compute's row) per row tile — one z row, 16 columns of block tx: columns tx * TC - 1 .. — weights and the whole of lo2 from LDS;
//   phase B  seg_k3_rows.inc (seg_k3_k's rows) per (tile, wave-of-the-tile-form) unit: a unit adds its rows' `sum` in that wave's order, wave_reduce16<0> puts it where the
//            tile's workgroup would have, and 16 lanes per tile add the 16 slots as store_partials does — the partial sums of lo are the tile form's bits;
//   gate     seg_gate.inc on the first 256 lanes, in this kernel's order: part 0 and the FC weights with the first loads, part 1 from the partial sums in LDS behind phase B.
// Sharing the text moved no instruction of either form: tools/isa_same.py compares the ahead-of-time instances and the graph-specialised modules with another
// revision's, symbol by symbol (profiles/r14a_isa_same.txt); tests/test_gpu_k3_frame.py keeps the two forms' results bit-identical.  No global load behind the first barrier.
// In the graph-specialised module only (gen_seg.cpp defines BSX_SEG_K3F where the plan takes the form): the ahead-of-time fallback keeps seg_k3_k + seg_gate_k, the
// same bits — tests/test_device_order.py wants that fallback's k3 launch to be seg_k3_k, and a 1024-lane instance with the descriptor in registers needs 120 of them.
// ==================================================================================================================================
#if defined(BSX_SEG_RTC) && BSX_SEG_K3F
// load_wtile from the staged tile at sw + base: rows of kSegK3FWStride floats, conflict-free (tests/test_k3_frame_codegen.py).  (As a function it moved this kernel's code.)
#define BSX_K3F_WTILE(wr, base) _Pragma("unroll") for (int r = 0; r < 4; r++) wr[r] = sw[base + (4 * g + r) * kSegK3FWStride + li];
constexpr SegK3F kSegK3F = seg_k3f_layout(kSegK3);
static_assert(kSegK3F.on && kSegTAIL.pre_gate_off >= 0 && kSegTAIL.gate.n_parts == 2 && kSegTAIL.gate.part[1].off == kSegK3.part_lo_off &&
              kSegTAIL.gate.part[1].n == kSegK3.tiles_y * kSegK3.tiles_x, "k3: the per-frame form does not fit this plan");
extern "C" __global__ __launch_bounds__(kSegK3FThreads) void bsx_seg_k3f(float* __restrict__ arena, long per_frame, const float* __restrict__ w) {
  constexpr SegK3 d = kSegK3;
  constexpr SegK3F L = kSegK3F;
  constexpr SegGate gt = kSegTAIL.gate;
  constexpr long long pre_gate_off = kSegTAIL.pre_gate_off;
  __shared__ __attribute__((aligned(16))) float smem[L.lds_floats];   // (static: the planned size is a constant here, and the function needs no attribute for its 100+ KiB)
  float* fa = arena + (size_t)blockIdx.x * (size_t)per_frame;
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6), li = lane & 15, g = lane >> 4, cq4 = 4 * g;
  const int H = d.H2, W = d.W2, TX = d.tiles_x, ZRW = TX * 256, ntile = (H + 2) * TX, tiles = d.tiles_y * TX, HL = d.HL, LRW = d.WL * kLoStride;
  const bool half_pixel = d.half_pixel != 0;
  float* z_t = smem + L.z_off;                                      // [H + 2][TX][16][16]: row zy = image row zy - 1
  float* l_t = smem + L.lo_off;                                     // lo2 [HL][WL][16]
  float* sw = smem + L.w_off;
  float* s_red = smem + L.red_off;
  float* s_plo = smem + L.plo_off;
  float* s_g2 = smem + kSegK3FGate;
  float* lo_out = fa + d.lo_off;
  // ---- every global read of the frame: skip operands (registers), lo2, the level-2 gate, every weight, the tail gate's A partial sums and FC weights
  float4 skp[kSegK3FRows];
#pragma unroll
  for (int j = 0; j < kSegK3FRows; j++) {
    const int t = wave + 16 * j, zy = t / TX, tx = t - zy * TX, iy = zy - 1, ix = tx * d.TC - 1 + li;
    skp[j] = f4zero();
    if (t < ntile && iy >= 0 && iy < H && ix >= 0 && ix < W) skp[j] = ldg4<H16>(fa + d.skip_off, (unsigned)((iy * W + ix) * 16 + cq4));
  }
  const int npl = d.HL * d.WL * 4;                                  // 16-byte pieces of lo2: piece p = quad p & 3 of pixel p >> 2
  float4 lv[kSegK3FLoPieces];
#pragma unroll
  for (int j = 0; j < kSegK3FLoPieces; j++) {
    const int p = tid + kSegK3FThreads * j;
    lv[j] = f4zero();
    if (p < npl) lv[j] = ldg4<H16>(fa + d.lo2_off, (unsigned)(4 * p));
  }
  // weights: piece wp of kSegK3FWPieces on lanes 256 .. (the first 256 lanes carry the gate's loads); a 1x1 tile piece = row (q & 15), columns 4 * (q >> 4) ..
  const int wp = tid - 256;
  int w_dst = 0;
  float4 wv = f4zero();
  if (wp >= 0 && wp < kSegK3FWPieces) {
    const float* src;
    if (wp < 64) { src = w + d.pw1.w_off + (unsigned)((wp & 15) * d.pw1.cout_pad + 4 * (wp >> 4)); w_dst = (wp & 15) * kSegK3FWStride + 4 * (wp >> 4); }
    else if (wp < 68) { src = w + d.pw1.b_off + 4 * (wp - 64); w_dst = kSegK3FWB1 + 4 * (wp - 64); }
    else if (wp < 104) { src = w + d.dw.w_off + 4 * (wp - 68); w_dst = kSegK3FWDw + 4 * (wp - 68); }
    else if (wp < 108) { src = w + d.dw.b_off + 4 * (wp - 104); w_dst = kSegK3FWDwB + 4 * (wp - 104); }
    else if (wp < 172) { const int q = wp - 108; src = w + d.pw2.w_off + (unsigned)((q & 15) * d.pw2.cout_pad + 4 * (q >> 4)); w_dst = kSegK3FWPw2 + (q & 15) * kSegK3FWStride + 4 * (q >> 4); }
    else { src = w + d.pw2.b_off + 4 * (wp - 172); w_dst = kSegK3FWB2 + 4 * (wp - 172); }
    wv = ld4(src);
  }
  float g2 = 0.f;
  if (tid >= 512 && tid < 528) g2 = fa[d.g_off + (tid - 512)];
#define BSX_GATE_SCR smem                                            // the tail gate (seg_gate.inc): its first pooled tensor and the FC weights
#define BSX_GATE_STAGE smem + L.stage_off
#define BSX_GATE_SRC(k) ((k) == 0 ? fa + gt.part[0].off : s_plo)      // the second pooled tensor is lo: its partial sums are still in LDS
#define BSX_GATE_FC_LANE tid < kSegThreads
#define BSX_GATE_FC_CAPTURE tid
#define BSX_GATE_PART 1
#include "seg_gate.inc"
  if (tid < kSegThreads) {
#define BSX_GATE_K 0
#define BSX_GATE_PART 2
#include "seg_gate.inc"
#define BSX_GATE_PART 3
#include "seg_gate.inc"
  }
#pragma unroll
  for (int j = 0; j < kSegK3FLoPieces; j++) {
    const int p = tid + kSegK3FThreads * j, pix = p >> 2, ly = pix / d.WL, lx = pix - ly * d.WL;
    if (p < npl) st4(l_t + ly * LRW + col_l(lx, p & 3), lv[j]);
  }
  if (wp >= 0 && wp < kSegK3FWPieces) st4(sw + w_dst, wv);
  if (tid >= 512 && tid < 528) s_g2[tid - 512] = g2;
  __syncthreads();

  // ---- phase A: z = act(pw1(skip * g + up(lo2))), zero outside the image (gated_compute's arithmetic; the window offsets ly0 / lx0 are 0: the whole of lo2 is here)
  {
    float wr[4];
    BSX_K3F_WTILE(wr, 0)
    const float4 bias = ld4(sw + kSegK3FWB1 + cq4);
    const float4 gv = ld4(s_g2 + cq4);
    const Clamp cl = clamp_of(d.pw1.act);
    const float hs = d.hs;
#pragma unroll
    for (int j = 0; j < kSegK3FRows; j++) {
      const int t = wave + 16 * j;
      if (t >= ntile) break;
      const int zy = t / TX, tx = t - zy * TX, iy = zy - 1, ix = tx * d.TC - 1 + li;
      int x0, x1;
      float dx;
      up_axis(min(max(ix, 0), W - 1), d.ws, half_pixel, d.WL, &x0, &x1, &dx);
      const int xo0 = col_l(x0, g), xo1 = col_l(x1, g);
      const bool ecol_in = ix >= 0 && ix < W;
#define BSX_GR_LO_ROW(y) (l_t + (y) * LRW)
#define BSX_GR_SKIP skp[j]
#define BSX_GR_STORE(v) st4(z_t + zy * ZRW + tx * 256 + col_a(li, g), v)
#include "seg_gated_row.inc"
    }
  }
  // ---- phase B: t = z + act(dw3x3(z)) on the MFMA's own lanes, straight into pw2 (seg_k3_k's loop; unit u = (tile u >> 2, that tile's wave u & 3))
  {
    const int pc = min(li, 13);
    const int coz[3] = {col_a(pc, g), col_a(pc + 1, g), col_a(pc + 2, g)};
    f4v wd[9];
#pragma unroll
    for (int k = 0; k < 9; k++) wd[k] = ldv(sw + kSegK3FWDw + k * 16 + cq4);
    const f4v bias_d = ldv(sw + kSegK3FWDwB + cq4);
    const Clamp cl_dw = clamp_of(d.dw.act), cl_2 = clamp_of(d.pw2.act);
    float wr[4];
    BSX_K3F_WTILE(wr, kSegK3FWPw2)
    const float4 bias2 = ld4(sw + kSegK3FWB2 + cq4);
    __syncthreads();
    for (int u = wave; u < 4 * tiles; u += 16) {
      const int t = u >> 2, ow = u & 3, ty = t / TX, tx = t - ty * TX, r0 = ty * d.TR, c0 = tx * d.TC;
      const float* zb = z_t + tx * 256;                               // the tile's block: its row py + fy is frame row r0 + py + fy
      float4 sum = f4zero();
#define BSX_K3R_FIRST ow
#define BSX_K3R_Z zb
#define BSX_K3R_ZRW ZRW
#define BSX_K3R_ZROW(py) (r0 + (py))
#include "seg_k3_rows.inc"
      wave_reduce16<0>(sum, s_red + t * 256, ow, lane);
    }
  }
  __syncthreads();
  if (tid < 16 * tiles) {                                             // store_partials, one tile per 16 lanes; the sums stay in LDS for the gate
    const float* r = s_red + (tid >> 4) * 256;
    float s = 0.f;
    BSX_SLOTS_SUM16(s, r, tid & 15);
    (fa + d.part_lo_off)[tid] = s;
    s_plo[tid] = s;
  }
  __syncthreads();
  // ---- the tail's gate: its second pooled tensor from LDS, then seg_gate's means and FC chain
  if (tid < kSegThreads)
#define BSX_GATE_K 1
#define BSX_GATE_PART 2
#include "seg_gate.inc"
  __syncthreads();
#define BSX_GATE_PART 4
#include "seg_gate.inc"
  if (tid < 16) fa[pre_gate_off + tid] = s_gate[tid];
}
#endif

// ==================================================================================================================================
// tail (decoder level 1 + output): g = gate(GAP(A), GAP(lo)); z = act(pw(A * g + up(lo))); t = z + act(dw3x3(z));
// out = act3(Convolution2DTransposeBias 2x2 (t)) → logits (LOGITS) or straight into decode + temporal IIR on `ofinal`.
// Tile = TR x TC (<= 14) at the A resolution = 2TR x 2TC output pixels.  Phase B lanes = the MFMA's: lane (li, g) = (pixel li of the tile row, channel
// quad g) runs the depthwise on its 4 channels, and its t = z + act(dw(z)) IS the B operand of the transpose convolution, one 16 x 16 MFMA tile per row
// (A = the 2 x 2 x CO filter as 16 rows n = 4 * pos + oc): lane (li, g) ends up with output position (fy, fx) = (g >> 1, g & 1) of pixel li.
// INVARIANT the MFMA forms here and in seg_k2_k / seg_k3_k rely on: a D column depends on the SAME B column only.  Lanes li >= TC (and LDS columns x >= BC in k2)
// feed unwritten LDS into B; their D columns are garbage and every store / sum of an MFMA result below is guarded by the lane's own pixel being inside the tile
// (lane_on / x2 < BC).  A new consumer of those results must carry the same guard.
// ==================================================================================================================================
#ifdef BSX_SEG_RTC
extern "C" __global__ __launch_bounds__(kSegThreads) __attribute__((amdgpu_waves_per_eu(5, 5))) void bsx_seg_tail(
#else
template <int CO, bool LOGITS, bool SIGMOID, bool H16>
__global__ __launch_bounds__(kSegThreads) __attribute__((amdgpu_waves_per_eu(5, 5))) void seg_tail_k(
#endif
    const SegTail d_rt, float* __restrict__ arena, long per_frame, float* __restrict__ net_out,
                                                          uint8_t* __restrict__ ofinal, const float* __restrict__ w, int n_frames, const int* __restrict__ slot_of) {
  BSX_SEG_D(SegTail, TAIL);
  unsigned f_, t_;
  xcd_frame_tile((unsigned)(d.tiles_y * d.tiles_x), (unsigned)n_frames, &f_, &t_);
  const int f = (int)f_, ty = (int)t_ / d.tiles_x, tx = (int)t_ - ty * d.tiles_x;
  const int r0 = ty * d.TR, c0 = tx * d.TC, ZH = d.TR + 2, ZC = d.TC + 2;
  float* fa = arena + (size_t)f * (size_t)per_frame;
  float* z_t = seg_smem + kScrFloats;                               // [ZH][16][16]
  float* l_t = z_t + max(ZH * 256, kGateStageFloats);               // staged window of lo
  uint8_t* of = ofinal + (size_t)(slot_of ? slot_of[f] : f) * (size_t)(d.H0 * d.W0);   // temporal state: slot slot_of[f] (bsx_step_batch_streams), else f — one scalar load
  float* no = net_out + (size_t)f * (size_t)(d.H0 * d.W0 * CO);
  // Phase B lanes = the MFMA's: lane (li, g) = (pixel li of the tile row, channel quad g) runs the depthwise on its 4 channels; its t = z + act(dw(z)) is then the B
  // operand of the transpose convolution, computed as ONE 16 x 16 MFMA tile per row (round 5): A = the 2x2xCO filter as 16 rows n = 4 * pos + oc (rows with oc >= CO are
  // zero) over k = 16 channels, so the accumulator of lane (li, g) holds out[pos = g][oc = 0..CO) of pixel li — the lane ends up with output position (fy, fx) = (g >> 1, g & 1)
  // of its pixel, as before.  Until then every lane held the 4 x CO filter quads of its channels (32 registers at CO = 2), did 16 CO FMAs and three DPP exchanges
  // per output (quad_reduce_scatter): 124 registers = 4 workgroups per CU where LDS allows 5.  (Summation order over the 16 channels changes: within float rounding of
  // the reference order, as every 1x1 convolution here.)
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6), li = lane & 15, g = lane >> 4, cq4 = 4 * g;
  const int fy = g >> 1, fx = g & 1, ix = c0 + li;
  // every global read of the workgroup is requested here, before the first wait: skip operands, the window of lo, the temporal
  // state bytes this lane will update, then (inside seg_gate) the pooled partial sums and the gate weights
  const GatedPre pre = gated_prefetch<H16>(fa + d.skip_off, fa + d.lo_off, d.H1, d.W1, d.HL, d.WL, d.half_pixel != 0, d.hs, d.ws, r0, c0, ZH, ZC, l_t);
  constexpr int kRowsB = 5;                                          // TR <= 18 → <= 5 tile rows per wave in phase B
  const bool lane_on = li < d.TC && ix < d.W1;
  uint8_t prev[kRowsB];
  if (!LOGITS) {
#pragma unroll
    for (int j = 0; j < kRowsB; j++) {
      const int py = wave + 4 * j, iy = r0 + py;
      prev[j] = 0;
      if (py < d.TR && iy < d.H1 && lane_on) prev[j] = of[(unsigned)((2 * iy + fy) * d.W0 + 2 * ix + fx)];
    }
  }
  if (d.pre_gate_off >= 0) {                                          // computed once per frame by seg_gate_k
    if (tid < 16) seg_smem[kScrGate + tid] = fa[d.pre_gate_off + tid];
    __syncthreads();
  } else seg_gate(d.gate, fa, w, seg_smem, z_t);
  if (!(d.dbg_skip & 1)) gated_compute(pre, l_t, d.H1, d.W1, d.HL, d.WL, d.half_pixel != 0, d.hs, d.ws, seg_smem + kScrGate, d.pw, w, r0, c0, ZH, ZC, z_t);
  if (d.dbg_skip & 2) return;
  f4v wd[9];
#pragma unroll
  for (int k = 0; k < 9; k++) wd[k] = ldv(w + d.dw.w_off + k * 16 + cq4);
  const f4v bias_d = ldv(w + d.dw.b_off + cq4);
  float wtr[4];                                                       // A operand: lane (li, g) holds Wt[n = li][k = 4 g + r], n = 4 * pos + oc
#pragma unroll
  for (int r = 0; r < 4; r++) wtr[r] = (li & 3) < CO ? w[d.tc_w_off + (unsigned)((((li >> 2) * CO + (li & 3)) * 16) + cq4 + r)] : 0.f;
  float bt[CO];
#pragma unroll
  for (int oc = 0; oc < CO; oc++) bt[oc] = w[d.tc_b_off + oc];
  const Clamp cl_dw = clamp_of(d.dw.act);
  const int pc = min(li, 13);                                         // TC <= 14: lanes 14, 15 repeat lane 13's columns (dropped)
  const int coz[3] = {col_a(pc, g), col_a(pc + 1, g), col_a(pc + 2, g)};
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kRowsB; j++) {
    const int py = wave + 4 * j, iy = r0 + py;
    if (py >= d.TR || iy >= d.H1) break;                              // scalar: the MFMAs below run with every lane of the wave
    const f4v zc = ldv(z_t + (py + 1) * 256 + coz[1]);
    const float4 t4 = f4add(clamp4(tof4(dw3x3(z_t, 256, py, coz, wd) + bias_d), cl_dw), tof4(zc));
    const f4acc acc = mma16(t4, wtr);
    if (lane_on) {
      float o[CO];
#pragma unroll
      for (int oc = 0; oc < CO; oc++) {
        o[oc] = bt[oc] + acc[oc];
        if (SIGMOID) o[oc] = sigmoid1(o[oc]);
      }
      const int oy = 2 * iy + fy, ox = 2 * ix + fx;
      const unsigned opix = (unsigned)(oy * d.W0 + ox);
      if (LOGITS) {
#pragma unroll
        for (int oc = 0; oc < CO; oc++) no[opix * CO + oc] = o[oc];
      } else {
        uint32_t val;
        if (CO == 2) val = seg_meet_val(o[0], o[CO - 1]);
        else val = ((double)o[0] > 0.65) ? 0u : 255u;                // MLKit: float promoted to double against the double literal (libbackscrub.cc:338)
        of[opix] = (uint8_t)((val & 0xE0u) | ((uint32_t)prev[j] >> 3));
      }
    }
  }
}

#ifndef BSX_SEG_RTC                // ---- from here on: ahead-of-time build only (the per-frame gate kernel, a 5 us launch, and the host side)
// the gate of one decoder level, once per frame: workgroup = frame; the prologue of the tile kernels as a kernel of its own (SegTail::pre_gate_off)
__global__ __launch_bounds__(kSegThreads) void seg_gate_k(const SegGate gt, float* __restrict__ arena, long per_frame, const float* __restrict__ w, long long out_off) {
  float* fa = arena + (size_t)blockIdx.x * (size_t)per_frame;
  seg_gate(gt, fa, w, seg_smem, seg_smem + kScrFloats);
  if (threadIdx.x < 16) fa[out_off + threadIdx.x] = seg_smem[kScrGate + threadIdx.x];
}

// The ahead-of-time instance of each segment kernel for a variant: run-time flags to template arguments (pick), one function per kernel.  The graph-specialised
// kernels of gen_seg.cpp are the same code with the descriptor and these arguments as constants.  The nesting and the polarity of the flags fix the order in which
// the instances are instantiated, and with it their order in the code object: it is the order of the list of instances these functions replaced.
template <class F> const void* pick(bool b, F f) { return !b ? f(std::false_type{}) : f(std::true_type{}); }
template <class K> const void* kernel_ptr(K k) { return reinterpret_cast<const void*>(k); }
const void* seg_head_instance(bool hswish, bool h16, bool u8) {
  return pick(u8, [&](auto U) { return pick(h16, [&](auto H) { return pick(!hswish, [&](auto PLAIN) { return kernel_ptr(seg_head_k<!PLAIN, H, U>); }); }); });
}
const void* seg_k2_instance(bool h16) { return pick(h16, [](auto H) { return kernel_ptr(seg_k2_k<H>); }); }
const void* seg_k3_instance(bool h16) { return pick(h16, [](auto H) { return kernel_ptr(seg_k3_k<H>); }); }
// outputs: 2 channels (Meet), 1 channel with or without a sigmoid (MLKit); nullptr for any other
const void* seg_tail_instance(int co, bool sigmoid, bool logits, bool h16) {
  if (co != 1 && co != 2) return nullptr;
  return pick(h16, [&](auto H) { return pick(co == 2, [&](auto C2) { return pick(!sigmoid, [&](auto LINEAR) { return pick(logits, [&](auto L) -> const void* {
    if constexpr (C2 && !LINEAR) return nullptr;
    else return kernel_ptr(seg_tail_k<C2 ? 2 : 1, L, !LINEAR, H>);
  }); }); }); });
}

// One launch of a segment kernel: the graph-specialised function `fn` when there is one, else the ahead-of-time instance `aot`.  Grid, block, dynamic LDS and the
// argument list are the same either way.
hipError_t seg_launch(hipFunction_t fn, const void* aot, int tiles, int n, size_t lds, hipStream_t s, void** args) {
  const unsigned grid = (unsigned)tiles * (unsigned)n;
  if (fn) return hipModuleLaunchKernel(fn, grid, 1, 1, kSegThreads, 1, 1, (unsigned)lds, s, args, nullptr);
  if (!aot) return hipErrorInvalidValue;
  return hipLaunchKernel(aot, dim3(grid), dim3(kSegThreads), args, lds, s);
}
#endif

}  // namespace

#ifndef BSX_SEG_RTC
hipError_t seg_prepare() {
  const int full = 160 * 1024;     // process-global kernel attributes: always the full LDS (cf. frame_program_prepare)
  hipError_t e = hipSuccess;
  auto one = [&](const void* k) { if (e == hipSuccess && k) e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, full); };
  for (bool h16 : {false, true}) {
    for (bool hs : {false, true}) for (bool u8 : {false, true}) one(seg_head_instance(hs, h16, u8));
    one(seg_k2_instance(h16));
    one(seg_k3_instance(h16));
    for (int co : {1, 2}) for (bool sig : {false, true}) for (bool logits : {false, true}) one(seg_tail_instance(co, sig, logits, h16));
  }
  return e;
}

// fn: the graph-specialised kernel (specialised.hpp), or nullptr for the ahead-of-time instance of the variant.
// h16: the boundary tensors are stored as halves (BSX_ACT16; the middle program must have been generated for the same storage)
// u8: net_in points at the 8-bit network input ([n][H0][W0] u32 pixels, prep_fused_k<2>) and (scale, offset) is the model's normalisation
hipError_t launch_seg_head(hipFunction_t fn, const SegHead& d, float* arena, long per_frame, const void* net_in, const float* weights, int n, hipStream_t s, bool h16, bool u8,
                           float in_scale, float in_offset) {
  if (u8 && 2 * (2 * d.TC + 1) + 1 > 64) return hipErrorInvalidValue;          // one lane per pixel of an input-tile row (the planner's TC <= 15)
  const float* in = static_cast<const float*>(net_in);
  int nf = xcd_frames(n);
  void* args[] = {(void*)&d, &arena, &per_frame, &in, &weights, &in_scale, &in_offset, &nf};
  return seg_launch(fn, seg_head_instance(d.stem.act == kActHswish, h16, u8), d.tiles_y * d.tiles_x, n, (size_t)d.lds_floats * sizeof(float), s, args);
}
hipError_t launch_seg_k2(hipFunction_t fn, const SegK2& d, float* arena, long per_frame, const float* weights, int n, hipStream_t s, bool h16) {
  int nf = xcd_frames(n);
  void* args[] = {(void*)&d, &arena, &per_frame, &weights, &nf};
  return seg_launch(fn, seg_k2_instance(h16), d.tiles_y * d.tiles_x, n, (size_t)d.lds_floats * sizeof(float), s, args);
}
hipError_t launch_seg_k3(hipFunction_t fn, const SegK3& d, float* arena, long per_frame, const float* weights, int n, hipStream_t s, bool h16) {
  int nf = xcd_frames(n);
  void* args[] = {(void*)&d, &arena, &per_frame, &weights, &nf};
  return seg_launch(fn, seg_k3_instance(h16), d.tiles_y * d.tiles_x, n, (size_t)d.lds_floats * sizeof(float), s, args);
}
// k3's per-frame form, the tail's gate included (bsx_seg_k3f of the specialised module, there where SegK3F::on): grid = frames, 1024 lanes, its LDS a static array.
hipError_t launch_seg_k3_frame(hipFunction_t fn, const SegK3F& L, float* arena, long per_frame, const float* weights, int n, hipStream_t s) {
  if (!fn || !L.on) return hipErrorInvalidValue;
  void* args[] = {&arena, &per_frame, &weights};
  return hipModuleLaunchKernel(fn, (unsigned)n, 1, 1, kSegK3FThreads, 1, 1, 0, s, args, nullptr);
}
// logits: the stage-debug variant, ahead of time only (the specialised tail is the decode-fused one)
hipError_t launch_seg_tail(hipFunction_t fn, const SegTail& d, float* arena, long per_frame, float* net_out, uint8_t* ofinal, const float* weights, bool logits, int n,
                           hipStream_t s, bool h16, const int* slot_of) {
  // BSX_SEG_TAIL_WGS=<k> (experiment switch, read once): pad the dynamic LDS so that at most k workgroups fit a CU — the A/B of the tail's 5th workgroup (round 5)
  static const int wgs_cap = BSX_DBG_ENV("BSX_SEG_TAIL_WGS") ? atoi(BSX_DBG_ENV("BSX_SEG_TAIL_WGS")) : 0;
  size_t lds = (size_t)d.lds_floats * sizeof(float);
  if (wgs_cap > 0) lds = std::max(lds, (size_t)(160 * 1024 / (wgs_cap + 1) + 256));
  int nf = xcd_frames(n);
  void* args[] = {(void*)&d, &arena, &per_frame, &net_out, &ofinal, &weights, &nf, &slot_of};
  return seg_launch(logits ? nullptr : fn, seg_tail_instance(d.Co, d.act3 == kActSigmoid, logits, h16), d.tiles_y * d.tiles_x, n, lds, s, args);
}
hipError_t launch_seg_gate(const SegGate& gt, float* arena, long per_frame, const float* weights, long long out_off, int n, hipStream_t s) {
  seg_gate_k<<<n, kSegThreads, (size_t)(kSegScratchFloats + kSegGateStageFloats) * sizeof(float), s>>>(gt, arena, per_frame, weights, out_off);
  return hipGetLastError();
}

#endif

}  // namespace bsx
