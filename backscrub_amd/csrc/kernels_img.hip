// kernels_img.hip — integer/byte image kernels of the hot path for gfx950 (wave64).
//
// Every kernel here is bit-exact against the CPU oracle's restatement of the OpenCV 8-bit
// paths and of the reference's own loops; all are HBM-bound byte work, so the design rules
// are: 16-byte vector accesses per lane, LDS tiles for neighbourhood ops, no GEMM shapes.
//
//   prep_fused_k         libbackscrub.cc:285-302  ROI crop + cv::resize(INTER_LINEAR) + BGR2RGB + cv::bilateralFilter(5,100,100) + convertTo(CV_32FC3)
//   decode_k             libbackscrub.cc:317-357  argmax / threshold / softmax-2 + temporal IIR
//   mask_upscale_blur_k  libbackscrub.cc:367-371  cv::resize ↑ + cv::blur 5x5 into the persistent mask ROI
//   blend4x4_k           deepseg.cc:108-134       alpha_blend
//   resize_bgr_k         background.cc:186,190    cv::resize of the background
//   yuyv_k               deepseg.cc:87-106        convert_rgb_to_yuyv
#include "debug_switches.hpp"
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include "kernels.hpp"
#include "mfma_tile.hpp"

namespace bsx {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxGridY = 65535;
inline unsigned blocks_for(long total) { return (unsigned)((total + kThreads - 1) / kThreads); }

__device__ __forceinline__ int reflect101(int p, int len) {  // cv::borderInterpolate(BORDER_REFLECT_101)
  if (len == 1) return 0;
  while (p < 0 || p >= len) p = p < 0 ? -p : 2 * len - 2 - p;
  return p;
}

// One INTER_LINEAR sample of an interleaved u8 image at destination (dx,dy), channel c.
// Horizontal pass in int32 with 11-bit coefficients, vertical pass
// (((b0*(r0>>4))>>16) + ((b1*(r1>>4))>>16) + 2) >> 2  — OpenCV resize.cpp 8u fixed point.
template <int CN>
__device__ __forceinline__ void sample_linear(const uint8_t* __restrict__ src, long sstride, const ResizeTab& t, int dx, int dy, int* out) {
  if (t.mode == 1) {
    const uint8_t* p = src + (long)dy * sstride + (long)dx * CN;
#pragma unroll
    for (int c = 0; c < CN; c++) out[c] = p[c];
    return;
  }
  if (t.mode == 2) {  // INTER_AREA 2x2 (both scales exactly 2): (s00+s01+s10+s11+2)>>2
    const uint8_t* p = src + (long)(2 * dy) * sstride + (long)(2 * dx) * CN;
#pragma unroll
    for (int c = 0; c < CN; c++) out[c] = (p[c] + p[CN + c] + p[sstride + c] + p[sstride + CN + c] + 2) >> 2;
    return;
  }
  int sx = t.xofs[dx], sx1 = min(sx + 1, t.sw - 1);
  int a0 = t.xa[2 * dx], a1 = t.xa[2 * dx + 1];
  int sy = t.yofs[dy];
  int sy0 = min(max(sy, 0), t.sh - 1), sy1 = min(max(sy + 1, 0), t.sh - 1);
  int b0 = t.ya[2 * dy], b1 = t.ya[2 * dy + 1];
  const uint8_t* r0 = src + (long)sy0 * sstride;
  const uint8_t* r1 = src + (long)sy1 * sstride;
  if constexpr (CN == 3) {
    // both taps of a row are 6 consecutive bytes: ONE (unaligned) 8-byte load per row instead of six byte loads — the texture
    // address unit, not HBM, was the limit of the byte form.  Only when the 8 bytes stay inside the row.
    if (sx1 == sx + 1 && sx * 3 + 8 <= (int)sstride) {
      struct __attribute__((packed, aligned(1))) U8 { uint64_t v; };
      const uint64_t q0 = reinterpret_cast<const U8*>(r0 + sx * 3)->v, q1 = reinterpret_cast<const U8*>(r1 + sx * 3)->v;
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const int h0 = (int)((q0 >> (8 * c)) & 255) * a0 + (int)((q0 >> (8 * (3 + c))) & 255) * a1;
        const int h1 = (int)((q1 >> (8 * c)) & 255) * a0 + (int)((q1 >> (8 * (3 + c))) & 255) * a1;
        out[c] = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
      }
      return;
    }
  }
#pragma unroll
  for (int c = 0; c < CN; c++) {
    int h0 = r0[sx * CN + c] * a0 + r0[sx1 * CN + c] * a1;
    int h1 = r1[sx * CN + c] * a0 + r1[sx1 * CN + c] * a1;
    out[c] = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
  }
}

// ---- prep: bilateral d=5 constants (libbackscrub.cc:295-302).  f32 accumulation in tap order with separate multiply and add (no FMA contraction), then
// cvRound(sum * (1/wsum)) — the association the oracle defines.
constexpr int kBilPix = 4;   // pixels per lane: amortises the 768-entry LUT fill + barrier of every workgroup
// the 13 taps of a radius-2 disc in OpenCV's (dy, dx) row-major order; bsx_api.hip builds bp.space_w in the same order
// and refuses to start if its table ever disagrees (bilateral_taps_match)
__device__ constexpr int kTapY[13] = {-2, -1, -1, -1, 0, 0, 0, 0, 0, 1, 1, 1, 2};
__device__ constexpr int kTapX[13] = {0, -1, 0, 1, -2, -1, 0, 1, 2, -1, 0, 1, 0};
// OUT bit 0: the network input as f32 [n][inH][inW][3] = convertTo (libbackscrub.cc:302) — what stems without a byte path and the stage tests read;
// bit 1: the filtered pixel itself, R | G<<8 | B<<16 [n][inH][inW] u32 — the stems that take it (seg_head_k, dl_head0_k) apply the SAME two roundings
// `fadd(fmul(float(q), scale), offset)` when they stage their input window, so the 12 B/px tensor never exists (bit-identical by construction).
// ---- YUYV -> BGR inside the kernels that read the camera frame (BSX_STEP_YUYV_IN: cv::COLOR_YUV2BGR_YUYV, app/deepseg.cc:553,725) --------------------------------
// The same integers as yuyv_to_bgr_k below (BT.601 limited range, 20-bit fixed point): a step that takes the camera's raw 2 B/px never materialises
// the 3 B/px BGR frame.  Every product is a full-rate 24-bit multiply (|c| < 2^23, |operand| <= 255).
constexpr int kYuvSH = 20, kYuvCY = 1220542, kYuvCUB = 2116026, kYuvCUG = -409993, kYuvCVG = -852492, kYuvCVR = 1673527;
// Saturating pack: sat_u8(lo >> 20) | sat_u8(hi >> 20) << 8 in ONE instruction (gfx950's v_ashr_pk_u8_i32) — spelled out, with its upper half masked, because the
// compiler's own use of the instruction is wrong on this toolchain (ROCm 7.2, clang 22): it forms it from `min(max(x >> 20, 0), 255)` pairs and then ORs further
// bytes into the result as if bits 31:16 were zero, while the hardware leaves whatever the destination register held there (found by tools/dbg_conv.hip: bytes 2-3
// of every word built that way carried bits of the unshifted sums).  Through the asm the compiler cannot see what the value is, so the mask stays.
__device__ __forceinline__ uint32_t sat_pk2_shr20(int lo, int hi) {
  uint32_t d;
  asm("v_ashr_pk_u8_i32 %0, %1, %2, 20" : "=v"(d) : "v"(lo), "v"(hi));
  return d;                                                      // bits 15:0 valid; callers mask or shift the rest away
}
__device__ __forceinline__ void yuv_chroma(int u, int v, int* buv, int* guv, int* ruv) {      // u, v already minus 128
  *ruv = (1 << (kYuvSH - 1)) + __mul24(kYuvCVR, v);
  *guv = (1 << (kYuvSH - 1)) + __mul24(kYuvCVG, v) + __mul24(kYuvCUG, u);
  *buv = (1 << (kYuvSH - 1)) + __mul24(kYuvCUB, u);
}
__device__ __forceinline__ int yuv_luma(uint32_t y) { return __mul24(max(0, (int)y - 16), kYuvCY); }
// one tap of prep_fused_k: Y | U << 8 | V << 16 (pulled out of the 8-byte window by v_perm_b32) -> B | G << 8 | R << 16
__device__ __forceinline__ uint32_t yuv_tap_to_bgr(uint32_t t) {
  int buv, guv, ruv;
  yuv_chroma((int)((t >> 8) & 255u) - 128, (int)((t >> 16) & 255u) - 128, &buv, &guv, &ruv);
  const int ya = yuv_luma(t & 255u);
  return (sat_pk2_shr20(ya + buv, ya + guv) & 0xffffu) | ((sat_pk2_shr20(ya + ruv, 0) & 0xffu) << 16);
}
// four pixels = two YUYV words (Y0 U Y1 V) -> the three words of four packed BGR pixels (the operand form of blend_quad): six saturating packs, one per byte pair
// of the output — B0 G0 | R0 B1 | G1 R1 | B2 G2 | R2 B3 | G3 R3
__device__ __forceinline__ void yuyv4_to_bgr3(uint32_t p0, uint32_t p1, uint32_t o[3]) {
  int bu0, gu0, ru0, bu1, gu1, ru1;
  yuv_chroma((int)((p0 >> 8) & 255u) - 128, (int)(p0 >> 24) - 128, &bu0, &gu0, &ru0);
  yuv_chroma((int)((p1 >> 8) & 255u) - 128, (int)(p1 >> 24) - 128, &bu1, &gu1, &ru1);
  const int y0 = yuv_luma(p0 & 255u), y1 = yuv_luma((p0 >> 16) & 255u), y2 = yuv_luma(p1 & 255u), y3 = yuv_luma((p1 >> 16) & 255u);
  o[0] = (sat_pk2_shr20(y0 + bu0, y0 + gu0) & 0xffffu) | (sat_pk2_shr20(y0 + ru0, y1 + bu0) << 16);
  o[1] = (sat_pk2_shr20(y1 + gu0, y1 + ru0) & 0xffffu) | (sat_pk2_shr20(y2 + bu1, y2 + gu1) << 16);
  o[2] = (sat_pk2_shr20(y2 + ru1, y3 + bu1) & 0xffffu) | (sat_pk2_shr20(y3 + gu1, y3 + ru1) << 16);
}

// ---- prep, both steps in ONE kernel: the workgroup resizes the (TW + 4) x (TH + 4) canvas pixels its bilateral tile reads straight into LDS -------
// (every sample of a lane requested before its first use: <= 6 independent tap pairs in flight per lane), filters from LDS and writes the network input.  The
// two-kernel form of rounds 1-2 (resize into a 4 B/px canvas with a stored BORDER_REFLECT_101 apron, then the bilateral reading it back: one write and one read of
// the canvas, a launch boundary, lanes that each waited for one dependent pair of loads) was bit-identical to this and was deleted in round 6; the halo is
// recomputed (1.27x the samples of a 32 x 32 tile, L2 hits).  The stage-0 tests read its output.  Tile sizes are chosen per model so that the tiles cover the
// canvas without a sliver (257 = 9 x 29, not 8 x 32 + 1).
constexpr int kPfS = 36;                    // LDS row stride of the tile (TW <= 32)
// YIN (BSX_STEP_YUYV_IN, LINEAR only): `frames` holds YUYV 4:2:2 (Y0 U Y1 V per pixel pair, 2 B/px) — the two taps of a sample are converted with
// cv::COLOR_YUV2BGR_YUYV's integers (yuv_tap_to_bgr) as they leave the 8-byte window, then resized exactly as BGR taps are: the same network input, bit for bit,
// as bsx_yuyv_to_bgr followed by the BGR step, without the 3 B/px frame in between.  The ROI must start on an even column (a macropixel).
template <int OUT, bool LINEAR, bool YIN = false>             // LINEAR: tab.mode == 0 (cv::resize INTER_LINEAR proper — the other modes are a copy and the exact 2x2 area average)
__global__ __launch_bounds__(kThreads) void prep_fused_k(const uint8_t* __restrict__ frames, int W, int H, Rect4 roi, float* __restrict__ input, uint32_t* __restrict__ input_u8,
                                                        int inW, int inH, Rect4 q, ResizeTab tab, BilateralParams bp, int TW, int TH, int ntx, int nty, int n_frames) {
  __shared__ float lut[768];
  __shared__ uint32_t tile[kPfS * kPfS];
  const int tid = threadIdx.x;
  unsigned f_, t_;
  xcd_frame_tile((unsigned)(ntx * nty), (unsigned)n_frames, &f_, &t_);      // a frame's tiles on ONE XCD: their shared halo lines are L2 hits
  const long n = f_;
#define BSX_PREP_FRAME n
#include "prep_tile.inc"
#undef BSX_PREP_FRAME
}
// the same body for ONE frame given by its own pointer (bsx_step_batch_geoms: prep_geoms_k below): tile t_ of its canvas, network input slot n
template <int OUT, bool LINEAR>
__device__ __forceinline__ void prep_geoms_tile(const uint8_t* __restrict__ frames, int W, int H, Rect4 roi, float* __restrict__ input, uint32_t* __restrict__ input_u8,
                                                int inW, int inH, Rect4 q, const ResizeTab& tab, const BilateralParams& bp, int TW, int TH, int ntx, const long n,
                                                const unsigned t_) {
  __shared__ float lut[768];
  __shared__ uint32_t tile[kPfS * kPfS];
  constexpr bool YIN = false;
  const int tid = threadIdx.x;
#define BSX_PREP_FRAME 0l
#include "prep_tile.inc"
#undef BSX_PREP_FRAME
}

// ---- decode + temporal IIR -------------------------------------------------------------------
// slot_of (the id form of a step, launch_decode): frame blockIdx.y's temporal state is slot slot_of[blockIdx.y] and `total` counts ONE frame's pixels; the dense form
// launches one flat grid (blockIdx.y = 0, slot_of = nullptr).  Same for the three kernels below.
__device__ __forceinline__ long decode_state_frame(const int* __restrict__ slot_of) { return slot_of ? slot_of[blockIdx.y] : (long)blockIdx.y; }
__global__ __launch_bounds__(kThreads) void decode_k(int type, const float* __restrict__ t, uint8_t* __restrict__ out, long total, int nch, const int* __restrict__ slot_of) {
  long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  t += (long)blockIdx.y * total * nch;
  out += decode_state_frame(slot_of) * total;
  uint8_t val = 255;
  if (type == 1) {  // DeepLab: first maximum wins, start value -10000, "person" = 15
    const float* p = t + i * nch;
    float maxval = -10000.f; int maxpos = 0;
    for (int c = 0; c < nch; c++) { float v = p[c]; if (v > maxval) { maxval = v; maxpos = c; } }
    val = maxpos == 15 ? 0 : 255;
  } else if (type == 2) {  // MLKit / BodyPix: float promoted to double against the double literal 0.65
    val = ((double)t[i] > 0.65) ? 0 : 255;
  } else {  // Meet: expf on both logits, normalise, compare (NaN from inf/inf compares false → 255)
    const float2 l = reinterpret_cast<const float2*>(t)[i];
    // Decided-by-margin fast path.  For logits in [-80, 80] (no overflow of exp or of the sum) that differ by >= 1e-4 the
    // outcome of the reference arithmetic is forced: exp is monotone with relative error < 2^-23, so e1/e0 > 1 + 9.9e-5;
    // the two correctly-rounded divisions by the same s perturb that ratio by < 2^-23 more, hence p0 < p1 strictly (and
    // symmetrically p0 > p1).  Only near-ties and out-of-range / NaN logits take the exact path below.
    const float d = l.y - l.x;
    if (fabsf(l.x) <= 80.f && fabsf(l.y) <= 80.f && fabsf(d) >= 1e-4f) {
      val = d > 0.f ? 0 : 255;
    } else {
      float e0 = (float)exp((double)l.x), e1 = (float)exp((double)l.y);  // correctly-rounded stand-in for libm expf
      float s = __fadd_rn(e0, e1);
      float p0 = __fdiv_rn(e0, s), p1 = __fdiv_rn(e1, s);
      val = p0 < p1 ? 0 : 255;
    }
  }
  out[i] = (uint8_t)((val & 0xE0) | (out[i] >> 3));
}

// Meet decode, 4 pixels per lane: two 16-byte logit loads, one 4-byte state word read-modified-written.  Same per-pixel
// arithmetic as decode_k (fast path by margin, exact path for near ties / out-of-range / NaN logits).
__device__ __forceinline__ uint32_t meet_val(float l0, float l1) {
  const float d = l1 - l0;
  if (fabsf(l0) <= 80.f && fabsf(l1) <= 80.f && fabsf(d) >= 1e-4f) return d > 0.f ? 0u : 255u;
  const float e0 = (float)exp((double)l0), e1 = (float)exp((double)l1);
  const float s = __fadd_rn(e0, e1);
  return __fdiv_rn(e0, s) < __fdiv_rn(e1, s) ? 0u : 255u;
}
__global__ __launch_bounds__(kThreads) void decode_meet4_k(const float4* __restrict__ t, uint32_t* __restrict__ out, long quads, const int* __restrict__ slot_of) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= quads) return;
  t += (long)blockIdx.y * quads * 2;
  out += decode_state_frame(slot_of) * quads;
  const float4 a = t[2 * i], b = t[2 * i + 1];               // (l0,l1) of pixels 0,1 | 2,3
  const uint32_t v = meet_val(a.x, a.y) | (meet_val(a.z, a.w) << 8) | (meet_val(b.x, b.y) << 16) | (meet_val(b.z, b.w) << 24);
  const uint32_t o = out[i];
  out[i] = (v & 0xE0E0E0E0u) | ((o >> 3) & 0x1F1F1F1Fu);      // per byte: (val & 0xE0) | (out >> 3)
}

// MLKit / BodyPix decode, 4 pixels per lane: `p > 0.65` with the float promoted to double (the literal is a double, libbackscrub.cc:338)
__global__ __launch_bounds__(kThreads) void decode_thresh4_k(const float4* __restrict__ t, uint32_t* __restrict__ out, long quads, const int* __restrict__ slot_of) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= quads) return;
  t += (long)blockIdx.y * quads;
  out += decode_state_frame(slot_of) * quads;
  const float4 p = t[i];
  const uint32_t v = ((double)p.x > 0.65 ? 0u : 255u) | (((double)p.y > 0.65 ? 0u : 255u) << 8) | (((double)p.z > 0.65 ? 0u : 255u) << 16) |
                     (((double)p.w > 0.65 ? 0u : 255u) << 24);
  const uint32_t o = out[i];
  out[i] = (v & 0xE0E0E0E0u) | ((o >> 3) & 0x1F1F1F1Fu);
}

// DeepLab argmax over nch interleaved classes: the 256 pixels of a workgroup are one contiguous block of 256*nch floats —
// read it with coalesced 4-byte loads into LDS, then every lane scans its own nch values (stride nch, conflict-free for odd
// nch).  A lane reading its classes straight from HBM touches 64 cache lines per load instruction.
constexpr int kArgmaxMaxCh = 32;
__global__ __launch_bounds__(kThreads) void decode_argmax_k(const float* __restrict__ t, uint8_t* __restrict__ out, long total, int nch, const int* __restrict__ slot_of) {
  __shared__ float tile[kThreads * kArgmaxMaxCh];
  const long p0 = (long)blockIdx.x * kThreads;
  t += (long)blockIdx.y * total * nch;
  out += decode_state_frame(slot_of) * total;
  const int valid = (int)min((long)kThreads, total - p0);
  const float* src = t + p0 * nch;
  for (int i = threadIdx.x; i < valid * nch; i += kThreads) tile[i] = src[i];
  __syncthreads();
  if ((int)threadIdx.x >= valid) return;
  const float* p = tile + threadIdx.x * nch;
  float maxval = -10000.f; int maxpos = 0;                       // libbackscrub.cc:318-332: first maximum wins
  for (int c = 0; c < nch; c++) { const float v = p[c]; if (v > maxval) { maxval = v; maxpos = c; } }
  const uint8_t val = maxpos == 15 ? 0 : 255;                    // class 15 = person
  out[p0 + threadIdx.x] = (uint8_t)((val & 0xE0) | (out[p0 + threadIdx.x] >> 3));
}

// ---- mask: upscale + 5x5 box blur, LDS tiled, separable -------------------------------------------------------------
// Tile = 128x32 output pixels per 256-lane workgroup.  All table lookups happen once per tile column / tile row:
//   1. per column of the (128+4)-wide halo tile: reflected ROI x → (sx, sx1, a0, a1);  per row of the (32+4)-tall
//      halo tile: reflected ROI y → (sy0, sy1, b0, b1)                               [LDS]
//   2. horizontal pass of cv::resize for the <= kMaxSrcRows source rows the tile touches:  hq[sy][x] = (S0*a0 + S1*a1) >> 4
//   3. vertical pass: up[y][x] = (((b0*hq[sy0][x]) >> 16) + ((b1*hq[sy1][x]) >> 16) + 2) >> 2   (exactly OpenCV's 8u formula)
//   4. horizontal 5-sums (u16), 5. vertical 5-sums, (s+12)/25, 4 pixels per 32-bit store.
// Steps 2-3 are the separable form of the per-pixel bilinear sample: identical integers, ~4x fewer operations.
// With BLEND the same workgroup also composites its tile (deepseg.cc:108-134) while the mask bytes are still in
// registers: the mask is written once and never re-read, and the HBM-bound blend traffic of some workgroups overlaps
// the LDS/ALU-bound mask phases of others.  (Used when W, roi.x and roi.w are multiples of 4; outside the ROI the composite
// is the background itself, copied by outside_roi_copy_k.)
typedef unsigned short us2 __attribute__((ext_vector_type(2)));   // v_pk_*_u16 operand
constexpr int kTW = 128, kTH = 32, kHW = kTW + 4, kHH = kTH + 4, kMaxSrcRows = 40;
constexpr int kTileItems = kTH * (kTW / 4) / kThreads;     // 4-pixel groups per lane in the last step
static_assert(kTileItems * kThreads == kTH * (kTW / 4) && kThreads == 8 * (kTW / 4), "tile / lane mapping: item i of a lane sits 8 rows below item i-1");

// ---- packed alpha-blend arithmetic (deepseg.cc:108-134), shared by the mask tile kernels and blend4x4_k --------------------
// Packed form of the same integers (v_pk_*_u16, two bytes per instruction):  a*m + b*(255-m) <= 255*255 fits a u16 lane,
// and floor(t/255) == (t + 1 + (t >> 8)) >> 8 for every t in [0, 65025] (exhaustively checked; the sum stays < 65536).
// Round 5: u = a*m + 1 + b*(255-m) as two v_pk_mad_u16 (u <= 65026 fits a u16 lane) and floor((u-1)/255) == (u + (u >> 8)) >> 8 (exhaustive: tests/test_oracle_image.py;
// u + (u >> 8) <= 65280) — five packed instructions per two bytes instead of six; the odd bytes of a word are pulled into u16 lanes by ONE v_perm_b32 each (was shift + and).
// 67 -> 55 VALU instructions per four pixels: the fused mask + blend's general tiles run their VALU at 75 % busy (profiles/r05z_pmc_sq_lite.md).
__device__ __forceinline__ us2 pk_blend(uint32_t a, uint32_t b, uint32_t m, uint32_t im) {   // operands: two u8 values in the u16 halves; im = 0x00ff00ff ^ m = 255 - m per half
  const us2 av = __builtin_bit_cast(us2, a), bv = __builtin_bit_cast(us2, b), mv = __builtin_bit_cast(us2, m), iv = __builtin_bit_cast(us2, im);
  // (written as `av * mv + one` the compiler moves the constant to the end of the sum: multiply, multiply-add, add — the first fused form is spelled out)
  uint32_t u0;
  asm("v_pk_mad_u16 %0, %1, %2, %3" : "=v"(u0) : "v"(a), "v"(m), "s"(0x00010001u));
  (void)av; (void)mv;
  us2 u = bv * iv + __builtin_bit_cast(us2, u0);
  return (u + (u >> 8)) >> 8;
}
__device__ __forceinline__ uint32_t blend_word(uint32_t a, uint32_t b, uint32_t m02, uint32_t m13) {
  const uint32_t K = 0x00ff00ffu;
  const uint32_t r02 = __builtin_bit_cast(uint32_t, pk_blend(a & K, b & K, m02, m02 ^ K));
  const uint32_t r13 = __builtin_bit_cast(uint32_t, pk_blend(__builtin_amdgcn_perm(a, a, 0x0c030c01u), __builtin_amdgcn_perm(b, b, 0x0c030c01u), m13, m13 ^ K));
  return r02 | (r13 << 8);
}
typedef uint32_t u3v __attribute__((ext_vector_type(3)));      // four packed BGR pixels: one global_{load,store}_dwordx3 (4-byte aligned)
// 4 pixels = 12 bytes = 3 words; mw holds their 4 mask bytes.  Byte→pixel map of the words: (0,0,0,1) (1,1,2,2) (2,3,3,3).
__device__ __forceinline__ void blend_quad(const uint32_t a[3], const uint32_t b[3], uint32_t mw, uint32_t o[3]) {
  const uint32_t m00 = __builtin_amdgcn_perm(mw, mw, 0x0c000c00u), m01 = __builtin_amdgcn_perm(mw, mw, 0x0c010c00u);
  const uint32_t m12 = __builtin_amdgcn_perm(mw, mw, 0x0c020c01u);
  const uint32_t m23 = __builtin_amdgcn_perm(mw, mw, 0x0c030c02u), m33 = __builtin_amdgcn_perm(mw, mw, 0x0c030c03u);
  o[0] = blend_word(a[0], b[0], m00, m01);
  o[1] = blend_word(a[1], b[1], m12, m12);
  o[2] = blend_word(a[2], b[2], m23, m33);
}

// ---- BGR → YUYV (cv::cvtColor(COLOR_RGB2YUV) on BGR-ordered bytes, then 4:2:2 pack Y0 V Y1 U) -----
__device__ __forceinline__ void rgb2yuv(int R, int G, int B, int* Y, int* U, int* V) {
  const int shift = 14, half = 1 << 13, delta = 128 << 14;
  int y = (R * 4899 + G * 9617 + B * 1868 + half) >> shift;
  int u = ((B - y) * 8061 + delta + half) >> shift;
  int v = ((R - y) * 14369 + delta + half) >> shift;
  *Y = min(max(y, 0), 255); *U = min(max(u, 0), 255); *V = min(max(v, 0), 255);
}
// two neighbouring pixels (bytes as stored: channel 0 is taken as "R", deepseg.cc:90) → one YUYV word Y0 | V<<8 | Y1<<16 | U<<24
__device__ __forceinline__ uint32_t yuyv_pair(uint32_t a0, uint32_t a1, uint32_t a2, uint32_t b0, uint32_t b1, uint32_t b2) {
  int y0, u0, v0, y1, u1, v1;
  rgb2yuv((int)a0, (int)a1, (int)a2, &y0, &u0, &v0);
  rgb2yuv((int)b0, (int)b1, (int)b2, &y1, &u1, &v1);
  return (uint32_t)y0 | ((uint32_t)((v0 + v1) / 2) << 8) | ((uint32_t)y1 << 16) | ((uint32_t)((u0 + u1) / 2) << 24);
}

// ---- pieces shared by the two mask tile kernels ------------------------------------------------------------------------------
// MixDesc n of the table a mixed launch passes as `bg` (kernels.hpp): ONE 16-byte uniform load; the background pointer is returned as a global-memory pointer (a
// pointer read from memory is otherwise a generic one, and the operand loads through it would be flat loads)
__device__ __forceinline__ const uint8_t* mix_desc(const uint8_t* table, int n, unsigned* flags) {
  const uint4 v = reinterpret_cast<const uint4*>(table)[n];
  *flags = v.z;
  return (const uint8_t*)(const __attribute__((address_space(1))) uint8_t*)(((uint64_t)v.y << 32) | v.x);
}
// Composite operands of a lane's kTileItems 4-pixel groups (12 B of background + 12 B of frame each), requested at the very
// top of the kernel so that their HBM latency hides behind the LDS phases.
struct TileBlendOperands { uint32_t a[kTileItems][3], b[kTileItems][3]; };
// `uniform` (wave-uniform): 0 = both operands; 1 = the tile's mask is 255 everywhere → only the background is needed; 2 = 0 everywhere → only the frame
// `parts` (wave-uniform): bit 0 = request the background operand, bit 1 = the frame operand — 3 = whatever `uniform` needs in one call; mask_tile_k requests a SHARED
// background before it knows the tile's class (parts = 1) and the frame after (parts = 2)
// `yin` (wave-uniform; BSX_STEP_YUYV_IN): `frames` holds YUYV 4:2:2 — a lane's four pixels are 8 bytes (b[i][0..1]), converted where they are consumed
// (tile_frame_bgr below); b[i][2] is then unused
// `sel` (wave-uniform, read only with SEL): which operand the composite is, when that is not what `uniform` says — 2 = the frame whatever the mask
// (bsx_step_batch_mixed: a stream with its filter switched off), -1 = as `uniform`.  A template parameter: the callers without it compile to what they were.
template <bool BLEND, bool WHOLE = false, bool SEL = false>      // WHOLE: every tile of the launch lies inside the ROI (roi.w % 128 == 0, roi.h % 32 == 0): no per-item edge tests
__device__ __forceinline__ void tile_load_blend_operands(TileBlendOperands& o, const uint8_t* __restrict__ bg, long bg_stride, const uint8_t* __restrict__ frames,
                                                         int n, int W, int H, Rect4 roi, int tx0, int ty0, int tid, int uniform = 0, int parts = 3, bool yin = false,
                                                         int sel = -1) {
  if constexpr (SEL) { if (sel >= 0) uniform = sel; }
  if constexpr (BLEND) {
    const int ly0 = tid / (kTW / 4), gx = tx0 + (tid % (kTW / 4)) * 4;
    const long pix0 = (long)(roi.y + ty0 + ly0) * W + roi.x + gx;        // frame coordinates of the ROI-relative tile pixel
    const int fb = yin ? 2 : 3;                                          // bytes per frame pixel
    const uint8_t* const a0 = bg + (bg_stride ? n * bg_stride : 0) + pix0 * 3;
    const uint8_t* const b0 = frames + ((long)n * W * H + pix0) * fb;
#pragma unroll
    for (int i = 0; i < kTileItems; i++) {
      if (parts & 1) o.a[i][0] = o.a[i][1] = o.a[i][2] = 0;
      if (parts & 2) o.b[i][0] = o.b[i][1] = o.b[i][2] = 0;
      if (WHOLE || (ty0 + ly0 + 8 * i < roi.h && gx < roi.w)) {
        const uint32_t* ap = reinterpret_cast<const uint32_t*>(a0 + (long)(8 * i) * W * 3);
        const uint32_t* bp = reinterpret_cast<const uint32_t*>(b0 + (long)(8 * i) * W * fb);
        if ((parts & 1) && uniform != 2) { o.a[i][0] = ap[0]; o.a[i][1] = ap[1]; o.a[i][2] = ap[2]; }
        if ((parts & 2) && uniform != 1) {                               // streamed once
          o.b[i][0] = __builtin_nontemporal_load(bp); o.b[i][1] = __builtin_nontemporal_load(bp + 1);
          if (!yin) o.b[i][2] = __builtin_nontemporal_load(bp + 2);
        }
      }
    }
  }
}
// the frame operand of item i as three BGR words, whatever form it was loaded in
__device__ __forceinline__ void tile_frame_bgr(const TileBlendOperands& o, int i, bool yin, uint32_t b3[3]) {
  if (yin) yuyv4_to_bgr3(o.b[i][0], o.b[i][1], b3);
  else { b3[0] = o.b[i][0]; b3[1] = o.b[i][1]; b3[2] = o.b[i][2]; }
}
// Step 3: vertical pass of cv::resize, 4 pixels per lane (64-bit LDS reads of the two source rows, one 32-bit write).
// row0 / row1: LDS tables of the two hq rows of every halo row; (y, xg) advance without a division.
template <typename RowT>
__device__ __forceinline__ void tile_vertical_pass(const uint16_t* hq, uint8_t* up, const RowT* row0, const RowT* row1, int row_bias, const short* row_b0,
                                                   const short* row_b1, int tid) {
  constexpr int kG = kHW / 4;
  for (int y = tid / kG, xg = tid % kG; y < kHH;) {
    const int x = xg * 4;
    const int b0 = row_b0[y], b1 = row_b1[y];                  // 16-bit coefficients: the products below are 24-bit multiplies
    const uint2 r0 = *reinterpret_cast<const uint2*>(&hq[((int)row0[y] - row_bias) * kHW + x]);
    const uint2 r1 = *reinterpret_cast<const uint2*>(&hq[((int)row1[y] - row_bias) * kHW + x]);
    const int h0[4] = {(int)(r0.x & 0xffff), (int)(r0.x >> 16), (int)(r0.y & 0xffff), (int)(r0.y >> 16)};
    const int h1[4] = {(int)(r1.x & 0xffff), (int)(r1.x >> 16), (int)(r1.y & 0xffff), (int)(r1.y >> 16)};
    uint32_t packed = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) packed |= (uint32_t)((((b0 * h0[j]) >> 16) + ((b1 * h1[j]) >> 16) + 2) >> 2) << (8 * j);
    *reinterpret_cast<uint32_t*>(&up[y * kHW + x]) = packed;
    xg += kThreads % kG; y += kThreads / kG;
    if (xg >= kG) { xg -= kG; y++; }
  }
}
// Step 4: horizontal 5-sums, 4 per lane: 8 consecutive bytes in, 4 u16 out.  v_sad_u8 against 0 adds the four bytes of a
// word (+ an accumulator) in one instruction; the sliding windows come from v_alignbyte.
__device__ __forceinline__ void tile_hsum5(const uint8_t* up, uint16_t* hs, int tid) {
  for (int k = tid; k < kHH * (kTW / 4); k += kThreads) {
    const int ly = k / (kTW / 4), lx = (k - ly * (kTW / 4)) * 4;
    const uint2 v = *reinterpret_cast<const uint2*>(&up[ly * kHW + lx]);            // bytes b0..b3 | b4..b7
    const uint32_t s0 = __builtin_amdgcn_sad_u8(v.x, 0u, v.y & 255u);                                                  // b0..b4
    const uint32_t s1 = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(v.y, v.x, 1), 0u, (v.y >> 8) & 255u);      // b1..b5
    const uint32_t s2 = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(v.y, v.x, 2), 0u, (v.y >> 16) & 255u);     // b2..b6
    const uint32_t s3 = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(v.y, v.x, 3), 0u, v.y >> 24);              // b3..b7
    *reinterpret_cast<uint2*>(&hs[ly * kTW + lx]) = make_uint2(s0 | (s1 << 16), s2 | (s3 << 16));
  }
}
// Step 5: vertical 5-sums (packed u16 adds: five sums <= 25*255 stay inside a u16 lane), (s + 12) / 25 as
// ((s + 12) * 5243) >> 17 (exhaustively checked for s <= 25*255), mask store, and with BLEND the composite of the same
// 4 pixels (W, roi.x and roi.w multiples of 4, checked by the launcher: 12 bytes = 3 aligned words per image).
// four packed BGR pixels (12 bytes in three words) in reverse pixel order: cv::flip(.., 1) of a 4-pixel group
__device__ __forceinline__ void reverse4px(uint32_t (&w)[3]) {
  const uint32_t n0 = (w[2] >> 8) | ((w[1] & 0x00FF0000u) << 8);
  const uint32_t n1 = (w[1] >> 24) | ((w[2] & 255u) << 8) | ((w[0] >> 24) << 16) | (w[1] << 24);
  const uint32_t n2 = ((w[1] >> 8) & 255u) | (w[0] << 8);
  w[0] = n0; w[1] = n1; w[2] = n2;
}
// flip (yuyv bits 1-2: 2 = horizontal, 4 = vertical): cv::flip of the COMPOSITE (deepseg.cc:667-673) folded into where the tile stores it — the lane's four
// pixels go to the mirrored column group in reverse order, the row to the mirrored row; the persistent mask is the unflipped frame's and stays put.
// `uniform` (wave-uniform; see mask_tile_k): 1 / 2 = every mask byte of the tile is 255 / 0 — no sums to form, and the composite IS the background / the frame
// ((a*255 + b*0)/255 == a for every byte: the exhaustive blend test covers m = 0 and 255)
// `sel` (SEL): which operand the composite is when that is not what `uniform` says (see tile_load_blend_operands) — the mask is still formed from `uniform`
template <bool BLEND, bool WHOLE = false, bool SEL = false>
__device__ __forceinline__ void tile_vsum5_store(const uint16_t* hs, uint8_t* __restrict__ mask, uint8_t* __restrict__ outp, const TileBlendOperands& o,
                                                 int n, int ms, int W, int H, Rect4 roi, int tx0, int ty0, int tid, int yuyv_flip, int uniform = 0, int sel = -1) {
  int take = uniform;                                            // the composite's operand: 0 = the blend, 1 = the background, 2 = the frame
  if constexpr (SEL) { if (sel >= 0) take = sel; }
  const int ly0 = tid / (kTW / 4), lx = (tid % (kTW / 4)) * 4;
  const int gx = tx0 + lx;
  const int yuyv = yuyv_flip & 1;
  const bool fh = (yuyv_flip & 2) != 0, fv = (yuyv_flip & 4) != 0, yin = (yuyv_flip & 16) != 0;      // bit 4 = BSX_STEP_YUYV_IN: the frame operand arrived as YUYV
  const int obpp = yuyv ? 2 : 3;                                 // composite written as packed BGR or as YUYV 4:2:2 (convert_rgb_to_yuyv fused in)
  uint8_t* const dst0 = mask + (long)ms * W * H + (long)(roi.y + ty0 + ly0) * W + roi.x + gx;      // ms: the frame's state slot (n: its position in the batch)
  const int oy0 = fv ? H - 1 - (roi.y + ty0 + ly0) : roi.y + ty0 + ly0, ox = fh ? W - 4 - (roi.x + gx) : roi.x + gx;
  const long orow = fv ? -(long)W : (long)W;                     // output row step per tile row
  uint8_t* const out0 = BLEND ? outp + ((long)n * W * H + (long)oy0 * W + ox) * obpp : nullptr;
#pragma unroll
  for (int i = 0; i < kTileItems; i++) {
    const int ly = ly0 + 8 * i, gy = ty0 + ly;
    if (!WHOLE && (gy >= roi.h || gx >= roi.w)) continue;
    uint32_t packed = uniform == 1 ? 0xFFFFFFFFu : 0u;
    if (!uniform) {
      uint2 acc = *reinterpret_cast<const uint2*>(&hs[ly * kTW + lx]);
#pragma unroll
      for (int r = 1; r < 5; r++) {
        const uint2 v = *reinterpret_cast<const uint2*>(&hs[(ly + r) * kTW + lx]);
        acc.x = __builtin_bit_cast(uint32_t, __builtin_bit_cast(us2, acc.x) + __builtin_bit_cast(us2, v.x));
        acc.y = __builtin_bit_cast(uint32_t, __builtin_bit_cast(us2, acc.y) + __builtin_bit_cast(us2, v.y));
      }
      const uint32_t m0 = (__umul24(acc.x & 0xffffu, 5243u) + 12u * 5243u) >> 17, m1 = (__umul24(acc.x >> 16, 5243u) + 12u * 5243u) >> 17;
      const uint32_t m2 = (__umul24(acc.y & 0xffffu, 5243u) + 12u * 5243u) >> 17, m3 = (__umul24(acc.y >> 16, 5243u) + 12u * 5243u) >> 17;
      packed = m0 | (m1 << 8) | (m2 << 16) | (m3 << 24);
    }
    uint8_t* dst = dst0 + (long)(8 * i) * W;
    if (BLEND && (yuyv_flip & 8)) { /* composite only (BSX_STEP_NO_MASK): the full-resolution mask stays in registers */ }
    else if (WHOLE || (gx + 3 < roi.w && ((uintptr_t)dst & 3) == 0)) *reinterpret_cast<uint32_t*>(dst) = packed;      // (nontemporal here: measured, no difference — profiles/r05d)
    else for (int j = 0; j < 4 && gx + j < roi.w; j++) dst[j] = (uint8_t)(packed >> (8 * j));
    if constexpr (BLEND) {
      uint32_t* op = reinterpret_cast<uint32_t*>(out0 + (long)(8 * i) * orow * obpp);
      uint32_t o3[3];
      if (take == 1) { o3[0] = o.a[i][0]; o3[1] = o.a[i][1]; o3[2] = o.a[i][2]; }
      else if (take == 2) tile_frame_bgr(o, i, yin, o3);
      else { uint32_t b3[3]; tile_frame_bgr(o, i, yin, b3); blend_quad(o.a[i], b3, packed, o3); }
      if (fh) reverse4px(o3);
      if (yuyv) {                                                  // deepseg.cc:87-106 on the four composited pixels: 8 bytes instead of 12
        __builtin_nontemporal_store(yuyv_pair(o3[0] & 255u, (o3[0] >> 8) & 255u, (o3[0] >> 16) & 255u, o3[0] >> 24, o3[1] & 255u, (o3[1] >> 8) & 255u), op);
        __builtin_nontemporal_store(yuyv_pair((o3[1] >> 16) & 255u, o3[1] >> 24, o3[2] & 255u, (o3[2] >> 8) & 255u, (o3[2] >> 16) & 255u, o3[2] >> 24), op + 1);
      } else {
        // ONE 12-byte store (global_store_dwordx3): the 32 lanes of a tile row then write 384 contiguous bytes per instruction — as three dword stores each
        // instruction wrote 4 of every 12 bytes (a third of every line, three times over)
        if (yuyv_flip & 128) *reinterpret_cast<u3v*>(op) = u3v{o3[0], o3[1], o3[2]};      // (debug build: plain instead of nontemporal stores, A/B — round 6)
        else __builtin_nontemporal_store(u3v{o3[0], o3[1], o3[2]}, reinterpret_cast<u3v*>(op));
      }
    }
  }
}

// MIX (bsx_step_batch_mixed): `bg` is the batch's MixDesc table (kernels.hpp) — the background, flip and filter-off bit of position n come from desc[n], one uniform
// load per workgroup; bg_stride is unused
template <bool BLEND, bool YIN = false, bool MIX = false>      // YIN (BSX_STEP_YUYV_IN): `frames` is YUYV 4:2:2 — a template parameter so that the BGR instantiation carries none of the conversion
__global__ __launch_bounds__(kThreads) void mask_upscale_blur_k(const uint8_t* __restrict__ ofinal, int outW, int outH, Rect4 q, ResizeTab tab,
                                                               uint8_t* __restrict__ mask, int W, int H, Rect4 roi,
                                                               const uint8_t* __restrict__ bg, long bg_stride, const uint8_t* __restrict__ frames,
                                                               uint8_t* __restrict__ outp, int yuyv, int ntx, int nty, int n_frames, const int* __restrict__ slot_of) {
  // coefficients are 0..2048: kept as 16-bit so that every product below is a full-rate 24-bit multiply
  __shared__ int col_sx[kHW], col_sx1[kHW], row_s0[kHH], row_s1[kHH];
  __shared__ short col_a0[kHW], col_a1[kHW], row_b0[kHH], row_b1[kHH];
  // hq (steps 2-3) and hs (steps 4-5) are never live together: one buffer, more workgroups per CU
  __shared__ __attribute__((aligned(16))) uint16_t hq_hs[kMaxSrcRows * kHW > kHH * kTW ? kMaxSrcRows * kHW : kHH * kTW];
  __shared__ __attribute__((aligned(16))) uint8_t up[kHH * kHW + 8];
  uint16_t* const hq = hq_hs;
  uint16_t* const hs = hq_hs;
  __shared__ int s_min, s_max;
  unsigned f_, t_;
  xcd_frame_tile((unsigned)(ntx * nty), (unsigned)n_frames, &f_, &t_);
  const int n = (int)f_, tby = (int)t_ / ntx, tbx = (int)t_ - tby * ntx;
  const int ms = slot_of ? slot_of[n] : n;                                   // the frame's state slot (ofinal, mask): one scalar load per workgroup
  const int tx0 = tbx * kTW, ty0 = tby * kTH;
  const uint8_t* src = ofinal + (long)ms * outW * outH + (long)q.y * outW + q.x;
  const int tid = threadIdx.x;
  TileBlendOperands ops;
  yuyv = YIN ? (yuyv | 16) : (yuyv & ~16);                                  // the helpers read bit 4: a compile-time constant per instantiation
  int sel = -1;                                                             // MIX: 2 = the filter is off, the composite is the frame
  if constexpr (MIX) {
    unsigned fl;
    bg = mix_desc(bg, n, &fl); bg_stride = 0;
    yuyv |= (int)(fl & (kMixFlipH | kMixFlipV));
    if (fl & kMixFilterOff) sel = 2;
  }
  tile_load_blend_operands<BLEND, false, MIX>(ops, bg, bg_stride, frames, n, W, H, roi, tx0, ty0, tid, 0, 3, YIN, sel);
  if (tid == 0) { s_min = 1 << 30; s_max = -1; }
  __syncthreads();
  // 1. column / row tables
  if (tid < kHW) {
    const int gx = reflect101(min(tx0 + tid - 2, roi.w + 1), roi.w);
    int sx, sx1, a0, a1;
    if (tab.mode == 1) { sx = sx1 = gx; a0 = 2048; a1 = 0; }
    else if (tab.mode == 2) { sx = 2 * gx; sx1 = 2 * gx + 1; a0 = a1 = 0; }
    else { sx = tab.xofs[gx]; sx1 = min(sx + 1, tab.sw - 1); a0 = tab.xa[2 * gx]; a1 = tab.xa[2 * gx + 1]; }
    col_sx[tid] = sx; col_sx1[tid] = sx1; col_a0[tid] = (short)a0; col_a1[tid] = (short)a1;
  } else if (tid >= 192 && tid < 192 + kHH) {
    const int r = tid - 192;
    const int gy = reflect101(min(ty0 + r - 2, roi.h + 1), roi.h);
    int s0, s1, b0, b1;
    if (tab.mode == 1) { s0 = s1 = gy; b0 = 2048; b1 = 0; }
    else if (tab.mode == 2) { s0 = 2 * gy; s1 = 2 * gy + 1; b0 = b1 = 0; }
    else { const int sy = tab.yofs[gy]; s0 = min(max(sy, 0), tab.sh - 1); s1 = min(max(sy + 1, 0), tab.sh - 1); b0 = tab.ya[2 * gy]; b1 = tab.ya[2 * gy + 1]; }
    row_s0[r] = s0; row_s1[r] = s1; row_b0[r] = (short)b0; row_b1[r] = (short)b1;
    atomicMin(&s_min, s0);
    atomicMax(&s_max, s1);
  }
  __syncthreads();
  const int smin = s_min, nsr = s_max - smin + 1;
  if (tab.mode == 0 && nsr <= kMaxSrcRows) {
    // 2. horizontal pass on the touched source rows.  A lane keeps ONE column (its table entries stay in registers) and
    //    walks the source rows — columns 0..127 two rows per pass, the four halo columns 128..131 by the first 4*nsr
    //    lanes.  No index division, 32-bit offsets from a uniform base, 24-bit multiplies.
    static_assert(kThreads == 2 * kTW && 4 * kMaxSrcRows <= kThreads, "lane mapping of step 2");
    {
      const uint8_t* const base = src + (long)smin * outW;
      const int x = tid & (kTW - 1), half = tid >> 7;
      const int a0 = col_a0[x], a1 = col_a1[x];
      unsigned o0 = (unsigned)(half * outW + col_sx[x]), o1 = (unsigned)(half * outW + col_sx1[x]);
      for (int r = half; r < nsr; r += 2, o0 += 2u * outW, o1 += 2u * outW)
        hq[r * kHW + x] = (uint16_t)((base[o0] * a0 + base[o1] * a1) >> 4);
      if (tid < 4 * nsr) {
        const int xr = kTW + (tid & 3), r = tid >> 2;
        hq[r * kHW + xr] = (uint16_t)((base[(unsigned)(r * outW + col_sx[xr])] * col_a0[xr] + base[(unsigned)(r * outW + col_sx1[xr])] * col_a1[xr]) >> 4);
      }
    }
    __syncthreads();
    tile_vertical_pass(hq, up, row_s0, row_s1, smin, row_b0, row_b1, tid);   // 3.
  } else {
    // copy / exact-2x area / very strong down-scale: direct per-pixel sample
    for (int k = tid; k < kHH * kHW; k += kThreads) {
      const int y = k / kHW, x = k - y * kHW;
      int v;
      if (tab.mode == 1) v = src[(long)row_s0[y] * outW + col_sx[x]];
      else if (tab.mode == 2) v = (src[(long)row_s0[y] * outW + col_sx[x]] + src[(long)row_s0[y] * outW + col_sx1[x]] + src[(long)row_s1[y] * outW + col_sx[x]] +
                                   src[(long)row_s1[y] * outW + col_sx1[x]] + 2) >> 2;
      else {
        const int h0 = src[(long)row_s0[y] * outW + col_sx[x]] * col_a0[x] + src[(long)row_s0[y] * outW + col_sx1[x]] * col_a1[x];
        const int h1 = src[(long)row_s1[y] * outW + col_sx[x]] * col_a0[x] + src[(long)row_s1[y] * outW + col_sx1[x]] * col_a1[x];
        v = (((row_b0[y] * (h0 >> 4)) >> 16) + ((row_b1[y] * (h1 >> 4)) >> 16) + 2) >> 2;
      }
      up[k] = (uint8_t)v;
    }
  }
  __syncthreads();
  tile_hsum5(up, hs, tid);                                                                       // 4.
  __syncthreads();
  tile_vsum5_store<BLEND, false, MIX>(hs, mask, outp, ops, n, ms, W, H, roi, tx0, ty0, tid, yuyv, 0, sel);   // 5.
}

// ---- mask tile, single-round-trip form ---------------------------------------------------------------------------------
// Same integers as mask_upscale_blur_k, restructured around what actually bounds it: with the composite fused in, a
// workgroup's life is a chain of dependent memory round trips taken while HBM is saturated by the blend traffic
// (loaded latency of several microseconds each).  Here every global load of the tile is issued in the first few
// instructions: the source-block extents come from four uniform (scalar) table reads, then the raw ofinal block, this
// lane's table entries and its composite operands are all requested back to back.  Steps 2-5 then run from LDS only.
// Used when the host verified that every tile's source block fits (ResizeTab::tile_ok); other cases take the kernel above.
constexpr int kSrcBlockBytes = kHH * kHW;        // the raw block lives in `up` until step 3 overwrites it
// a tile's class byte (tile_class_k), read through the aligned word that holds it: a SCALAR load (uniform address), not a vector load + readfirstlane
__device__ __forceinline__ int tile_class_byte(uintptr_t ca) { return (int)((*reinterpret_cast<const uint32_t*>(ca & ~(uintptr_t)3) >> (8 * (unsigned)(ca & 3))) & 255u); }
// F0: the launch has no flag set (no YUYV out, no flip, mask stored, default load order) — the default step.  A template parameter like YIN because this kernel pays
// for every wave-uniform branch it carries: with the YUYV-in conversion behind a run-time flag the BGR step's launch was 12-15 % slower (profiles/r06l: 105-111 ->
// 94-97 us at configs[1], 1064-1114 -> 946-955 us at the configs[4] slice), code that never ran.
// WH: whole tiles only (see tile_load_blend_operands) and a 4-byte aligned mask — decided by the launcher from the geometry
// MIX (bsx_step_batch_mixed): `bg` is the batch's MixDesc table, as in mask_upscale_blur_k — its uniform load goes out next to the tile-class byte's, and the flip
// and the filter-off bit become wave-uniform run-time branches (a mixed batch has no F0 / WH launch)
template <bool BLEND, bool YIN = false, bool F0 = false, bool WH = false, bool MIX = false>
__global__ __launch_bounds__(kThreads) void mask_tile_k(const uint8_t* __restrict__ ofinal, int outW, int outH, Rect4 q, ResizeTab tab,
                                                       uint8_t* __restrict__ mask, int W, int H, Rect4 roi,
                                                       const uint8_t* __restrict__ bg, long bg_stride, const uint8_t* __restrict__ frames,
                                                       uint8_t* __restrict__ outp, int yuyv, int ntx, int nty, int n_frames, int ty_base, int nty_all,
                                                       const int* __restrict__ slot_of) {
  // (ty_base, nty_all: this launch covers tile rows [ty_base, ty_base + nty) of the nty_all rows of a frame — the launcher cuts a frame whose last tile row is partial
  //  into the whole rows, run by the WH instantiation, and that last row)
  __shared__ short col_c0[kHW], col_c1[kHW], col_a0[kHW], col_a1[kHW];     // block-relative tap columns, coefficients
  __shared__ short row_r0[kHH], row_r1[kHH], row_b0[kHH], row_b1[kHH];     // block-relative tap rows, coefficients
  __shared__ __attribute__((aligned(16))) uint16_t hq_hs[kMaxSrcRows * kHW > kHH * kTW ? kMaxSrcRows * kHW : kHH * kTW];
  __shared__ __attribute__((aligned(16))) uint8_t up[kHH * kHW + 8];
  uint16_t* const hq = hq_hs;
  uint16_t* const hs = hq_hs;
  uint8_t* const blk = up;
  // XCD-aware order: a frame's tiles run on ONE XCD.  Where the ROI does not start on a 128-byte line (roi.x = 80 / 280: DeepLab, MLKit) the 384-byte row
  // segments of neighbouring tiles share cache lines — fetched once per L2 that touches them (PMC: 1.8x the frame bytes in the plain order).
  unsigned f_, t_;
  xcd_frame_tile((unsigned)(ntx * nty), (unsigned)n_frames, &f_, &t_);
  const int n = (int)f_, tid = threadIdx.x, tby0 = (int)t_ / ntx, tbx = (int)t_ - tby0 * ntx, tby = tby0 + ty_base;
  const int tx0 = tbx * kTW, ty0 = tby * kTH;
  // UNIFORM TILES (round 4).  In the steady state of the temporal filter the model-resolution mask is exactly 0x00 or 0xFF wherever the person's outline is not
  //     (lib/libbackscrub.cc:330-355: three equal decisions in a row), and a tile whose whole source block (taps of the halo included) holds one of those two values
  //     gets that value in every pixel: cv::resize of a constant is the constant ((b0 * 32640 >> 16) + (b1 * 32640 >> 16) + 2) >> 2 == 255 for every b0 + b1 == 2048,
  //     tests/test_oracle_image.py), and so is the box blur ((25 v + 12) / 25).  Such a tile skips steps 1-5, and its composite is a copy: of the background where the
  //     mask is 255 — the frame is not even read — and of the frame where it is 0.  tile_class_k (below) classified every tile of the launch a moment ago: one
  //     scalar load here, no vote, no barrier, nothing serialised in front of the operand loads (the first version voted inside this kernel: block load → ballot →
  //     barrier → operand loads cost the general path 6 %, profiles/r04e).  Bit-identical by construction; BSX_NO_UNIFORM_TILES=1 (read when the context is
  //     created) keeps every tile on the general path (A/B timing; the parity tests run both).
  int uniform = 0;
  // A SHARED background (bg_stride == 0: one image for all streams, L2-resident) is requested BEFORE the tile's class is known (round 5): the class byte is a second
  // dependent round trip behind the kernel arguments, and two thirds of the tiles (uniform 255: composite = background) then need nothing else.  A per-stream
  // background is HBM traffic a uniform-0 tile must not pay: it keeps the order class -> operands.
  if (F0) yuyv = 0;                                                                                 // flags as compile-time constants: F0 = none, YIN = bit 4 (read again by
  yuyv = YIN ? (yuyv | 16) : (yuyv & ~16);                                                          // tile_vsum5_store)
  const bool early_bg = BLEND && !MIX && bg_stride == 0 && tab.tile_class != nullptr && !(yuyv & 64);      // (bit 6: the debug build's A/B switch for this order)
  constexpr bool yin = YIN;                                                                         // BSX_STEP_YUYV_IN
  TileBlendOperands ops;
  if (early_bg) tile_load_blend_operands<BLEND, WH>(ops, bg, bg_stride, frames, n, W, H, roi, tx0, ty0, tid, 0, 1, yin);
  if (tab.tile_class) uniform = tile_class_byte((uintptr_t)tab.tile_class + (size_t)n * (size_t)(ntx * nty_all) + (size_t)(tby * ntx + tbx));
  int sel = -1;                                             // MIX: 2 = the filter is off — the mask is formed as always, the composite is the frame
  if constexpr (MIX) {
    unsigned fl;
    bg = mix_desc(bg, n, &fl); bg_stride = 0;
    yuyv |= (int)(fl & (kMixFlipH | kMixFlipV));
    if (fl & kMixFilterOff) sel = 2;
  }
  // The frame's state slot (ofinal, mask; n = its position: frames, output, tile classes): slot_of[n] — one scalar load — or n.  Formed only AFTER the class byte is
  // requested, on both paths: anything in front of that load lengthens the dependent chain every tile waits on (formed at the top, the dense step's launch measured
  // 78 -> 82 us at configs[1]).
  if (uniform) {                                           // wave-uniform: nothing of the general path below is even requested
    tile_load_blend_operands<BLEND, WH, MIX>(ops, bg, bg_stride, frames, n, W, H, roi, tx0, ty0, tid, uniform, early_bg ? 2 : 3, yin, sel);
    const int ms = slot_of ? slot_of[n] : n;
    tile_vsum5_store<BLEND, WH, MIX>(hq_hs, mask, outp, ops, n, ms, W, H, roi, tx0, ty0, tid, yuyv, uniform, sel);
    return;
  }
#define BSX_MT_FRAME n                                   /* the general path: steps (a)-(c) and 1-5, shared with mask_tile_geoms_k */
#define BSX_MT_SLOT (slot_of ? slot_of[n] : n)
#define BSX_MT_MASK_SLOT ms
#include "mask_tile.inc"
#undef BSX_MT_FRAME
#undef BSX_MT_SLOT
#undef BSX_MT_MASK_SLOT
}

// ---- alpha blend (deepseg.cc:108-134), stand-alone: bsx_composite_batch ---------------------------------------------------------------
// Every memory instruction COALESCED ACROSS LANES (round 4; the 16-consecutive-pixels-per-lane form it replaced — 16-byte accesses 48 bytes apart between
// neighbouring lanes, every line visited by three instructions — moved 4.8 TB/s and was deleted in round 6).  A lane owns kB4 groups of FOUR pixels, group j of lane l at group index (block * kB4 + j) * 256 + l: one wave instruction = 64 lanes x 12 contiguous bytes
// = 768 bytes = six whole lines (global_load_dwordx3 / global_store_dwordx3, 4-byte aligned), the mask 64 x 4 bytes = two lines.  tools/microbench_mix.hip: a
// plain streaming kernel with this mix and coalesced accesses moves 5.7-6.2 TB/s through HBM.
constexpr int kB4 = 4;
__global__ __launch_bounds__(kThreads) void blend4x4_k(const uint8_t* __restrict__ bg, long bg_stride, const uint8_t* __restrict__ fr,
                                                      const uint8_t* __restrict__ mask, uint8_t* __restrict__ out, unsigned quads_per_frame, long npix,
                                                      const int* __restrict__ slot_of) {
  const long n = blockIdx.y;
  const unsigned q0 = blockIdx.x * (kThreads * kB4) + threadIdx.x;      // first 4-pixel group of this lane
  const uint8_t* const a0 = bg + (bg_stride ? n * bg_stride : 0);
  const uint8_t* const b0 = fr + n * npix * 3;
  const uint8_t* const m0 = mask + (slot_of ? (long)slot_of[n] : n) * npix;      // the frame's persistent mask: state slot, one scalar load
  uint8_t* const o0 = out + n * npix * 3;
  u3v av[kB4], bv[kB4];
  uint32_t mw[kB4];
#pragma unroll
  for (int j = 0; j < kB4; j++) {
    const unsigned q = min(q0 + j * kThreads, quads_per_frame - 1);     // groups past the end re-read the last one (never stored)
    av[j] = *reinterpret_cast<const u3v*>(a0 + (size_t)q * 12);
    bv[j] = __builtin_nontemporal_load(reinterpret_cast<const u3v*>(b0 + (size_t)q * 12));
    mw[j] = *reinterpret_cast<const uint32_t*>(m0 + (size_t)q * 4);
  }
#pragma unroll
  for (int j = 0; j < kB4; j++) {
    const unsigned q = q0 + j * kThreads;
    const uint32_t a3[3] = {av[j].x, av[j].y, av[j].z}, b3[3] = {bv[j].x, bv[j].y, bv[j].z};
    uint32_t o3[3];
    blend_quad(a3, b3, mw[j], o3);
    if (q < quads_per_frame) __builtin_nontemporal_store(u3v{o3[0], o3[1], o3[2]}, reinterpret_cast<u3v*>(o0 + (size_t)q * 12));
  }
}

// scalar tail / unaligned fallback: one pixel per lane
__global__ __launch_bounds__(kThreads) void blend1_k(const uint8_t* __restrict__ bg, long bg_stride, const uint8_t* __restrict__ fr,
                                                    const uint8_t* __restrict__ mask, uint8_t* __restrict__ out, long npix, const int* __restrict__ slot_of) {
  const long p = (long)blockIdx.x * kThreads + threadIdx.x;
  if (p >= npix) return;
  const long n = blockIdx.y;
  int m = mask[(slot_of ? (long)slot_of[n] : n) * npix + p];
  const uint8_t* a = bg + (bg_stride ? n * bg_stride : 0) + p * 3;
  const uint8_t* b = fr + (n * npix + p) * 3;
  uint8_t* o = out + (n * npix + p) * 3;
#pragma unroll
  for (int c = 0; c < 3; c++) o[c] = (uint8_t)((a[c] * m + b[c] * (255 - m)) / 255);
}

// composite outside the ROI = background: copies of the rows above / below the ROI and of the row segments left / right of it (W and roi.x, roi.w multiples of 4 →
// every segment boundary is word aligned).  Lane = FOUR consecutive outside words of frame blockIdx.y (round 4: one word per lane — a division and a 4-byte access per lane —
// ran this pure copy at 2.8 TB/s of writes, 110 us per 256 HD frames with the MLKit ROI): where the four words are adjacent in memory (always, except across a strip or ROI
// boundary) they move as one 16-byte access, otherwise word by word.
__device__ __forceinline__ long outside_word_offset(unsigned i, unsigned wpr, unsigned lw, unsigned rw0, unsigned sw, unsigned full, int W, Rect4 roi) {
  unsigned row, word;
  if (i < full) {
    const unsigned r = i / wpr;
    word = i - r * wpr;
    row = r < (unsigned)roi.y ? r : r + (unsigned)roi.h;
  } else {
    const unsigned j = i - full, r = j / sw, k = j - r * sw;
    row = (unsigned)roi.y + r;
    word = k < lw ? k : rw0 + (k - lw);
  }
  return ((long)row * W) * 3 + (long)word * 4;
}
__global__ __launch_bounds__(kThreads) void outside_roi_copy_k(const uint8_t* __restrict__ bg, long bg_stride, uint8_t* __restrict__ out, int W, int H, Rect4 roi) {
  const unsigned wpr = (unsigned)W * 3 / 4;                                   // words per row
  const unsigned lw = (unsigned)roi.x * 3 / 4, rw0 = (unsigned)(roi.x + roi.w) * 3 / 4, sw = lw + (wpr - rw0);   // strip words per ROI row
  const unsigned full = (unsigned)(H - roi.h) * wpr;                           // words of the rows entirely outside
  const unsigned total = full + (unsigned)roi.h * sw;
  const unsigned i = (blockIdx.x * kThreads + threadIdx.x) * 4u;
  if (i >= total) return;
  const long n = blockIdx.y;
  const uint8_t* src = bg + (bg_stride ? n * bg_stride : 0);
  uint8_t* dst = out + n * (long)W * H * 3;
  const long o0 = outside_word_offset(i, wpr, lw, rw0, sw, full, W, roi);
  if (i + 3 < total && outside_word_offset(i + 3, wpr, lw, rw0, sw, full, W, roi) == o0 + 12) {
    struct __attribute__((packed, aligned(4))) W4 { uint32_t v[4]; };          // 4-byte aligned 16-byte access (a strip need not start on a 16-byte boundary)
    *reinterpret_cast<W4*>(dst + o0) = *reinterpret_cast<const W4*>(src + o0);
    return;
  }
  for (unsigned k = 0; k < 4 && i + k < total; k++) {
    const long o = k ? outside_word_offset(i + k, wpr, lw, rw0, sw, full, W, roi) : o0;
    *reinterpret_cast<uint32_t*>(dst + o) = *reinterpret_cast<const uint32_t*>(src + o);
  }
}

// ---- generic BGR resize -------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void resize_bgr_k(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, ResizeTab tab) {
  const unsigned p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= (unsigned)(tab.dw * tab.dh)) return;
  const int y = (int)(p / (unsigned)tab.dw), x = (int)(p - (unsigned)y * (unsigned)tab.dw);
  const long n = blockIdx.y;
  int v[3];
  sample_linear<3>(src + n * (long)tab.sw * tab.sh * 3, (long)tab.sw * 3, tab, x, y, v);
  uint8_t* o = dst + (n * (long)tab.dw * tab.dh + p) * 3;
  o[0] = (uint8_t)v[0]; o[1] = (uint8_t)v[1]; o[2] = (uint8_t)v[2];
}

// ---- n BGR resizes of one output size in ONE launch (bsx_resize_bgr_batch / bsx_background_grab_batch) ------------------------------------------
// Block row blockIdx.y reads descriptor blockIdx.y: its own source (of its own size, so the three table modes can meet in one launch), its own destination.
// The index is the block's, so the descriptor arrives through uniform (scalar) loads; its pointers are rebuilt as global-memory pointers (mix_desc: a pointer
// read from memory is otherwise a generic one and everything through it a flat access).  A lane makes FOUR adjacent pixels of one output row — sample_linear,
// the integers of resize_bgr_k — and stores them as three dwords when the row is whole groups and that destination is 4-byte aligned (group g of an image lies
// at byte 12 g); any other destination takes byte stores, twelve partial writes where the other form has three full ones.  Same bytes either way.
template <typename T>
__device__ __forceinline__ T* as_global(T* p) { return (T*)(__attribute__((address_space(1))) T*)(uint64_t)p; }

__global__ __launch_bounds__(kThreads) void resize_bgr_batch_k(const ResizeBatchDesc* __restrict__ desc, int dw, int dh) {
  const unsigned gpr = ((unsigned)dw + 3u) / 4u, g = blockIdx.x * kThreads + threadIdx.x;
  if (g >= gpr * (unsigned)dh) return;
  const ResizeBatchDesc d = desc[blockIdx.y];
  ResizeTab tab;
  tab.xofs = as_global(d.xofs); tab.xa = as_global(d.xa); tab.yofs = as_global(d.yofs); tab.ya = as_global(d.ya);
  tab.sw = d.sw; tab.sh = d.sh; tab.dw = dw; tab.dh = dh; tab.mode = d.mode;
  const uint8_t* const src = as_global(d.src);
  uint8_t* const dst = as_global(d.dst);
  const int y = (int)(g / gpr), x = (int)(g - (unsigned)y * gpr) * 4;
  uint8_t* const o = dst + ((long)y * dw + x) * 3;
  if ((dw & 3) == 0 && ((uintptr_t)dst & 3) == 0) {                 // (uniform: the launch's width, the descriptor's pointer)
    int v[12];
#pragma unroll
    for (int k = 0; k < 4; k++) sample_linear<3>(src, (long)tab.sw * 3, tab, x + k, y, v + 3 * k);
    uint32_t w[3];
#pragma unroll
    for (int j = 0; j < 3; j++) w[j] = (uint32_t)v[4 * j] | ((uint32_t)v[4 * j + 1] << 8) | ((uint32_t)v[4 * j + 2] << 16) | ((uint32_t)v[4 * j + 3] << 24);
    uint32_t* const ow = reinterpret_cast<uint32_t*>(o);
    ow[0] = w[0]; ow[1] = w[1]; ow[2] = w[2];
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if (x + k >= dw) break;
    int v[3];
    sample_linear<3>(src, (long)tab.sw * 3, tab, x + k, y, v);
    o[3 * k] = (uint8_t)v[0]; o[3 * k + 1] = (uint8_t)v[1]; o[3 * k + 2] = (uint8_t)v[2];
  }
}

__global__ __launch_bounds__(kThreads) void yuyv_k(const uint8_t* __restrict__ in, uint32_t* __restrict__ out, long pairs) {
  long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= pairs) return;
  const uint8_t* p = in + i * 6;
  out[i] = yuyv_pair(p[0], p[1], p[2], p[3], p[4], p[5]);
}
// composite outside the ROI in YUYV form = the background converted: lane = one pixel pair of the frame, pairs inside the ROI belong to the tiles
// outside the ROI when the composite is flipped: one lane per group of four pixels of the frame (the ROI's groups return at once); BGR or YUYV out
__global__ __launch_bounds__(kThreads) void outside_roi_flip_k(const uint8_t* __restrict__ bg, long bg_stride, uint8_t* __restrict__ out, int W, int H, Rect4 roi, int yuyv_flip) {
  const unsigned i = blockIdx.x * kThreads + threadIdx.x, gpr = (unsigned)W / 4;
  if (i >= gpr * (unsigned)H) return;
  const int row = (int)(i / gpr), x = (int)(i - (unsigned)row * gpr) * 4;
  if (row >= roi.y && row < roi.y + roi.h && x >= roi.x && x < roi.x + roi.w) return;
  const long n = blockIdx.y;
  const uint32_t* p = reinterpret_cast<const uint32_t*>(bg + (bg_stride ? n * bg_stride : 0) + ((long)row * W + x) * 3);
  uint32_t w[3] = {p[0], p[1], p[2]};
  const bool fh = (yuyv_flip & 2) != 0, fv = (yuyv_flip & 4) != 0;
  if (fh) reverse4px(w);
  const int oy = fv ? H - 1 - row : row, ox = fh ? W - 4 - x : x;
  if (yuyv_flip & 1) {
    uint32_t* o = reinterpret_cast<uint32_t*>(out + (n * (long)W * H + (long)oy * W + ox) * 2);
    o[0] = yuyv_pair(w[0] & 255u, (w[0] >> 8) & 255u, (w[0] >> 16) & 255u, w[0] >> 24, w[1] & 255u, (w[1] >> 8) & 255u);
    o[1] = yuyv_pair((w[1] >> 16) & 255u, w[1] >> 24, w[2] & 255u, (w[2] >> 8) & 255u, (w[2] >> 16) & 255u, w[2] >> 24);
  } else {
    uint32_t* o = reinterpret_cast<uint32_t*>(out + (n * (long)W * H + (long)oy * W + ox) * 3);
    o[0] = w[0]; o[1] = w[1]; o[2] = w[2];
  }
}
__global__ __launch_bounds__(kThreads) void outside_roi_yuyv_k(const uint8_t* __restrict__ bg, long bg_stride, uint32_t* __restrict__ out, int W, int H, Rect4 roi) {
  const unsigned i = blockIdx.x * kThreads + threadIdx.x, ppr = (unsigned)W / 2;
  if (i >= ppr * (unsigned)H) return;
  const unsigned row = i / ppr, x = (i - row * ppr) * 2;
  if ((int)row >= roi.y && (int)row < roi.y + roi.h && (int)x >= roi.x && (int)x < roi.x + roi.w) return;
  const long n = blockIdx.y;
  const uint8_t* p = bg + (bg_stride ? n * bg_stride : 0) + ((long)row * W + x) * 3;
  out[n * (long)(W / 2) * H + i] = yuyv_pair(p[0], p[1], p[2], p[3], p[4], p[5]);
}
// outside the ROI in a mixed batch (bsx_step_batch_mixed): per position its own background and flip from desc[n] (one uniform load), or with the filter off its
// own frame — converted on load when the batch's frames are YUYV (flags bit 4); BGR or YUYV out (bit 0).  One lane per group of four pixels, as outside_roi_flip_k.
__global__ __launch_bounds__(kThreads) void outside_roi_mixed_k(const MixDesc* __restrict__ desc, const uint8_t* __restrict__ frames, uint8_t* __restrict__ out, int W,
                                                               int H, Rect4 roi, int flags) {
  const unsigned i = blockIdx.x * kThreads + threadIdx.x, gpr = (unsigned)W / 4;
  if (i >= gpr * (unsigned)H) return;
  const int row = (int)(i / gpr), x = (int)(i - (unsigned)row * gpr) * 4;
  if (row >= roi.y && row < roi.y + roi.h && x >= roi.x && x < roi.x + roi.w) return;
  const long n = blockIdx.y;
  unsigned fl;
  const uint8_t* const bgp = mix_desc(reinterpret_cast<const uint8_t*>(desc), (int)n, &fl);
  const long px = (long)row * W + x;
  uint32_t w[3];
  if (!(fl & kMixFilterOff)) {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(bgp + px * 3);
    w[0] = p[0]; w[1] = p[1]; w[2] = p[2];
  } else if (flags & 16) {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(frames + (n * (long)W * H + px) * 2);
    yuyv4_to_bgr3(p[0], p[1], w);
  } else {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(frames + (n * (long)W * H + px) * 3);
    w[0] = p[0]; w[1] = p[1]; w[2] = p[2];
  }
  const bool fh = (fl & kMixFlipH) != 0, fv = (fl & kMixFlipV) != 0;
  if (fh) reverse4px(w);
  const int oy = fv ? H - 1 - row : row, ox = fh ? W - 4 - x : x;
  if (flags & 1) {
    uint32_t* o = reinterpret_cast<uint32_t*>(out + (n * (long)W * H + (long)oy * W + ox) * 2);
    o[0] = yuyv_pair(w[0] & 255u, (w[0] >> 8) & 255u, (w[0] >> 16) & 255u, w[0] >> 24, w[1] & 255u, (w[1] >> 8) & 255u);
    o[1] = yuyv_pair((w[1] >> 16) & 255u, w[1] >> 24, w[2] & 255u, (w[2] >> 8) & 255u, (w[2] >> 16) & 255u, w[2] >> 24);
  } else {
    uint32_t* o = reinterpret_cast<uint32_t*>(out + (n * (long)W * H + (long)oy * W + ox) * 3);
    o[0] = w[0]; o[1] = w[1]; o[2] = w[2];
  }
}

// the same for ONE position given by its own pointers (bsx_step_batch_geoms: outside_roi_geoms_k below) — the statements of outside_roi_mixed_k for group i of
// the frame: bgp / fl = the position's descriptor, frame / out = ITS images.  (A function of its own and not the kernel's body: called from outside_roi_mixed_k
// it changed that kernel's code.)  EDGE (outside_roi_geoms_edge_k: roi.x and roi.w off the 4-pixel grid): a group that straddles a ROI bound belongs to the tile
// launch — only groups WHOLLY outside the ROI are written here.
template <bool EDGE = false>
__device__ __forceinline__ void outside_mixed_group(unsigned i, const uint8_t* __restrict__ bgp, unsigned fl, const uint8_t* __restrict__ frame, uint8_t* __restrict__ out,
                                                    int W, int H, Rect4 roi, int flags) {
  const unsigned gpr = (unsigned)W / 4;
  if (i >= gpr * (unsigned)H) return;
  const int row = (int)(i / gpr), x = (int)(i - (unsigned)row * gpr) * 4;
  if (row >= roi.y && row < roi.y + roi.h && x + (EDGE ? 3 : 0) >= roi.x && x < roi.x + roi.w) return;
  const long px = (long)row * W + x;
  uint32_t w[3];
  if (!(fl & kMixFilterOff)) {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(bgp + px * 3);
    w[0] = p[0]; w[1] = p[1]; w[2] = p[2];
  } else if (flags & 16) {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(frame + px * 2);
    yuyv4_to_bgr3(p[0], p[1], w);
  } else {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(frame + px * 3);
    w[0] = p[0]; w[1] = p[1]; w[2] = p[2];
  }
  const bool fh = (fl & kMixFlipH) != 0, fv = (fl & kMixFlipV) != 0;
  if (fh) reverse4px(w);
  const int oy = fv ? H - 1 - row : row, ox = fh ? W - 4 - x : x;
  if (flags & 1) {
    uint32_t* o = reinterpret_cast<uint32_t*>(out + ((long)oy * W + ox) * 2);
    o[0] = yuyv_pair(w[0] & 255u, (w[0] >> 8) & 255u, (w[0] >> 16) & 255u, w[0] >> 24, w[1] & 255u, (w[1] >> 8) & 255u);
    o[1] = yuyv_pair((w[1] >> 16) & 255u, w[1] >> 24, w[2] & 255u, (w[2] >> 8) & 255u, (w[2] >> 16) & 255u, w[2] >> 24);
  } else {
    uint32_t* o = reinterpret_cast<uint32_t*>(out + ((long)oy * W + ox) * 3);
    o[0] = w[0]; o[1] = w[1]; o[2] = w[2];
  }
}
// ---- YUYV → BGR ingest (cv::COLOR_YUV2BGR_YUYV, BT.601 limited range, 20-bit fixed point) --------------------------------
__global__ __launch_bounds__(kThreads) void yuyv_to_bgr_k(const uint32_t* __restrict__ in, uint8_t* __restrict__ out, long pairs) {
  long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= pairs) return;
  const int SH = 20, CY = 1220542, CUB = 2116026, CUG = -409993, CVG = -852492, CVR = 1673527;
  const uint32_t p = in[i];                       // Y0 | U<<8 | Y1<<16 | V<<24
  const int y0 = p & 255, u = (int)((p >> 8) & 255) - 128, y1 = (p >> 16) & 255, v = (int)(p >> 24) - 128;
  const int ruv = (1 << (SH - 1)) + CVR * v, guv = (1 << (SH - 1)) + CVG * v + CUG * u, buv = (1 << (SH - 1)) + CUB * u;
  const int ya = max(0, y0 - 16) * CY, yb = max(0, y1 - 16) * CY;
  uint8_t* o = out + 6 * i;
  o[0] = (uint8_t)min(max((ya + buv) >> SH, 0), 255); o[1] = (uint8_t)min(max((ya + guv) >> SH, 0), 255); o[2] = (uint8_t)min(max((ya + ruv) >> SH, 0), 255);
  o[3] = (uint8_t)min(max((yb + buv) >> SH, 0), 255); o[4] = (uint8_t)min(max((yb + guv) >> SH, 0), 255); o[5] = (uint8_t)min(max((yb + ruv) >> SH, 0), 255);
}

// ---- cv::flip on packed BGR (deepseg.cc:667-673): code 0 = around the x axis (rows reversed), > 0 = around the y axis
// (columns reversed), < 0 = both.  Out of place; lane = one pixel of frame blockIdx.y.
__global__ __launch_bounds__(kThreads) void flip_bgr_k(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int w, int h, int code) {
  const unsigned p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= (unsigned)(w * h)) return;
  const int y = (int)(p / (unsigned)w), x = (int)(p - (unsigned)y * (unsigned)w);
  const int sy = code <= 0 ? h - 1 - y : y, sx = code != 0 ? w - 1 - x : x;
  const long base = (long)blockIdx.y * w * h * 3;
  const uint8_t* s = src + base + ((long)sy * w + sx) * 3;
  uint8_t* d = dst + base + (long)p * 3;
  d[0] = s[0]; d[1] = s[1]; d[2] = s[2];
}

__global__ __launch_bounds__(kThreads) void fill_k(uint4* p, uint4 v, long n16) {
  long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i < n16) p[i] = v;
}

// ---- composite at the virtual camera's geometry (bsx_step_batch_vcam): blend → flip → cv::resize(INTER_LINEAR) → [YUYV pack], deepseg.cc:634-681 ---------
// The persistent mask holds every pixel (255 outside the ROI), so the composite at any source pixel is a pointwise function of frame, background and mask: the
// resampling kernel forms its own taps, and neither the capture-size composite nor the full-size resized image exists in memory.  One workgroup per kVW x kVH
// output tile, two 4-pixel groups per lane:
//   LDS form (DIRECT = false): the composite of the tile's source footprint — in the UNFLIPPED frame's coordinates, widened to whole 4-pixel groups — is staged in
//     LDS as one word per pixel (B | G << 8 | R << 16), each source pixel blended once whatever the scale; every output pixel then reads its four taps there.
//   DIRECT form: tables whose footprints do not fit kVLdsWords (strong down-scales; decided once per table on the host, vcam_tile_fits) blend each tap where it
//     is read.
// The resample is sample_linear's fixed point.  The 2x2 area mode (both scales exactly 2) arrives as a linear table with xofs = 2 dx, yofs = 2 dy and coefficients
// 1024 / 1024, whose integers ARE the area mean: (1024 * (((s0 + s1) * 1024) >> 4)) >> 16 == s0 + s1, then (.. + .. + 2) >> 2.  A flip is evaluated in the flipped
// frame's coordinates: output column dx takes taps x0 = xofs[dx] and x1 = min(x0 + 1, W - 1) of the flipped image, i.e. columns W-1-x0 and W-1-x1 of the composite
// (rows likewise, clamped before mirroring) — resize(flip(C)) and flip(resize(C)) differ at ratios such as 640 -> 426.
constexpr int kVW = 64, kVH = 32, kVLdsWords = 8192;                 // output tile; LDS staging area: 32 KiB = 8192 source pixels
static_assert(kVW * kVH == 2 * 4 * kThreads, "vcam tile: two 4-pixel groups per lane");
constexpr int kVcYuyvOut = 1, kVcFlipH = 2, kVcFlipV = 4, kVcWords = 8, kVcOutWords = 16;      // bits of the kernel's `opt` word
struct __attribute__((packed, aligned(4))) VcW2 { uint32_t x, y; };

// the frame's pixel (cx, cy), p = cy * W + cx, as B | G << 8 | R << 16: byte loads (YIN: U / V from the macropixel of column cx & ~1, yuyv_to_bgr_k's integers)
template <bool YIN>
__device__ __forceinline__ uint32_t vcam_frame_px(const uint8_t* __restrict__ fr, int W, int cx, int cy, long p) {
  if constexpr (YIN) {
    const uint8_t* q = fr + ((long)cy * W + (cx & ~1)) * 2;
    return yuv_tap_to_bgr((uint32_t)q[(cx & 1) * 2] | ((uint32_t)q[1] << 8) | ((uint32_t)q[3] << 16));
  } else {
    const uint8_t* b = fr + p * 3;
    return (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16);
  }
}
// composite of ONE pixel (cx, cy) as B | G << 8 | R << 16: byte loads, any geometry.
// SEL (the per-stream form, vg_mixed_k): with `off` (workgroup-uniform: the stream's filter is switched off) the composite IS the frame pixel — neither the
// background nor the mask is read.  A template parameter: the dense kernel compiles to what it was.
template <bool YIN, bool SEL = false>
__device__ __forceinline__ uint32_t vcam_px(const uint8_t* __restrict__ fr, const uint8_t* __restrict__ bgp, const uint8_t* __restrict__ mk, int W, int cx, int cy,
                                            bool off = false) {
  const long p = (long)cy * W + cx;
  if constexpr (SEL) {               // the frame's load goes out first, whatever the switch says: the background's and the mask's then join it in flight
    const uint32_t fw = vcam_frame_px<YIN>(fr, W, cx, cy, p);
    if (off) return fw & 0xffffffu;
    const uint8_t* a = bgp + p * 3;
    const uint32_t m = (uint32_t)mk[p] * 0x00010001u;
    return blend_word((uint32_t)a[0] | ((uint32_t)a[1] << 8) | ((uint32_t)a[2] << 16), fw, m, m);
  }
  const uint8_t* a = bgp + p * 3;
  const uint32_t aw = (uint32_t)a[0] | ((uint32_t)a[1] << 8) | ((uint32_t)a[2] << 16);
  const uint32_t bw = vcam_frame_px<YIN>(fr, W, cx, cy, p);
  const uint32_t m = (uint32_t)mk[p] * 0x00010001u;
  return blend_word(aw, bw, m, m);                                   // byte 3: 0 blended with 0
}
// the frame's 4-pixel group at p (12 B, YIN: 8 B) as three BGR words, and three such words as four pixel words
template <bool YIN>
__device__ __forceinline__ void vcam_frame_quad(const uint8_t* __restrict__ fr, long p, uint32_t b3[3]) {
  if constexpr (YIN) {
    const VcW2 y = *reinterpret_cast<const VcW2*>(fr + p * 2);
    yuyv4_to_bgr3(y.x, y.y, b3);
  } else {
    const u3v bv = *reinterpret_cast<const u3v*>(fr + p * 3);
    b3[0] = bv.x; b3[1] = bv.y; b3[2] = bv.z;
  }
}
__device__ __forceinline__ void vcam_quad_words(const uint32_t o[3], uint32_t w[4]) {
  w[0] = o[0] & 0xffffffu;
  w[1] = (o[0] >> 24) | ((o[1] & 0xffffu) << 8);
  w[2] = (o[1] >> 16) | ((o[2] & 0xffu) << 16);
  w[3] = o[2] >> 8;
}
// composite of the 4-pixel group (cx .. cx + 3, cy) as four pixel words.  words: W % 4 == 0 and 4-byte aligned images (cx % 4 == 0 here) — 12 B of background,
// 12 B (YIN: 8 B) of frame and 4 mask bytes, blend_quad; else pixel by pixel, columns past the row's end left 0 (no tap reads them: x1 <= W - 1).  SEL / off: as vcam_px
template <bool YIN, bool SEL = false>
__device__ __forceinline__ void vcam_group(const uint8_t* __restrict__ fr, const uint8_t* __restrict__ bgp, const uint8_t* __restrict__ mk, int W, int cx, int cy,
                                           bool words, uint32_t w[4], bool off = false) {
  if (words) {
    const long p = (long)cy * W + cx;
    if constexpr (SEL) {             // (the frame's load first, as in vcam_px)
      uint32_t f3[3], o[3];
      vcam_frame_quad<YIN>(fr, p, f3);
      if (off) { vcam_quad_words(f3, w); return; }
      const u3v av = *reinterpret_cast<const u3v*>(bgp + p * 3);
      const uint32_t a3[3] = {av.x, av.y, av.z};
      blend_quad(a3, f3, *reinterpret_cast<const uint32_t*>(mk + p), o);
      vcam_quad_words(o, w);
      return;
    }
    const u3v av = *reinterpret_cast<const u3v*>(bgp + p * 3);
    uint32_t b3[3];
    vcam_frame_quad<YIN>(fr, p, b3);
    const uint32_t a3[3] = {av.x, av.y, av.z};
    uint32_t o[3];
    blend_quad(a3, b3, *reinterpret_cast<const uint32_t*>(mk + p), o);
    vcam_quad_words(o, w);
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; k++) w[k] = cx + k < W ? vcam_px<YIN, SEL>(fr, bgp, mk, W, cx + k, cy, off) : 0u;
}
// one output channel from the four tap words: sample_linear's horizontal pass (11-bit coefficients) and vertical pass
__device__ __forceinline__ uint32_t vcam_lerp(uint32_t t00, uint32_t t01, uint32_t t10, uint32_t t11, int a0, int a1, int b0, int b1, int sh) {
  const int h0 = (int)((t00 >> sh) & 255u) * a0 + (int)((t01 >> sh) & 255u) * a1;
  const int h1 = (int)((t10 >> sh) & 255u) * a0 + (int)((t11 >> sh) & 255u) * a1;
  return (uint32_t)((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2) & 255u;
}
// (the body: vcam_tile.inc)
template <bool DIRECT, bool YIN>
__global__ __launch_bounds__(kThreads) void vcam_blend_resize_k(const uint8_t* __restrict__ frames, const uint8_t* __restrict__ bg, long bg_stride,
                                                               const uint8_t* __restrict__ masks, uint8_t* __restrict__ out, int W, int H, ResizeTab tab, int ntx,
                                                               int opt) {
  constexpr bool SEL = false;
  [[maybe_unused]] const int* const slot_of = nullptr;
#define BSX_VT_TILE blockIdx.x                           /* grid: output tiles x positions */
#define BSX_VT_POS blockIdx.y
#define BSX_VT_DESC(fl) bg = mix_desc(bg, (int)n, &fl); bg_stride = 0
#include "vcam_tile.inc"
}
// The per-stream form (bsx_step_batch_vcam_mixed): every position with its own background, flip bits and filter switch (desc[n]) and the mask of its own slot —
// the same body with SEL.  A kernel of its own, not a further parameter of the dense one, whose instantiations stay the four they were.
static_assert(kVcFlipH == (int)kMixFlipH && kVcFlipV == (int)kMixFlipV, "a descriptor's flip bits are the opt word's");
template <bool DIRECT, bool YIN>
__global__ __launch_bounds__(kThreads) void vg_mixed_k(const uint8_t* __restrict__ frames, const MixDesc* __restrict__ desc, const uint8_t* __restrict__ masks,
                                                      const int* __restrict__ slot_of, uint8_t* __restrict__ out, int W, int H, ResizeTab tab, int ntx, int opt) {
  constexpr bool SEL = true;
  const uint8_t* bg = reinterpret_cast<const uint8_t*>(desc);
  long bg_stride = 0;
#include "vcam_tile.inc"
}
#undef BSX_VT_TILE
#undef BSX_VT_POS
#undef BSX_VT_DESC

}  // namespace

// ---- the launch rule shared by the launchers below (kernels.hpp) ----
int xcd_tiles_mode() {
  static const int mode = dbg_env_int(BSX_DBG_ENV("BSX_XCD_TILES"), 1);
  return mode;
}

MaskTileGrid mask_tile_grid(int W, const Rect4& roi, int n) {
  MaskTileGrid g;
  g.ntx = (roi.w + kTW - 1) / kTW; g.nty = (roi.h + kTH - 1) / kTH;
  g.ok = (unsigned long long)g.ntx * g.nty * (unsigned long long)n < (1ull << 31);
  // one-XCD-per-frame order only where neighbouring tiles SHARE cache lines, i.e. the ROI's rows do not start on a 128-byte line (roi.x = 80 / 280: measured
  // mask+blend 0.480 -> 0.464 ms at 256 HD MLKit streams); on line-aligned geometries nothing is shared and the plain order measured 2-3 % faster (profiles/r03o)
  const bool shared_lines = ((roi.x * 3) & 127) != 0 || ((W * 3) & 127) != 0;
  g.nf = shared_lines ? xcd_frames(n) : 0;
  return g;
}

// the debug build's A/B switches of the tile kernels as bits of their flag word (each launcher applies the bits its kernels read): bit 6 (BSX_NO_EARLY_BG) = request a
// shared background only after the tile's class is known (rounds 1-4), bit 7 (BSX_TILE_PLAIN_STORES) = the composite leaves with plain instead of nontemporal stores
static int tile_debug_bits() {
  static const int bits = (BSX_DBG_ENV("BSX_NO_EARLY_BG") ? 64 : 0) | (BSX_DBG_ENV("BSX_TILE_PLAIN_STORES") ? 128 : 0);
  return bits;
}

// resize + bilateral in one launch (prep_fused_k); input (f32 [n][inH][inW][3]) and / or input_u8 (R|G<<8|B<<16 [n][inH][inW]): whichever is non-null is written
bool prep_yuyv_fusable(int W, Rect4 roi, const ResizeTab& tab) {      // the YIN form of prep_fused_k: INTER_LINEAR proper, whole macropixels, an 8-byte window inside the row
  return tab.mode == 0 && (W & 1) == 0 && (roi.x & 1) == 0 && (W - roi.x) * 2 >= 8;
}

hipError_t launch_prep_fused(const uint8_t* frames, int W, int H, Rect4 roi, float* input, uint32_t* input_u8, int inW, int inH, Rect4 in_roi, ResizeTab tab,
                             BilateralParams bp, int n, hipStream_t s, bool yuyv_in) {
  if (!input && !input_u8) return hipErrorInvalidValue;
  if (yuyv_in && !prep_yuyv_fusable(W, roi, tab)) return hipErrorInvalidValue;      // (the caller converts the frames first: bsx_api.hip step_impl)
  const int ntx = (inW + 31) / 32, nty = (inH + 31) / 32, TW = (inW + ntx - 1) / ntx, TH = (inH + nty - 1) / nty;      // even tiles, <= 32 x 32
  const long per_frame = (long)inW * inH;
  const int chunk = 1 << 20;                                            // frames per launch: keeps the 1-D grid far below 2^31 workgroups
  for (int n0 = 0; n0 < n; n0 += chunk) {
    const int nn = n - n0 < chunk ? n - n0 : chunk;
    const dim3 grid((unsigned)(ntx * nty) * (unsigned)nn);
    const uint8_t* fr = frames + (size_t)n0 * W * H * (yuyv_in ? 2 : 3);
    float* f = input ? input + (size_t)n0 * per_frame * 3 : nullptr;
    uint32_t* u = input_u8 ? input_u8 + (size_t)n0 * per_frame : nullptr;
#define BSX_PF(O, L) prep_fused_k<O, L><<<grid, kThreads, 0, s>>>(fr, W, H, roi, f, u, inW, inH, in_roi, tab, bp, TW, TH, ntx, nty, xcd_frames(nn))
#define BSX_PFY(O) prep_fused_k<O, true, true><<<grid, kThreads, 0, s>>>(fr, W, H, roi, f, u, inW, inH, in_roi, tab, bp, TW, TH, ntx, nty, xcd_frames(nn))
    if (yuyv_in) { if (f && u) BSX_PFY(3); else if (u) BSX_PFY(2); else BSX_PFY(1); }
    else
    if (tab.mode == 0 && (W - roi.x) * 3 >= 8) { if (f && u) BSX_PF(3, true); else if (u) BSX_PF(2, true); else BSX_PF(1, true); }   // (the 8-byte tap window needs an 8-byte row)
    else { if (f && u) BSX_PF(3, false); else if (u) BSX_PF(2, false); else BSX_PF(1, false); }
#undef BSX_PF
#undef BSX_PFY
  }
  return hipGetLastError();
}

bool bilateral_taps_match(const BilateralParams& bp) {
  static const int ty[13] = {-2, -1, -1, -1, 0, 0, 0, 0, 0, 1, 1, 1, 2}, tx[13] = {0, -1, 0, 1, -2, -1, 0, 1, 2, -1, 0, 1, 0};
  for (int k = 0; k < 13; k++) if (bp.off_y[k] != ty[k] || bp.off_x[k] != tx[k]) return false;
  return true;
}


hipError_t launch_decode(int model_type, const float* logits, uint8_t* ofinal, int npix, int nch, int n, hipStream_t s, const int* slot_of) {
  // dense: one flat grid over the n frames; slot_of: one grid row per frame (a frame's state lives at slot_of[frame], not next to the previous frame's)
  const long total = slot_of ? (long)npix : (long)n * npix;
  const unsigned rows = slot_of ? (unsigned)n : 1u;
  if (rows > (unsigned)kMaxGridY) return hipErrorInvalidValue;
  int type = model_type == 1 ? 1 : (model_type == 3 ? 3 : 2);
  if (type == 3 && nch == 2 && (total & 3) == 0 && ((((uintptr_t)logits) & 15) | (((uintptr_t)ofinal) & 3)) == 0)
    decode_meet4_k<<<dim3(blocks_for(total / 4), rows), kThreads, 0, s>>>(reinterpret_cast<const float4*>(logits), reinterpret_cast<uint32_t*>(ofinal), total / 4, slot_of);
  else if (type == 2 && nch == 1 && (total & 3) == 0 && ((((uintptr_t)logits) & 15) | (((uintptr_t)ofinal) & 3)) == 0)
    decode_thresh4_k<<<dim3(blocks_for(total / 4), rows), kThreads, 0, s>>>(reinterpret_cast<const float4*>(logits), reinterpret_cast<uint32_t*>(ofinal), total / 4, slot_of);
  else if (type == 1 && nch <= kArgmaxMaxCh) decode_argmax_k<<<dim3(blocks_for(total), rows), kThreads, 0, s>>>(logits, ofinal, total, nch, slot_of);
  else decode_k<<<dim3(blocks_for(total), rows), kThreads, 0, s>>>(type, logits, ofinal, total, nch, slot_of);
  return hipGetLastError();
}

// Every tile's source block must fit the LDS staging area of mask_tile_k (host tables, checked once per ResizeTab).
int mask_tile_width() { return kTW; }
int mask_tile_height() { return kTH; }
bool mask_tile_fits(const int* xofs, const int* yofs, int sw, int sh, int dw, int dh, int shift) {
  auto clampi = [](int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); };
  int max_rows = 0, max_cols = 0;
  for (int ty0 = 0; ty0 < dh; ty0 += kTH) {
    const int lo = std::max(ty0 - 2, 0), hi = std::min(ty0 + kTH + 1, dh - 1);
    max_rows = std::max(max_rows, clampi(yofs[hi] + 1, 0, sh - 1) - clampi(yofs[lo], 0, sh - 1) + 1);
  }
  for (int tx0 = -shift; tx0 < dw; tx0 += kTW) {
    const int lo = std::max(tx0 - 2, 0), hi = std::min(tx0 + kTW + 1, dw - 1);
    max_cols = std::max(max_cols, std::min(xofs[hi] + 1, sw - 1) - xofs[lo] + 1);
  }
  return max_rows <= kMaxSrcRows && max_rows * max_cols <= kSrcBlockBytes;
}

// BSX_NO_MASK_TILE=1 (read ONCE, when the context builds its resize tables: it clears ResizeTab::tile_ok) forces the generic kernel: the parity tests use it to cover both.
static bool mask_tile_usable(const ResizeTab& tab) { return tab.mode == 0 && tab.tile_ok; }

hipError_t launch_mask_upscale_blur(const uint8_t* ofinal, int outW, int outH, Rect4 in_roi, ResizeTab tab, uint8_t* mask, int W, int H, Rect4 roi,
                                    int n, hipStream_t s, const int* slot_of) {
  const MaskTileGrid g = mask_tile_grid(W, roi, n);
  if (!g.ok) return hipErrorInvalidValue;
  const int ntx = g.ntx, nty = g.nty, nf = g.nf;
  const dim3 grid = g.grid(nty, n);
  if (hipError_t e = launch_tile_class(ofinal, outW, outH, in_roi, tab, roi, n, s, slot_of)) return e;
  if (mask_tile_usable(tab)) mask_tile_k<false><<<grid, kThreads, 0, s>>>(ofinal, outW, outH, in_roi, tab, mask, W, H, roi, nullptr, 0, nullptr, nullptr, 0, ntx, nty, nf, 0, nty, slot_of);
  else mask_upscale_blur_k<false><<<grid, kThreads, 0, s>>>(ofinal, outW, outH, in_roi, tab, mask, W, H, roi, nullptr, 0, nullptr, nullptr, 0, ntx, nty, nf, slot_of);
  return hipGetLastError();
}

// Tile classes of one frame per workgroup: is a tile's source block — the extents mask_tile_k computes — all 0xFF (→ 1), all 0x00 (→ 2) or neither (→ 0)?
// Two steps through LDS so that every model-resolution byte is looked at once per tile COLUMN, with wide loads: (1) item (row r, tile column tbx) scans the bytes
// [cmin(tbx), cmax(tbx)] of row r as unaligned dwords, AND / OR accumulated → two flags; (2) tile (tby, tbx) ANDs the flags of its rows [smin(tby), smax(tby)].
// (The first version gave every tile a wave that walked its block row by row, byte by byte: 17 us at 256 lite/VGA streams, 151 us at 1024 DeepLab streams —
// more than the shortcut saved; profiles/r04g.)
constexpr int kClsMaxItems = 8192, kClsMaxTx = 16;
__global__ __launch_bounds__(kThreads) void tile_class_k(const uint8_t* __restrict__ ofinal, int outW, int outH, Rect4 q, ResizeTab tab, Rect4 roi, int ntx, int nty,
                                                        const int* __restrict__ slot_of) {
  const int n = blockIdx.x, tid = threadIdx.x;
#define BSX_CLS_FRAME ofinal + (long)(slot_of ? slot_of[n] : n) * outW * outH + (long)q.y * outW + q.x      /* state slot; the classes stay per position n */
#define BSX_CLS_BYTE(t) tab.tile_class[(size_t)n * (size_t)(ntx * nty) + t]
#include "tile_class.inc"
#undef BSX_CLS_FRAME
#undef BSX_CLS_BYTE
}

hipError_t launch_tile_class(const uint8_t* ofinal, int outW, int outH, const Rect4& in_roi, const ResizeTab& tab, const Rect4& roi, int n, hipStream_t s, const int* slot_of) {
  if (!tab.tile_class || !mask_tile_usable(tab)) return hipSuccess;
  const int ntx = (roi.w + kTW - 1) / kTW, nty = (roi.h + kTH - 1) / kTH;
  if (ntx > kClsMaxTx || (long)tab.sh * ntx > kClsMaxItems) return hipMemsetAsync(tab.tile_class, 0, (size_t)ntx * nty * n, s);      // out of the classifier's range: all general
  tile_class_k<<<dim3((unsigned)n), kThreads, 0, s>>>(ofinal, outW, outH, in_roi, tab, roi, ntx, nty, slot_of);
  return hipGetLastError();
}

bool mask_blend_fusable(int W, int H, Rect4 roi, const uint8_t* bg, size_t bg_stride, const uint8_t* frames, const uint8_t* out) {
  return (W % 4) == 0 && (roi.x % 4) == 0 && (roi.w % 4) == 0 && (bg_stride % 4) == 0 &&
         ((((uintptr_t)bg) | ((uintptr_t)frames) | ((uintptr_t)out)) & 3) == 0;
}

hipError_t launch_mask_blend(const uint8_t* ofinal, int outW, int outH, Rect4 in_roi, ResizeTab tab, uint8_t* mask, int W, int H, Rect4 roi,
                             const uint8_t* bg, size_t bg_stride, const uint8_t* frames, uint8_t* out, int n, hipStream_t s, int yuyv, int lds_pad, const int* slot_of) {
  // lds_pad (bytes of dynamic LDS nobody uses): an OCCUPANCY CAP for the two-deep pipeline (bsx_step_batch_pipelined) — left alone this HBM-bound launch takes every wave
  // slot of every CU and the latency-bound network kernels of the other stream run on what is left (seg_head 2.65x slower, profiles/r04k); with the pad only
  // 160 KB / (static + pad) workgroups fit a CU
  // outside the ROI the persistent mask is 255 forever (libbackscrub.cc:248-249), i.e. the composite there IS the background
  // ((a*255 + b*0)/255 == a): those strips are copied, the ROI is composited by the mask tiles
  // `yuyv`: bit 0 = YUYV output, bits 1-2 = horizontal / vertical flip of the composite, bit 3 = do not store the full-resolution mask, bit 4 = `frames` is YUYV
  // 4:2:2 (bsx.h: BSX_STEP_*); outside the ROI no frame pixel is read
  const bool strips = !roi_is_frame(W, H, roi);
  if (strips && (yuyv & 6))
    outside_roi_flip_k<<<dim3(blocks_for((long)(W / 4) * H), n), kThreads, 0, s>>>(bg, (long)bg_stride, out, W, H, roi, yuyv);
  else if (strips && (yuyv & 1))
    outside_roi_yuyv_k<<<dim3(blocks_for((long)(W / 2) * H), n), kThreads, 0, s>>>(bg, (long)bg_stride, reinterpret_cast<uint32_t*>(out), W, H, roi);
  else if (strips)
    outside_roi_copy_k<<<dim3(blocks_for(((long)(H - roi.h) * (W * 3 / 4) + (long)roi.h * ((W - roi.w) * 3 / 4) + 3) / 4), n), kThreads, (size_t)lds_pad, s>>>(bg, (long)bg_stride, out, W, H,
                                                                                                                                 roi);
  const MaskTileGrid g = mask_tile_grid(W, roi, n);
  if (!g.ok) return hipErrorInvalidValue;
  const int ntx = g.ntx, nty = g.nty, nf = g.nf;
  const dim3 grid = g.grid(nty, n);
  if (hipError_t e = launch_tile_class(ofinal, outW, outH, in_roi, tab, roi, n, s, slot_of)) return e;
  yuyv |= tile_debug_bits();
  const bool yin = (yuyv & 16) != 0;
  if (mask_tile_usable(tab)) {
    const bool f0 = (yuyv & ~16) == 0;
    // whole tile rows (every item inside the ROI: the WH instantiation) and, where the ROI height is not a multiple of the tile height (720 = 22.5 x 32), the last,
    // partial row as a second launch of the edge-testing instantiation
    const bool whole_x = f0 && roi.w % kTW == 0 && ((uintptr_t)mask & 3) == 0;      // (W, roi.x multiples of 4: mask_blend_fusable)
    const int nty_whole = whole_x ? roi.h / kTH : 0;
#define BSX_MT(Y, F, WHL, GRID, NTY, TYB) mask_tile_k<true, Y, F, WHL><<<GRID, kThreads, (size_t)lds_pad, s>>>(ofinal, outW, outH, in_roi, tab, mask, W, H, roi, bg, (long)bg_stride, frames, out, yuyv, ntx, NTY, nf, TYB, nty, slot_of)
    if (nty_whole > 0) {
      const dim3 gw = g.grid(nty_whole, n), gr = g.grid(nty - nty_whole, n);
      if (yin) { BSX_MT(true, true, true, gw, nty_whole, 0); if (nty > nty_whole) BSX_MT(true, true, false, gr, nty - nty_whole, nty_whole); }
      else { BSX_MT(false, true, true, gw, nty_whole, 0); if (nty > nty_whole) BSX_MT(false, true, false, gr, nty - nty_whole, nty_whole); }
    } else if (yin) { if (f0) BSX_MT(true, true, false, grid, nty, 0); else BSX_MT(true, false, false, grid, nty, 0); }
    else { if (f0) BSX_MT(false, true, false, grid, nty, 0); else BSX_MT(false, false, false, grid, nty, 0); }
#undef BSX_MT
  } else if (yin) mask_upscale_blur_k<true, true><<<grid, kThreads, 0, s>>>(ofinal, outW, outH, in_roi, tab, mask, W, H, roi, bg, (long)bg_stride, frames, out, yuyv, ntx, nty, nf, slot_of);
  else mask_upscale_blur_k<true, false><<<grid, kThreads, 0, s>>>(ofinal, outW, outH, in_roi, tab, mask, W, H, roi, bg, (long)bg_stride, frames, out, yuyv, ntx, nty, nf, slot_of);
  return hipGetLastError();
}

// the mixed batch (bsx_step_batch_mixed): the geometry of launch_mask_blend, every position's background / flip / filter from the descriptor table — the strips
// outside the ROI by outside_roi_mixed_k, the ROI by the MIX instantiations (one tile launch whatever the settings); the descriptor table travels in the
// kernels' `bg` argument, so the dense instantiations keep their argument list
hipError_t launch_mask_blend_mixed(const uint8_t* ofinal, int outW, int outH, Rect4 in_roi, ResizeTab tab, uint8_t* mask, int W, int H, Rect4 roi,
                                   const MixDesc* desc, const uint8_t* frames, uint8_t* out, int n, hipStream_t s, int flags, const int* slot_of) {
  flags &= 1 | 8 | 16;
  if (!roi_is_frame(W, H, roi))
    outside_roi_mixed_k<<<dim3(blocks_for((long)(W / 4) * H), n), kThreads, 0, s>>>(desc, frames, out, W, H, roi, flags);
  const MaskTileGrid g = mask_tile_grid(W, roi, n);
  if (!g.ok) return hipErrorInvalidValue;
  const int ntx = g.ntx, nty = g.nty, nf = g.nf;
  const dim3 grid = g.grid(nty, n);
  if (hipError_t e = launch_tile_class(ofinal, outW, outH, in_roi, tab, roi, n, s, slot_of)) return e;
  flags |= tile_debug_bits() & 128;                                     // (no early background request to switch off here)
  const uint8_t* const d = reinterpret_cast<const uint8_t*>(desc);
  const bool yin = (flags & 16) != 0;
  if (mask_tile_usable(tab)) {
    if (yin) mask_tile_k<true, true, false, false, true><<<grid, kThreads, 0, s>>>(ofinal, outW, outH, in_roi, tab, mask, W, H, roi, d, 0, frames, out, flags, ntx, nty, nf, 0, nty, slot_of);
    else mask_tile_k<true, false, false, false, true><<<grid, kThreads, 0, s>>>(ofinal, outW, outH, in_roi, tab, mask, W, H, roi, d, 0, frames, out, flags, ntx, nty, nf, 0, nty, slot_of);
  } else if (yin) mask_upscale_blur_k<true, true, true><<<grid, kThreads, 0, s>>>(ofinal, outW, outH, in_roi, tab, mask, W, H, roi, d, 0, frames, out, flags, ntx, nty, nf, slot_of);
  else mask_upscale_blur_k<true, false, true><<<grid, kThreads, 0, s>>>(ofinal, outW, outH, in_roi, tab, mask, W, H, roi, d, 0, frames, out, flags, ntx, nty, nf, slot_of);
  return hipGetLastError();
}

// ---- bsx_step_batch_geoms: positions of several capture sizes in one prep, one tile-class, one tile [and one outside-ROI] launch (kernels.hpp: GeomClass, GeomDesc,
// GeomSpans).  The kernels below are the bodies of prep_fused_k, tile_class_k, mask_tile_k<BLEND, .., MIX> and outside_roi_mixed_k with the geometry read per position.
// They keep names of their own, so no dense instantiation changes its template arguments or its mangled name, and they share the TEXT of those bodies (prep_tile.inc,
// tile_class.inc, mask_tile.inc; outside_mixed_group): what one stream computes cannot differ between the two forms.  That sharing changes no kernel's code is checked,
// not assumed: tools/isa_same.py compares every kernel's assembly with another revision's.
namespace {
// workgroup (or position) `id` of a ragged grid: its class g, the class's first workgroup w0, first position p0, one-past-last position p1 and workgroups per position
// — compares and selects on SGPRs (id is workgroup-uniform, the spans are kernel arguments): nothing is loaded
__device__ __forceinline__ void geom_span(const GeomSpans& sp, int id, int* g, int* w0, int* p0, int* p1, int* per) {
  *g = 0; *w0 = sp.wg[0]; *p0 = sp.pos[0]; *p1 = sp.pos[1]; *per = sp.per[0];
#pragma unroll
  for (int k = 1; k < kMaxGeoms; k++)
    if (id >= sp.wg[k]) { *g = k; *w0 = sp.wg[k]; *p0 = sp.pos[k]; *p1 = sp.pos[k + 1]; *per = sp.per[k]; }
}
__device__ __forceinline__ int geom_class_of_position(const GeomSpans& sp, int n) {
  int g = 0;
#pragma unroll
  for (int k = 1; k < kMaxGeoms; k++) if (n >= sp.pos[k]) g = k;
  return g;
}
// a resize table read from a class record: its pointers as global-memory pointers (as_global: a pointer read from memory is otherwise a generic one)
__device__ __forceinline__ ResizeTab geom_tab(const ResizeTab& t) {
  ResizeTab r = t;
  r.xofs = as_global(t.xofs); r.xa = as_global(t.xa); r.yofs = as_global(t.yofs); r.ya = as_global(t.ya); r.tile_class = nullptr;
  return r;
}
// descriptor n: three 16-byte uniform loads, the pointers rebuilt as global-memory pointers (mix_desc)
struct GeomDescRegs { const uint8_t* frame; uint8_t* out; const uint8_t* bg; uint8_t* mask; unsigned flags; int slot; };
__device__ __forceinline__ GeomDescRegs geom_desc(const GeomDesc* __restrict__ desc, int n) {
  const uint4* p = reinterpret_cast<const uint4*>(desc) + 3 * (size_t)n;
  const uint4 a = p[0], b = p[1], c = p[2];
  typedef __attribute__((address_space(1))) uint8_t* gp;
  GeomDescRegs d;
  d.frame = (const uint8_t*)(gp)(((uint64_t)a.y << 32) | a.x);
  d.out = (uint8_t*)(gp)(((uint64_t)a.w << 32) | a.z);
  d.bg = (const uint8_t*)(gp)(((uint64_t)b.y << 32) | b.x);
  d.mask = (uint8_t*)(gp)(((uint64_t)b.w << 32) | b.z);
  d.flags = c.x; d.slot = (int)c.y;
  return d;
}

// prep_fused_k per position: the uniform grid of the model canvas (ntx * nty tiles per position), frame, capture size, ROIs and the down-scale table from the position's
// class.  The table mode is the class's (a run-time, workgroup-uniform choice between the two bodies prep_fused_k picks at launch); the body is prep_tile.inc.
template <int OUT>
__global__ __launch_bounds__(kThreads) void prep_geoms_k(const GeomClass* __restrict__ classes, const GeomDesc* __restrict__ desc, GeomSpans sp, float* __restrict__ input,
                                                        uint32_t* __restrict__ input_u8, int inW, int inH, BilateralParams bp, int TW, int TH, int ntx, int nty, int n_frames) {
  unsigned f_, t_;
  xcd_frame_tile((unsigned)(ntx * nty), (unsigned)n_frames, &f_, &t_);
  const int g = geom_class_of_position(sp, (int)f_);
  const GeomClass c = classes[g];                                     // (uniform index: scalar loads) — independent of the descriptor's
  const uint8_t* const frame = geom_desc(desc, (int)f_).frame;
  const ResizeTab tab = geom_tab(c.down);
  if (tab.mode == 0 && (c.W - c.roi.x) * 3 >= 8)                      // launch_prep_fused's rule for the LINEAR body
    prep_geoms_tile<OUT, true>(frame, c.W, c.H, c.roi, input, input_u8, inW, inH, c.in_roi, tab, bp, TW, TH, ntx, (long)f_, t_);
  else
    prep_geoms_tile<OUT, false>(frame, c.W, c.H, c.roi, input, input_u8, inW, inH, c.in_roi, tab, bp, TW, TH, ntx, (long)f_, t_);
}

// tile_class_k per position: one workgroup per position, the class bytes at the position's place in the ragged tile grid (plain order: first workgroup of the class
// + position in the class x tiles per frame + tile) — where mask_tile_geoms_k finds its byte without loading anything first
__global__ __launch_bounds__(kThreads) void tile_class_geoms_k(const GeomClass* __restrict__ classes, const GeomDesc* __restrict__ desc, GeomSpans sp,
                                                              const uint8_t* __restrict__ ofinal, int outW, int outH, uint8_t* __restrict__ tile_class) {
  const int n = blockIdx.x, g = geom_class_of_position(sp, n);
  const GeomClass c = classes[g];
  const int slot = geom_desc(desc, n).slot;
  uint8_t* const cls = tile_class + sp.wg[g] + (size_t)(n - sp.pos[g]) * (size_t)(c.ntx * c.nty);
  const ResizeTab tab = geom_tab(c.up);
  if (c.ntx > kClsMaxTx || tab.sh * c.ntx > kClsMaxItems) {           // out of the classifier's range (launch_tile_class): all general
    for (int t = threadIdx.x; t < c.ntx * c.nty; t += kThreads) cls[t] = 0;
    return;
  }
  const int tid = threadIdx.x, ntx = c.ntx, nty = c.nty;
  const Rect4 roi = c.roi;
#define BSX_CLS_FRAME ofinal + (long)slot * outW * outH + (long)c.in_roi.y * outW + c.in_roi.x
#define BSX_CLS_BYTE(t) cls[t]
#include "tile_class.inc"
#undef BSX_CLS_FRAME
#undef BSX_CLS_BYTE
}

// mask_tile_k<BLEND = true, YIN = false, F0 = false, WH = false, MIX = true> per position: its own prologue and uniform-tile branch, then mask_tile.inc with the
// position's own bases (index 0 of each) and its class's geometry.  The order of the loads is mask_tile_k's: class byte first (its address needs only the kernel
// arguments), class record and descriptor — two independent uniform loads — next to it, the state slot only where it is consumed.
__global__ __launch_bounds__(kThreads) void mask_tile_geoms_k(const GeomClass* __restrict__ classes, const GeomDesc* __restrict__ desc, GeomSpans sp, unsigned xcd_mask,
                                                             const uint8_t* __restrict__ ofinal, int outW, int outH, const uint8_t* __restrict__ tile_class, int yuyv) {
  __shared__ short col_c0[kHW], col_c1[kHW], col_a0[kHW], col_a1[kHW];
  __shared__ short row_r0[kHH], row_r1[kHH], row_b0[kHH], row_b1[kHH];
  __shared__ __attribute__((aligned(16))) uint16_t hq_hs[kMaxSrcRows * kHW > kHH * kTW ? kMaxSrcRows * kHW : kHH * kTW];
  __shared__ __attribute__((aligned(16))) uint8_t up[kHH * kHW + 8];
  uint16_t* const hq = hq_hs;
  uint16_t* const hs = hq_hs;
  uint8_t* const blk = up;
  const int tid = threadIdx.x;
  int g, w0, p0, p1, per;
  geom_span(sp, (int)blockIdx.x, &g, &w0, &p0, &p1, &per);
  unsigned f_, t_;
  xcd_frame_tile_at(blockIdx.x - (unsigned)w0, (unsigned)per, ((xcd_mask >> g) & 1u) ? (unsigned)(p1 - p0) : 0u, &f_, &t_);
  const int n = p0 + (int)f_;                                          // the position (descriptor index)
  int uniform = 0;
  if (tile_class) uniform = tile_class_byte((uintptr_t)tile_class + (size_t)w0 + (size_t)f_ * (size_t)per + (size_t)t_);
  const GeomClass c = classes[g];
  const GeomDescRegs d = geom_desc(desc, n);
  const int W = c.W, H = c.H;
  const Rect4 roi = c.roi, q = c.in_roi;
  const ResizeTab tab = geom_tab(c.up);
  const int tby = (int)t_ / c.ntx, tbx = (int)t_ - tby * c.ntx, tx0 = tbx * kTW, ty0 = tby * kTH;
  yuyv = (yuyv & ~16) | (int)(d.flags & (kMixFlipH | kMixFlipV));
  const int sel = (d.flags & kMixFilterOff) ? 2 : -1;
  TileBlendOperands ops;
  constexpr bool BLEND = true, WH = false, MIX = true, yin = false, early_bg = false;      // mask_tile.inc's names: the instantiation, the position's descriptor
  constexpr long bg_stride = 0;
  const uint8_t *const bg = d.bg, *const frames = d.frame;
  uint8_t *const mask = d.mask, *const outp = d.out;
  if (uniform) {
    tile_load_blend_operands<BLEND, WH, MIX>(ops, bg, bg_stride, frames, 0, W, H, roi, tx0, ty0, tid, uniform, 3, yin, sel);
    tile_vsum5_store<BLEND, WH, MIX>(hq_hs, mask, outp, ops, 0, 0, W, H, roi, tx0, ty0, tid, yuyv, uniform, sel);
    return;
  }
#define BSX_MT_FRAME 0                                               /* the position's own bases: index 0 of each */
#define BSX_MT_SLOT d.slot
#define BSX_MT_MASK_SLOT 0
#include "mask_tile.inc"
#undef BSX_MT_FRAME
#undef BSX_MT_SLOT
#undef BSX_MT_MASK_SLOT
}

// outside_roi_mixed_k per position: sp.per[g] workgroups for every position of a class whose ROI is not the frame, none for the others
__global__ __launch_bounds__(kThreads) void outside_roi_geoms_k(const GeomClass* __restrict__ classes, const GeomDesc* __restrict__ desc, GeomSpans sp, int flags) {
  int g, w0, p0, p1, per;
  geom_span(sp, (int)blockIdx.x, &g, &w0, &p0, &p1, &per);
  const unsigned local = blockIdx.x - (unsigned)w0, pl = local / (unsigned)per, blk = local - pl * (unsigned)per;
  const GeomClass c = classes[g];
  const GeomDescRegs d = geom_desc(desc, p0 + (int)pl);
  outside_mixed_group(blk * kThreads + threadIdx.x, d.bg, d.flags, d.frame, d.out, c.W, c.H, c.roi, flags & ~16);
}
}  // namespace

bool geom_class_fusable(int W, const Rect4& roi, const ResizeTab& up) { return (W % 4) == 0 && (roi.x % 4) == 0 && (roi.w % 4) == 0 && mask_tile_usable(up); }
int geom_outside_blocks(int W, int H, const Rect4& roi) {
  return roi_is_frame(W, H, roi) ? 0 : (int)blocks_for((long)(W / 4) * H);
}
bool geom_class_xcd(int W, const Rect4& roi) { return mask_tile_grid(W, roi, 1).nf != 0; }      // launch_mask_blend's rule, asked for one frame

hipError_t launch_prep_geoms(const GeomClass* classes, const GeomDesc* desc, const GeomSpans& spans, float* input, uint32_t* input_u8, int inW, int inH, BilateralParams bp,
                             int n, hipStream_t s) {
  if ((!input && !input_u8) || n <= 0) return hipErrorInvalidValue;
  const int ntx = (inW + 31) / 32, nty = (inH + 31) / 32, TW = (inW + ntx - 1) / ntx, TH = (inH + nty - 1) / nty;      // launch_prep_fused's tiles
  if ((unsigned long long)ntx * nty * (unsigned long long)n >= (1ull << 31)) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(ntx * nty) * (unsigned)n);
#define BSX_PG(O) prep_geoms_k<O><<<grid, kThreads, 0, s>>>(classes, desc, spans, input, input_u8, inW, inH, bp, TW, TH, ntx, nty, xcd_frames(n))
  if (input && input_u8) BSX_PG(3); else if (input_u8) BSX_PG(2); else BSX_PG(1);
#undef BSX_PG
  return hipGetLastError();
}

hipError_t launch_mask_blend_geoms(const GeomClass* classes, const GeomDesc* desc, const GeomSpans& tiles, unsigned xcd_mask, const GeomSpans& outside, const uint8_t* ofinal,
                                   int outW, int outH, uint8_t* tile_class, int n, hipStream_t s, int flags) {
  flags &= 1 | 8;
  if (n <= 0 || tiles.wg[kMaxGeoms] <= 0) return hipErrorInvalidValue;
  if (outside.wg[kMaxGeoms] > 0) outside_roi_geoms_k<<<dim3((unsigned)outside.wg[kMaxGeoms]), kThreads, 0, s>>>(classes, desc, outside, flags);
  if (tile_class) tile_class_geoms_k<<<dim3((unsigned)n), kThreads, 0, s>>>(classes, desc, tiles, ofinal, outW, outH, tile_class);
  flags |= tile_debug_bits() & 128;
  mask_tile_geoms_k<<<dim3((unsigned)tiles.wg[kMaxGeoms]), kThreads, 0, s>>>(classes, desc, tiles, xcd_mask, ofinal, outW, outH, tile_class, flags);
  return hipGetLastError();
}

hipError_t launch_blend(const uint8_t* bg, size_t bg_stride, const uint8_t* frames, const uint8_t* masks, uint8_t* out, size_t npix, int n,
                        hipStream_t s, const int* slot_of) {
  // lane-coalesced form: 4-byte alignment and whole 4-pixel groups are enough; anything else takes the per-pixel kernel
  const bool quad_ok = (((uintptr_t)bg | (uintptr_t)frames | (uintptr_t)masks | (uintptr_t)out) & 3) == 0 && (npix % 4 == 0) && (bg_stride % 4 == 0) && npix / 4 < (1l << 31);
  const long quads = quad_ok ? (long)(npix / 4) : 0;
  for (int n0 = 0; n0 < n; n0 += kMaxGridY) {
    const int nn = n - n0 < kMaxGridY ? n - n0 : kMaxGridY;
    const uint8_t* bgp = bg + (size_t)n0 * bg_stride;
    const uint8_t* fp = frames + (size_t)n0 * npix * 3;
    const uint8_t* mp = slot_of ? masks : masks + (size_t)n0 * npix;        // (with slot_of the masks are addressed by stream id, not by position)
    const int* sp = slot_of ? slot_of + n0 : nullptr;
    uint8_t* op = out + (size_t)n0 * npix * 3;
    if (quads) blend4x4_k<<<dim3((unsigned)((quads + kThreads * kB4 - 1) / (kThreads * kB4)), nn), kThreads, 0, s>>>(bgp, (long)bg_stride, fp, mp, op, (unsigned)quads, (long)npix, sp);
    else blend1_k<<<dim3(blocks_for((long)npix), nn), kThreads, 0, s>>>(bgp, (long)bg_stride, fp, mp, op, (long)npix, sp);
  }
  return hipGetLastError();
}

hipError_t launch_resize_bgr(const uint8_t* src, uint8_t* dst, ResizeTab tab, int n, hipStream_t s) {
  for (int n0 = 0; n0 < n; n0 += kMaxGridY) {
    const int nn = n - n0 < kMaxGridY ? n - n0 : kMaxGridY;
    resize_bgr_k<<<dim3(blocks_for((long)tab.dw * tab.dh), nn), kThreads, 0, s>>>(src + (size_t)n0 * tab.sw * tab.sh * 3, dst + (size_t)n0 * tab.dw * tab.dh * 3, tab);
  }
  return hipGetLastError();
}

hipError_t launch_resize_bgr_batch(const ResizeBatchDesc* desc, int n, int dw, int dh, hipStream_t s) {
  const long groups = (long)((dw + 3) / 4) * dh;
  if (groups >= (1l << 31)) return hipErrorInvalidValue;
  for (int n0 = 0; n0 < n; n0 += kMaxGridY) {
    const int nn = n - n0 < kMaxGridY ? n - n0 : kMaxGridY;
    resize_bgr_batch_k<<<dim3(blocks_for(groups), nn), kThreads, 0, s>>>(desc + n0, dw, dh);
  }
  return hipGetLastError();
}

// ---- cv::GaussianBlur(bg, bg, Size(n, n), 0) on packed BGR u8 (app/deepseg.cc:657-658, `-p bgblur:<n>`) ------------------------------
// OpenCV's 8-bit Gaussian is an integer separable filter: u8-valued coefficients c[k] = cvRound(kernel * 256) (host table), the
// horizontal pass Σ c·src in u16 (8 fractional bits), the vertical pass Σ c·h in u32 (16 fractional bits), (v + 2^15) >> 16,
// BORDER_REFLECT_101.  With Σc <= 257 neither intermediate can overflow, so the saturating adds of the reference never trigger.
// Tile = 64 x 16 output pixels per workgroup.  The source tile (+ radius r <= 15 on every side) is de-interleaved into three byte
// planes in LDS so that consecutive taps of one channel are consecutive bytes: the horizontal pass then does 4 taps per
// v_dot4_u32_u8 on windows shifted out of aligned dwords with v_alignbyte; its u16 results are stored transposed ([col][row]) so the
// vertical pass does 2 taps per v_dot2_u32_u16 the same way.  HBM traffic = the image once in, once out.
constexpr int kGTW = 64, kGTH = 16, kGMaxR = 15, kGSW = kGTW + 2 * kGMaxR, kGSH = kGTH + 2 * kGMaxR;    // 94 x 46 source tile
constexpr int kGSrcStride = 96;                  // bytes per plane row (multiple of 4)
constexpr int kGHStride = 48;                    // u16 per hbuf column (rows of the source tile, even)
// hbuf column c of a plane starts 2 * (c / 8) dwords late: the horizontal pass writes 16 column groups (4 columns = 96 dwords apart: banks 0 / 32 only, an 8-way
// conflict on every store) at once, the shift spreads them over 16 banks; the vertical pass reads 8 CONSECUTIVE columns per wave (24 dwords apart: conflict-free),
// which share one shift.
constexpr int kGHPlane = kGTW * kGHStride + 32;  // u16 per plane: 64 columns + the largest shift (14 dwords) rounded up
__device__ __forceinline__ int gh_col(int plane, int col) { return plane * kGHPlane + col * kGHStride + 4 * (col >> 3); }
// c[k] packed 4 per dword (bytes) and 2 per dword (u16), zero padded — once per output phase: c4[j] is the tap sequence delayed by j bytes, c2[s] by s halves, so that
// the 4 neighbouring outputs of a horizontal item (2 of a vertical item) are dot products of the SAME aligned data words with different coefficient words
// (one v_dot per word and output) instead of realigned windows with one coefficient set (v_alignbyte + v_dot per word and output).
struct GaussCoef { uint32_t c4[4][9]; uint32_t c2[2][17]; int n, r, sh; };   // sh: the LDS planes start sh (0..3) pixels left of the tile's first source column
typedef unsigned short us2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int reflect101_far(int p, int len) {   // cv::borderInterpolate(BORDER_REFLECT_101) for overshoots beyond one period
  if (len == 1) return 0;
  while (p < 0 || p >= len) p = p < 0 ? -p : 2 * len - 2 - p;
  return p;
}
// MODE 0: the vertical pass stores its bytes itself (any geometry).  MODE 1 (W % 4 == 0, 4-byte aligned images): the vertical pass leaves the blurred tile in LDS
// as packed BGR rows and the workgroup writes it as whole dwords, one 4-pixel group (12 B) per lane — each lane of the vertical pass owns two ROWS of one column of
// one plane, i.e. byte stores scattered over 16 image rows.  MODE 2 = MODE 1 with the alpha blend (deepseg.cc:108-134) applied to the group on its way out:
// `-p bgblur` without `-b` (deepseg.cc:652-661) composites the camera frame over ITS OWN blur, so the blurred image is consumed where it is produced — it never
// exists in HBM, and neither does the blend's second read of the frame (the lane's frame / mask words are requested at the top of the kernel).
// NT = ceil((ksize + 3 + sh) / 4), a template parameter: the tap loops are straight-line code over NT horizontal / 2 NT - 1 vertical data words (the coefficient bytes past
// ksize are zero, so the surplus taps add 0 whatever bytes they read), not loops predicated tap by tap.
// The kernel is bound by VALU issue, not by memory (ksize 3 costs half of ksize 25), so the per-byte index arithmetic is what there is to save:
//   * items advance by precomputed (row, column) steps instead of a runtime division per item, addresses are 32-bit offsets from a uniform base;
//   * opt bit 0 (rows dword aligned), tiles whose source columns lie inside the image: the source tile is staged 4 pixels (three dwords) per item and
//     de-interleaved with six v_perm_b32 into one dword per plane, instead of three byte loads + three byte LDS stores per pixel (rows still reflect).
constexpr int kGOStride = 196;                   // bytes per packed output row in LDS: 64 px x 3 B + 4 (49 dwords: the 16 rows start on distinct banks)
static_assert(kGTH * (kGTW / 4) == kThreads && kGTH * kGOStride <= 3 * kGSH * kGSrcStride, "one 4-pixel group per lane; the output tile aliases the source planes");
template <int MODE, int NT>
__global__ __launch_bounds__(kThreads) void gauss_blur_k(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const uint8_t* __restrict__ mask, int W, int H, GaussCoef gc,
                                                         int opts, const int* __restrict__ slot_of) {
  __shared__ __attribute__((aligned(16))) uint8_t s_src[3 * kGSH * kGSrcStride];          // [plane][row][col]; MODE >= 1: later the packed output tile [row][kGOStride]
  __shared__ __attribute__((aligned(16))) uint16_t s_h[3 * kGHPlane];                     // [plane][col][row], gh_col()
  // MODE 0 / 1 read slot_of as a position list when one is given (bsx_step_batch_mixed: the positions of one blur size): image blockIdx.z of the launch is image
  // slot_of[blockIdx.z] of src and dst; MODE 2 reads it as the frames' state slots (below)
  const size_t img = (size_t)(MODE < 2 && slot_of ? (unsigned)slot_of[blockIdx.z] : blockIdx.z) * (size_t)W * H * 3;
  const uint8_t* in = src + img;
  uint8_t* out = dst + img;
  const int x0 = blockIdx.x * kGTW, y0 = blockIdx.y * kGTH, r = gc.r;
  const int SW = kGTW + 2 * r, SH = kGTH + 2 * r;                                          // live part of the source tile
  // MODE >= 1: this lane's 4-pixel group of the tile
  const int orow = threadIdx.x >> 4, ogx = x0 + 4 * (threadIdx.x & 15), ogy = y0 + orow;
  const bool olive = MODE >= 1 && ogx < W && ogy < H;
  uint32_t fr[3] = {0u, 0u, 0u}, mw = 0u;
  if (MODE == 2 && olive) {
    const uint32_t* fp = reinterpret_cast<const uint32_t*>(in + (unsigned)(ogy * W + ogx) * 3u);
    fr[0] = fp[0]; fr[1] = fp[1]; fr[2] = fp[2];
    const size_t ms = slot_of ? (size_t)slot_of[blockIdx.z] : (size_t)blockIdx.z;      // the frame's persistent mask: state slot (one scalar load)
    mw = *reinterpret_cast<const uint32_t*>(mask + ms * (size_t)W * H + (unsigned)(ogy * W + ogx));
  }
  // 1. stage + de-interleave (reflected at the image border)
  //    The planes start at source column x0 - r - sh, sh = (-r) & 3 when 4-pixel staging is on (a multiple of 4 → aligned 12-byte groups), else 0; the horizontal
  //    pass never sees the difference: its coefficient words are delayed by sh more bytes (gauss_coefficients).
  const int sh = gc.sh, G = (SW + sh + 3) >> 2;                        // 4-pixel groups per staged row
  const bool xin = (opts & 1) && x0 - r - sh >= 0 && x0 - r - sh + 4 * G <= W;   // uniform: every group of every row lies inside the image row
  if (xin) {                                                          // item = (row, group of 4 pixels): 12 source bytes → one dword per plane
    int row = (int)threadIdx.x / G, grp = (int)threadIdx.x - row * G;
    const int dr = kThreads / G, dc = kThreads - dr * G;
    const unsigned xb = (unsigned)(x0 - r - sh);
    while (row < SH) {
      const int gy = reflect101_far(y0 - r + row, H);
      const uint32_t* p = reinterpret_cast<const uint32_t*>(in + ((unsigned)(gy * W) + xb + 4u * (unsigned)grp) * 3u);
      const uint32_t d0 = p[0], d1 = p[1], d2 = p[2];                 // B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3
      const uint32_t pb = __builtin_amdgcn_perm(d2, __builtin_amdgcn_perm(d1, d0, 0x00060300u), 0x05020100u);
      const uint32_t pg = __builtin_amdgcn_perm(d2, __builtin_amdgcn_perm(d1, d0, 0x00070401u), 0x06020100u);
      const uint32_t pr = __builtin_amdgcn_perm(d2, __builtin_amdgcn_perm(d1, d0, 0x00000502u), 0x07040100u);
      uint32_t* o = reinterpret_cast<uint32_t*>(s_src + row * kGSrcStride) + grp;
      o[0] = pb; o[kGSH * kGSrcStride / 4] = pg; o[2 * kGSH * kGSrcStride / 4] = pr;
      grp += dc; row += dr;
      if (grp >= G) { grp -= G; row++; }
    }
  } else {
    int row = (int)threadIdx.x / SW, col = (int)threadIdx.x - row * SW;
    const int dr = kThreads / SW, dc = kThreads - dr * SW;
    while (row < SH) {
      const int gy = reflect101_far(y0 - r + row, H), gx = reflect101_far(x0 - r + col, W);
      const uint8_t* p = in + (unsigned)(gy * W + gx) * 3u;
      const uint8_t b = p[0], g = p[1], rr = p[2];
      s_src[(0 * kGSH + row) * kGSrcStride + col + sh] = b;
      s_src[(1 * kGSH + row) * kGSrcStride + col + sh] = g;
      s_src[(2 * kGSH + row) * kGSrcStride + col + sh] = rr;
      col += dc; row += dr;
      if (col >= SW) { col -= SW; row++; }
    }
  }
  __syncthreads();
  // 2. horizontal pass: item = (plane, source row, group of 4 output columns); consecutive items of a lane are kThreads / 16 = 16 rows apart (SH > 16: one wrap at most)
  static_assert(kGTW / 4 == 16 && kThreads / 16 == kGTH && NT >= 2 && NT <= 9, "lane → (row, column group) mapping of the horizontal pass");
  for (int grp = threadIdx.x & 15, row = threadIdx.x >> 4, plane = 0; plane < 3;) {
    const uint32_t* rowp = reinterpret_cast<const uint32_t*>(s_src + (plane * kGSH + row) * kGSrcStride) + grp;   // bytes 4*grp ..
    uint32_t d[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) d[t] = rowp[t];                           // stays inside the 96-byte row: 4 * (15 + NT) <= 96
    uint32_t acc[4] = {0, 0, 0, 0};
#pragma unroll
    for (int t = 0; t < NT; t++) {
#pragma unroll
      for (int j = 0; j < 4; j++) acc[j] = __builtin_amdgcn_udot4(d[t], gc.c4[j][t], acc[j], false);
    }
#pragma unroll
    for (int j = 0; j < 4; j++) s_h[gh_col(plane, 4 * grp + j) + row] = (uint16_t)acc[j];      // sum(c) <= 257 (gauss_coefficients): 255 * 257 fits 16 bits
    row += kGTH;
    if (row >= SH) { row -= SH; plane++; }
  }
  __syncthreads();
  // 3. vertical pass: item = (plane, output column, pair of output rows)
  constexpr int NP = 2 * NT - 1;                                           // ksize <= 4 NT - 3: ceil((ksize + 1) / 2) data words
  for (int i = threadIdx.x; i < 3 * kGTW * (kGTH / 2); i += kThreads) {
    const int m = i & (kGTH / 2 - 1), pc = i / (kGTH / 2), col = pc & (kGTW - 1), plane = pc / kGTW;
    const uint32_t* colp = reinterpret_cast<const uint32_t*>(s_h + gh_col(plane, col)) + m;                        // rows 2m ..
    uint32_t hd[NP];
#pragma unroll
    for (int t = 0; t < NP; t++) hd[t] = colp[t];                           // 2 (m + NP - 1) + 1 <= 47 < kGHStride
    uint32_t a0 = 0, a1 = 0;
#pragma unroll
    for (int t = 0; t < NP; t++) {
      a0 = __builtin_amdgcn_udot2(__builtin_bit_cast(us2v, hd[t]), __builtin_bit_cast(us2v, gc.c2[0][t]), a0, false);
      a1 = __builtin_amdgcn_udot2(__builtin_bit_cast(us2v, hd[t]), __builtin_bit_cast(us2v, gc.c2[1][t]), a1, false);
    }
    const uint8_t v0 = (uint8_t)min((a0 + (1u << 15)) >> 16, 255u), v1 = (uint8_t)min((a1 + (1u << 15)) >> 16, 255u);
    if (MODE >= 1) {
      s_src[(2 * m) * kGOStride + 3 * col + plane] = v0;
      s_src[(2 * m + 1) * kGOStride + 3 * col + plane] = v1;
    } else {
      const int gx = x0 + col, gy = y0 + 2 * m;
      if (gx < W) {
        if (gy < H) out[(unsigned)(gy * W + gx) * 3u + plane] = v0;
        if (gy + 1 < H) out[(unsigned)((gy + 1) * W + gx) * 3u + plane] = v1;
      }
    }
  }
  if (MODE >= 1) {
    __syncthreads();
    if (olive) {
      const uint32_t* bp = reinterpret_cast<const uint32_t*>(s_src + orow * kGOStride + 12 * (threadIdx.x & 15));
      uint32_t o3[3] = {bp[0], bp[1], bp[2]};
      if (MODE == 2) { const uint32_t a[3] = {o3[0], o3[1], o3[2]}; blend_quad(a, fr, mw, o3); }    // background = the blur, foreground = the frame itself
      uint32_t* op = reinterpret_cast<uint32_t*>(out + (unsigned)(ogy * W + ogx) * 3u);
      op[0] = o3[0]; op[1] = o3[1]; op[2] = o3[2];
    }
  }
}

// Coefficients of cv::GaussianBlur(ksize = n, sigma = 0) for 8-bit images (OpenCV 3.4 - 4.4 rule; DESIGN.md records the
// version ambiguity): fixed tables for n <= 7, else cvRound(exp(-x^2 / (2 sigma^2)) / sum * 256), sigma = 0.3 * ((n-1)/2 - 1) + 0.8.
bool gauss_coefficients(int n, GaussCoef* gc, int sh) {
  if (n < 1 || n > 2 * kGMaxR + 1 || !(n & 1)) return false;
  unsigned c[32] = {0};
  if (n == 1) c[0] = 256;
  else if (n == 3) { c[0] = 64; c[1] = 128; c[2] = 64; }
  else if (n == 5) { const unsigned t[] = {16, 64, 96, 64, 16}; for (int i = 0; i < 5; i++) c[i] = t[i]; }
  else if (n == 7) { const unsigned t[] = {8, 28, 56, 72, 56, 28, 8}; for (int i = 0; i < 7; i++) c[i] = t[i]; }
  else {
    const double sigma = ((n - 1) * 0.5 - 1) * 0.3 + 0.8, scale2x = (-0.5 * 0.25) / (sigma * sigma);
    double v[32], sum = 0;
    for (int i = 0, x = 1 - n; i < n; i++, x += 2) { v[i] = std::exp((double)(x * x) * scale2x); sum += v[i]; }
    const double inv = 1.0 / sum;
    for (int i = 0; i < n; i++) c[i] = (unsigned)std::lrint(v[i] * inv * 256.0);
  }
  unsigned total = 0;
  for (int i = 0; i < n; i++) { if (c[i] > 255 && n > 1) return false; total += c[i]; }
  if (total > 257) return false;                          // the kernel relies on Σc·255 fitting 16 bits
  *gc = GaussCoef{};
  gc->n = n; gc->r = n / 2; gc->sh = sh;
  if (n == 1) return true;                                // 256 does not fit a byte: n = 1 is served as a copy by the caller
  for (int j = 0; j < 4; j++)
    for (int i = 0; i < n; i++) gc->c4[j][(i + j + sh) >> 2] |= c[i] << (8 * ((i + j + sh) & 3));
  for (int h = 0; h < 2; h++)
    for (int i = 0; i < n; i++) gc->c2[h][(i + h) >> 1] |= c[i] << (16 * ((i + h) & 1));
  return true;
}
bool gauss_coeff_words(int ksize, int shift, uint32_t* c4, uint32_t* c2) {
  GaussCoef gc;
  if (shift < 0 || shift > 3 || ksize + shift > 32 || !gauss_coefficients(ksize, &gc, shift)) return false;
  memcpy(c4, gc.c4, sizeof(gc.c4));
  memcpy(c2, gc.c2, sizeof(gc.c2));
  return true;
}
static bool gauss_words(const void* a, const void* b, const void* c, int w) {      // whole-dword output groups: 4 pixels = 12 bytes at 4-byte aligned addresses
  static const bool off = [] { const char* e = BSX_DBG_ENV("BSX_GAUSS_BYTE_STORE"); return e && *e == '1'; }();
  return !off && (w & 3) == 0 && ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c)) & 3) == 0;
}
static int gauss_opts(const void* src, int w) {                                    // bit 0: 4-pixel staging of interior tiles (dword aligned rows)
  static const bool off = [] { const char* e = BSX_DBG_ENV("BSX_GAUSS_BYTE_STAGE"); return e && *e == '1'; }();
  return !off && (w & 3) == 0 && (((uintptr_t)src) & 3) == 0 ? 1 : 0;
}
template <int MODE>
static void gauss_launch(dim3 grid, hipStream_t s, const uint8_t* src, uint8_t* dst, const uint8_t* mask, int w, int h, const GaussCoef& gc, int opts,
                         const int* slot_of = nullptr) {
  switch ((gc.n + gc.sh + 6) >> 2) {                      // NT = ceil((ksize + 3 + sh) / 4): 2 .. 9
#define BSX_G(NT) case NT: gauss_blur_k<MODE, NT><<<grid, kThreads, 0, s>>>(src, dst, mask, w, h, gc, opts, slot_of); break;
    BSX_G(2) BSX_G(3) BSX_G(4) BSX_G(5) BSX_G(6) BSX_G(7) BSX_G(8) BSX_G(9)
#undef BSX_G
    default: break;
  }
}
hipError_t launch_gauss_blur(const uint8_t* src, uint8_t* dst, int w, int h, int ksize, int n, hipStream_t s, const int* positions) {
  GaussCoef gc;
  const int opts = gauss_opts(src, w);
  if (!gauss_coefficients(ksize, &gc, (opts & 1) ? (-(ksize / 2)) & 3 : 0)) return hipErrorInvalidValue;
  if (ksize == 1) return positions ? hipErrorInvalidValue : hipMemcpyAsync(dst, src, (size_t)n * w * h * 3, hipMemcpyDeviceToDevice, s);
  const bool words = gauss_words(src, dst, nullptr, w);
  for (int n0 = 0; n0 < n; n0 += kMaxGridY) {
    const int nn = n - n0 < kMaxGridY ? n - n0 : kMaxGridY;
    const dim3 grid((w + kGTW - 1) / kGTW, (h + kGTH - 1) / kGTH, nn);
    const size_t off = positions ? 0 : (size_t)n0 * w * h * 3;           // a position list addresses the images itself
    const int* pos = positions ? positions + n0 : nullptr;
    if (words) gauss_launch<1>(grid, s, src + off, dst + off, nullptr, w, h, gc, opts, pos);
    else gauss_launch<0>(grid, s, src + off, dst + off, nullptr, w, h, gc, opts, pos);
  }
  return hipGetLastError();
}
// out = alpha_blend(GaussianBlur(frames, ksize), frames, masks) in one pass over the frames (gauss_blur_k<2, ..>)
bool gauss_blend_fusable(const uint8_t* frames, const uint8_t* masks, const uint8_t* out, int w, int ksize) {
  return ksize >= 3 && ksize <= 2 * kGMaxR + 1 && (ksize & 1) && frames != out && gauss_words(frames, masks, out, w);
}
hipError_t launch_gauss_blend(const uint8_t* frames, const uint8_t* masks, uint8_t* out, int w, int h, int ksize, int n, hipStream_t s, const int* slot_of) {
  GaussCoef gc;
  const int opts = gauss_opts(frames, w);
  if (!gauss_coefficients(ksize, &gc, (opts & 1) ? (-(ksize / 2)) & 3 : 0) || !gauss_blend_fusable(frames, masks, out, w, ksize)) return hipErrorInvalidValue;
  for (int n0 = 0; n0 < n; n0 += kMaxGridY) {
    const int nn = n - n0 < kMaxGridY ? n - n0 : kMaxGridY;
    const uint8_t* mp = slot_of ? masks : masks + (size_t)n0 * w * h;        // (with slot_of the masks are addressed by stream id, not by position)
    gauss_launch<2>(dim3((w + kGTW - 1) / kGTW, (h + kGTH - 1) / kGTH, nn), s, frames + (size_t)n0 * w * h * 3, out + (size_t)n0 * w * h * 3, mp, w, h, gc, opts,
                    slot_of ? slot_of + n0 : nullptr);
  }
  return hipGetLastError();
}

// ---- composite at the virtual camera's geometry --------------------------------------------------------------------------------
// Does the source footprint of every output tile (both column orders: the footprint's 4-pixel grid depends on the horizontal flip) fit vcam_blend_resize_k's
// LDS staging area?  The same arithmetic as the kernel's; every (tile column, tile row) pair exists, so the largest product is the largest width times height.
// All four flip combinations are covered, which the per-stream kernel (vg_mixed_k: every workgroup its own flips) relies on: a vertical flip mirrors the rows
// fy_lo .. fy_hi as a block — the kernel stages fy_hi - fy_lo + 1 rows either way — and the column count does not depend on it.
bool vcam_tile_fits(const int* xofs, const int* yofs, int sw, int sh, int dw, int dh) {
  auto clampi = [](int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); };
  int max_rows = 0, max_cols = 0;
  for (int dy0 = 0; dy0 < dh; dy0 += kVH) {
    const int dy1 = std::min(dy0 + kVH, dh) - 1;
    max_rows = std::max(max_rows, clampi(yofs[dy1] + 1, 0, sh - 1) - clampi(yofs[dy0], 0, sh - 1) + 1);
  }
  for (int dx0 = 0; dx0 < dw; dx0 += kVW) {
    const int dx1 = std::min(dx0 + kVW, dw) - 1, lo = xofs[dx0], hi = std::min(xofs[dx1] + 1, sw - 1);
    for (int fh = 0; fh < 2; fh++) {
      const int c_lo = fh ? sw - 1 - hi : lo, c_hi = fh ? sw - 1 - lo : hi, g0 = c_lo & ~3;
      max_cols = std::max(max_cols, 4 * (((c_hi - g0) >> 2) + 1));
    }
  }
  return (long)max_rows * max_cols <= kVLdsWords;
}

hipError_t launch_vcam_blend_resize(const uint8_t* frames, bool yuyv_in, const uint8_t* bg, size_t bg_stride, const uint8_t* masks, uint8_t* out, int W, int H,
                                    ResizeTab tab, bool direct, int n, hipStream_t s, unsigned flags) {
  if (tab.mode != 0 || tab.sw != W || tab.sh != H || (yuyv_in && (W & 1)) || ((flags & 1) && (tab.dw & 1))) return hipErrorInvalidValue;
  const int ntx = (tab.dw + kVW - 1) / kVW, nty = (tab.dh + kVH - 1) / kVH;
  if ((long)ntx * nty >= (1l << 31)) return hipErrorInvalidValue;
  const bool words = W % 4 == 0 && bg_stride % 4 == 0 && ((((uintptr_t)frames) | ((uintptr_t)bg) | ((uintptr_t)masks)) & 3) == 0;
  const bool owords = (((uintptr_t)out) & 3) == 0 && ((flags & 1) || tab.dw % 4 == 0);
  const int opt = (int)(flags & 7u) | (words ? kVcWords : 0) | (owords ? kVcOutWords : 0);
  const size_t fb = (size_t)W * H * (yuyv_in ? 2 : 3), ob = (size_t)tab.dw * tab.dh * ((flags & 1) ? 2 : 3);
  for (int n0 = 0; n0 < n; n0 += kMaxGridY) {
    const int nn = n - n0 < kMaxGridY ? n - n0 : kMaxGridY;
    const dim3 grid((unsigned)(ntx * nty), (unsigned)nn);
    const uint8_t* f = frames + (size_t)n0 * fb;
    const uint8_t* b = bg + (size_t)n0 * bg_stride;
    const uint8_t* m = masks + (size_t)n0 * W * H;
    uint8_t* o = out + (size_t)n0 * ob;
#define BSX_VC(D, Y) vcam_blend_resize_k<D, Y><<<grid, kThreads, 0, s>>>(f, b, (long)bg_stride, m, o, W, H, tab, ntx, opt)
    if (direct) { if (yuyv_in) BSX_VC(true, true); else BSX_VC(true, false); }
    else { if (yuyv_in) BSX_VC(false, true); else BSX_VC(false, false); }
#undef BSX_VC
  }
  return hipGetLastError();
}

hipError_t launch_vg_mixed(const uint8_t* frames, bool yuyv_in, const MixDesc* desc, const uint8_t* masks, const int* slot_of, uint8_t* out, int W, int H,
                           ResizeTab tab, bool direct, int n, hipStream_t s, unsigned flags) {
  if (tab.mode != 0 || tab.sw != W || tab.sh != H || (yuyv_in && (W & 1)) || ((flags & 1) && (tab.dw & 1)) || (flags & ~1u)) return hipErrorInvalidValue;
  const int ntx = (tab.dw + kVW - 1) / kVW, nty = (tab.dh + kVH - 1) / kVH;
  if ((long)ntx * nty >= (1l << 31)) return hipErrorInvalidValue;
  const bool words = W % 4 == 0 && ((((uintptr_t)frames) | ((uintptr_t)masks)) & 3) == 0;      // and the position's background: decided per workgroup
  const bool owords = (((uintptr_t)out) & 3) == 0 && ((flags & 1) || tab.dw % 4 == 0);
  const int opt = (int)(flags & 1u) | (words ? kVcWords : 0) | (owords ? kVcOutWords : 0);
  const size_t fb = (size_t)W * H * (yuyv_in ? 2 : 3), ob = (size_t)tab.dw * tab.dh * ((flags & 1) ? 2 : 3);
  for (int n0 = 0; n0 < n; n0 += kMaxGridY) {
    const int nn = n - n0 < kMaxGridY ? n - n0 : kMaxGridY;
    const dim3 grid((unsigned)(ntx * nty), (unsigned)nn);
    const uint8_t* f = frames + (size_t)n0 * fb;
    const uint8_t* m = slot_of ? masks : masks + (size_t)n0 * W * H;
    const int* so = slot_of ? slot_of + n0 : nullptr;
    uint8_t* o = out + (size_t)n0 * ob;
#define BSX_VG(D, Y) vg_mixed_k<D, Y><<<grid, kThreads, 0, s>>>(f, desc + n0, m, so, o, W, H, tab, ntx, opt)
    if (direct) { if (yuyv_in) BSX_VG(true, true); else BSX_VG(true, false); }
    else { if (yuyv_in) BSX_VG(false, true); else BSX_VG(false, false); }
#undef BSX_VG
  }
  return hipGetLastError();
}

hipError_t launch_flip_bgr(const uint8_t* src, uint8_t* dst, int w, int h, int code, int n, hipStream_t s) {
  for (int n0 = 0; n0 < n; n0 += kMaxGridY) {
    const int nn = n - n0 < kMaxGridY ? n - n0 : kMaxGridY;
    flip_bgr_k<<<dim3(blocks_for((long)w * h), nn), kThreads, 0, s>>>(src + (size_t)n0 * w * h * 3, dst + (size_t)n0 * w * h * 3, w, h, code);
  }
  return hipGetLastError();
}

hipError_t launch_bgr_to_yuyv(const uint8_t* bgr, uint8_t* yuyv, int w, int h, int n, hipStream_t s) {
  long pairs = (long)n * w * h / 2;
  yuyv_k<<<blocks_for(pairs), kThreads, 0, s>>>(bgr, reinterpret_cast<uint32_t*>(yuyv), pairs);
  return hipGetLastError();
}

hipError_t launch_yuyv_to_bgr(const uint8_t* yuyv, uint8_t* bgr, int w, int h, int n, hipStream_t s) {
  long pairs = (long)n * w * h / 2;
  yuyv_to_bgr_k<<<blocks_for(pairs), kThreads, 0, s>>>(reinterpret_cast<const uint32_t*>(yuyv), bgr, pairs);
  return hipGetLastError();
}

// bsx_reset_streams: grid row y = listed slot ids[y]; its ofinal bytes -> 0 (the reference leaves them uninitialised, bsx_reset defines 0) and its mask bytes -> 255
// (libbackscrub.cc:248).  A slot's bytes start at any offset (outW * outH need not be a multiple of 4): byte stores, grid-stride — a reset is rare and small.
__global__ __launch_bounds__(kThreads) void reset_slots_k(uint8_t* __restrict__ ofinal, size_t ofinal_bytes, uint8_t* __restrict__ masks, size_t mask_bytes,
                                                        const int* __restrict__ ids) {
  const size_t slot = (size_t)ids[blockIdx.y];
  uint8_t* const o = ofinal + slot * ofinal_bytes;
  uint8_t* const m = masks + slot * mask_bytes;
  const size_t step = (size_t)gridDim.x * kThreads;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < ofinal_bytes; i += step) o[i] = 0;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < mask_bytes; i += step) m[i] = 255;
}
hipError_t launch_reset_slots(uint8_t* ofinal, size_t ofinal_bytes, uint8_t* masks, size_t mask_bytes, const int* ids, int n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (n > kMaxGridY) return hipErrorInvalidValue;
  const size_t most = ofinal_bytes > mask_bytes ? ofinal_bytes : mask_bytes;
  const unsigned bx = (unsigned)std::min<size_t>((most + kThreads - 1) / kThreads, 256);
  reset_slots_k<<<dim3(bx, (unsigned)n), kThreads, 0, s>>>(ofinal, ofinal_bytes, masks, mask_bytes, ids);
  return hipGetLastError();
}

hipError_t launch_fill_u8(uint8_t* p, uint8_t v, size_t bytes, hipStream_t s) {
  return hipMemsetAsync(p, v, bytes, s);
}

// (Both kernels are templates of one instance, launched by the file's last launcher: the compiler emits plain kernels first and instances in the order of their first
//  use, and numbers a file's functions as it emits them.  The numbers appear in the assembly of every function behind; as the last two, these move no other
//  kernel's text, which tools/isa_same.py compares with earlier revisions'.)
namespace {
// ---- bsx_step_batch_vcam_geoms: the back end of the geoms step at the virtual camera's geometry — the persistent masks by mask_geoms_k, then ONE resize pass over
// frame, background and mask taps of every position (vg_geoms_k); no capture-size composite exists.
// mask_tile_k<BLEND = false> per position: mask_tile_geoms_k's prologue and uniform-tile branch (class byte first, class record and descriptor as two independent
// uniform loads), then mask_tile.inc without the composite.  Writes the position's persistent mask only: frame, background and output pointers are not read.
template <int = 0>
__global__ __launch_bounds__(kThreads) void mask_geoms_k(const GeomClass* __restrict__ classes, const GeomDesc* __restrict__ desc, GeomSpans sp, unsigned xcd_mask,
                                                        const uint8_t* __restrict__ ofinal, int outW, int outH, const uint8_t* __restrict__ tile_class) {
  __shared__ short col_c0[kHW], col_c1[kHW], col_a0[kHW], col_a1[kHW];
  __shared__ short row_r0[kHH], row_r1[kHH], row_b0[kHH], row_b1[kHH];
  __shared__ __attribute__((aligned(16))) uint16_t hq_hs[kMaxSrcRows * kHW > kHH * kTW ? kMaxSrcRows * kHW : kHH * kTW];
  __shared__ __attribute__((aligned(16))) uint8_t up[kHH * kHW + 8];
  uint16_t* const hq = hq_hs;
  uint16_t* const hs = hq_hs;
  uint8_t* const blk = up;
  const int tid = threadIdx.x;
  int g, w0, p0, p1, per;
  geom_span(sp, (int)blockIdx.x, &g, &w0, &p0, &p1, &per);
  unsigned f_, t_;
  xcd_frame_tile_at(blockIdx.x - (unsigned)w0, (unsigned)per, ((xcd_mask >> g) & 1u) ? (unsigned)(p1 - p0) : 0u, &f_, &t_);
  const int n = p0 + (int)f_;                                          // the position (descriptor index)
  int uniform = 0;
  if (tile_class) uniform = tile_class_byte((uintptr_t)tile_class + (size_t)w0 + (size_t)f_ * (size_t)per + (size_t)t_);
  const GeomClass c = classes[g];
  const GeomDescRegs d = geom_desc(desc, n);
  const int W = c.W, H = c.H;
  const Rect4 roi = c.roi, q = c.in_roi;
  const ResizeTab tab = geom_tab(c.up);
  const int tby = (int)t_ / c.ntx, tbx = (int)t_ - tby * c.ntx, tx0 = tbx * kTW, ty0 = tby * kTH;
  TileBlendOperands ops;
  constexpr bool BLEND = false, WH = false, MIX = false, yin = false, early_bg = false;      // mask_tile.inc's names: masks only
  constexpr long bg_stride = 0;
  constexpr int yuyv = 0, sel = -1;
  const uint8_t *const bg = nullptr, *const frames = nullptr;
  uint8_t *const mask = d.mask, *const outp = nullptr;
  if (uniform) {
    tile_vsum5_store<BLEND, WH, MIX>(hq_hs, mask, outp, ops, 0, 0, W, H, roi, tx0, ty0, tid, yuyv, uniform, sel);
    return;
  }
#define BSX_MT_FRAME 0                                               /* the position's own bases: index 0 of each */
#define BSX_MT_SLOT d.slot
#define BSX_MT_MASK_SLOT 0
#include "mask_tile.inc"
#undef BSX_MT_FRAME
#undef BSX_MT_SLOT
#undef BSX_MT_MASK_SLOT
}

// vg_mixed_k per position: a flat grid of `per` output tiles for each of the call's positions (one output size for all of them).  Capture size, table and the choice
// between the staged and the per-tap form come from the record of the position's class (workgroup-uniform, as prep_geoms_k chooses between its two bodies); frame,
// background, mask and output are the position's own pointers, flips and filter switch its descriptor's.  The body is vcam_tile.inc, once per form.
template <int = 0>
__global__ __launch_bounds__(kThreads) void vg_geoms_k(const VgClass* __restrict__ vg, const GeomDesc* __restrict__ desc, GeomSpans sp, int per, int ntx, int opt) {
  const unsigned pn = blockIdx.x / (unsigned)per, tile_ = blockIdx.x - pn * (unsigned)per;
  const int g = geom_class_of_position(sp, (int)pn);
  const VgClass c = vg[g];                                            // (uniform index: scalar loads) — independent of the descriptor's
  const GeomDescRegs d = geom_desc(desc, (int)pn);
  const int W = c.W, H = c.H;
  const ResizeTab tab = geom_tab(c.tab);
  const uint8_t *const frames = d.frame, *const bg = d.bg, *const masks = d.mask;
  uint8_t* const out = d.out;
  if ((W & 3) == 0 && ((((uintptr_t)frames) | ((uintptr_t)masks)) & 3) == 0) opt |= kVcWords;      // launch_vg_mixed's rule, per position
  constexpr bool SEL = true, YIN = false;
  constexpr long bg_stride = 0;
  [[maybe_unused]] const int* const slot_of = nullptr;
#define BSX_VT_TILE tile_
#define BSX_VT_POS 0l                                                /* the position's own bases: index 0 of each */
#define BSX_VT_DESC(fl) fl = d.flags
  if (c.direct) {
    constexpr bool DIRECT = true;
#include "vcam_tile.inc"
  } else {
    constexpr bool DIRECT = false;
#include "vcam_tile.inc"
  }
#undef BSX_VT_TILE
#undef BSX_VT_POS
#undef BSX_VT_DESC
}
}  // namespace

// the front of every vcam geoms back end: [one tile-class launch,] ONE masks-only tile launch over the call's positions (reads no frame)
static void launch_vcam_masks(const GeomClass* classes, const GeomDesc* desc, const GeomSpans& tiles, unsigned xcd_mask, const uint8_t* ofinal, int outW, int outH,
                              uint8_t* tile_class, int n, hipStream_t s) {
  if (tile_class) tile_class_geoms_k<<<dim3((unsigned)n), kThreads, 0, s>>>(classes, desc, tiles, ofinal, outW, outH, tile_class);
  mask_geoms_k<><<<dim3((unsigned)tiles.wg[kMaxGeoms]), kThreads, 0, s>>>(classes, desc, tiles, xcd_mask, ofinal, outW, outH, tile_class);
}

hipError_t launch_vcam_geoms(const GeomClass* classes, const VgClass* vg, const GeomDesc* desc, const GeomSpans& tiles, unsigned xcd_mask, const uint8_t* ofinal, int outW,
                             int outH, uint8_t* tile_class, int out_w, int out_h, int n, hipStream_t s, unsigned flags) {
  if (n <= 0 || tiles.wg[kMaxGeoms] <= 0 || out_w <= 0 || out_h <= 0 || (flags & ~1u) || ((flags & 1) && (out_w & 1))) return hipErrorInvalidValue;
  const int ntx = (out_w + kVW - 1) / kVW, nty = (out_h + kVH - 1) / kVH;
  if ((unsigned long long)ntx * nty * (unsigned long long)n >= (1ull << 31)) return hipErrorInvalidValue;
  launch_vcam_masks(classes, desc, tiles, xcd_mask, ofinal, outW, outH, tile_class, n, s);
  const bool owords = (flags & 1) || out_w % 4 == 0;                   // (every d_out is 4-byte aligned: checked by the caller)
  const int opt = (int)(flags & 1u) | (owords ? kVcOutWords : 0);
  vg_geoms_k<><<<dim3((unsigned)(ntx * nty) * (unsigned)n), kThreads, 0, s>>>(vg, desc, tiles, ntx * nty, ntx, opt);
  return hipGetLastError();
}

// ---- the geoms steps with a frame format per position (BSX_STREAM_YUYV_IN in an item's setting: kGeomYuyvIn in its descriptor) --------------------------------------
// The four kernels above that read a frame, each with the descriptor's format bit — workgroup-uniform, it arrives with the loads geom_desc makes anyway — choosing
// ONCE between the YIN = true and the YIN = false inclusion of the shared body (prep_tile.inc, mask_tile.inc, vcam_tile.inc; outside_mixed_group reads the bit from its
// flags), the way prep_geoms_k chooses between its two table modes.  Kernels of their own, launched only by the launchers below and only for a call with at least one
// YUYV item: a call of BGR items launches prep_geoms_k, mask_tile_geoms_k, outside_roi_geoms_k and vg_geoms_k, the code it always did.  LDS is declared once per
// kernel and shared by its inclusions (an array declared inside each inclusion would be allocated once per inclusion).  Templates used by the file's last launchers
// for the reason given above mask_geoms_k.
namespace {
// prep_geoms_k + prep_fused_k<OUT, true, true> per position.  A YUYV position's class has a linear table and an even ROI column (prep_yuyv_fusable: the host refuses
// the item otherwise), so the format bit alone selects the YIN body.
template <int OUT>
__global__ __launch_bounds__(kThreads) void prep_geoms_fmt_k(const GeomClass* __restrict__ classes, const GeomDesc* __restrict__ desc, GeomSpans sp, float* __restrict__ input,
                                                            uint32_t* __restrict__ input_u8, int inW, int inH, BilateralParams bp, int TW, int TH, int ntx, int nty, int n_frames) {
  __shared__ float lut[768];
  __shared__ uint32_t tile[kPfS * kPfS];
  const int tid = threadIdx.x;
  unsigned f_, t_;
  xcd_frame_tile((unsigned)(ntx * nty), (unsigned)n_frames, &f_, &t_);
  const int g = geom_class_of_position(sp, (int)f_);
  const GeomClass c = classes[g];                                     // (uniform index: scalar loads) — independent of the descriptor's
  const GeomDescRegs d = geom_desc(desc, (int)f_);
  const uint8_t* const frames = d.frame;
  const ResizeTab tab = geom_tab(c.down);
  const int W = c.W, H = c.H;
  const Rect4 roi = c.roi, q = c.in_roi;
  const long n = (long)f_;
#define BSX_PREP_FRAME 0l                                            /* the position's own frame */
  if (d.flags & kGeomYuyvIn) {
    constexpr bool LINEAR = true, YIN = true;
#include "prep_tile.inc"
  } else if (tab.mode == 0 && (W - roi.x) * 3 >= 8) {                 // prep_geoms_k's choice
    constexpr bool LINEAR = true, YIN = false;
#include "prep_tile.inc"
  } else {
    constexpr bool LINEAR = false, YIN = false;
#include "prep_tile.inc"
  }
#undef BSX_PREP_FRAME
}

// mask_tile_geoms_k + mask_tile_k<true, YIN, false, false, true> per position: mask_tile_geoms_k's prologue, then uniform-tile branch and mask_tile.inc once per format
template <int = 0>
__global__ __launch_bounds__(kThreads) void mask_tile_geoms_fmt_k(const GeomClass* __restrict__ classes, const GeomDesc* __restrict__ desc, GeomSpans sp, unsigned xcd_mask,
                                                                 const uint8_t* __restrict__ ofinal, int outW, int outH, const uint8_t* __restrict__ tile_class, int flags) {
  __shared__ short col_c0[kHW], col_c1[kHW], col_a0[kHW], col_a1[kHW];
  __shared__ short row_r0[kHH], row_r1[kHH], row_b0[kHH], row_b1[kHH];
  __shared__ __attribute__((aligned(16))) uint16_t hq_hs[kMaxSrcRows * kHW > kHH * kTW ? kMaxSrcRows * kHW : kHH * kTW];
  __shared__ __attribute__((aligned(16))) uint8_t up[kHH * kHW + 8];
  uint16_t* const hq = hq_hs;
  uint16_t* const hs = hq_hs;
  uint8_t* const blk = up;
  const int tid = threadIdx.x;
  int g, w0, p0, p1, per;
  geom_span(sp, (int)blockIdx.x, &g, &w0, &p0, &p1, &per);
  unsigned f_, t_;
  xcd_frame_tile_at(blockIdx.x - (unsigned)w0, (unsigned)per, ((xcd_mask >> g) & 1u) ? (unsigned)(p1 - p0) : 0u, &f_, &t_);
  const int n = p0 + (int)f_;                                          // the position (descriptor index)
  int uniform = 0;
  if (tile_class) uniform = tile_class_byte((uintptr_t)tile_class + (size_t)w0 + (size_t)f_ * (size_t)per + (size_t)t_);
  const GeomClass c = classes[g];
  const GeomDescRegs d = geom_desc(desc, n);
  const int W = c.W, H = c.H;
  const Rect4 roi = c.roi, q = c.in_roi;
  const ResizeTab tab = geom_tab(c.up);
  const int tby = (int)t_ / c.ntx, tbx = (int)t_ - tby * c.ntx, tx0 = tbx * kTW, ty0 = tby * kTH;
  flags = (flags & ~16) | (int)(d.flags & (kMixFlipH | kMixFlipV));
  const int sel = (d.flags & kMixFilterOff) ? 2 : -1;
  TileBlendOperands ops;
  constexpr bool BLEND = true, WH = false, MIX = true, early_bg = false;      // mask_tile.inc's names: the instantiation, the position's descriptor
  constexpr long bg_stride = 0;
  const uint8_t *const bg = d.bg, *const frames = d.frame;
  uint8_t *const mask = d.mask, *const outp = d.out;
#define BSX_MT_FRAME 0                                               /* the position's own bases: index 0 of each */
#define BSX_MT_SLOT d.slot
#define BSX_MT_MASK_SLOT 0
#define BSX_MT_POSITION                                                                                                        \
    if (uniform) {                                                                                                             \
      tile_load_blend_operands<BLEND, WH, MIX>(ops, bg, bg_stride, frames, 0, W, H, roi, tx0, ty0, tid, uniform, 3, yin, sel); \
      tile_vsum5_store<BLEND, WH, MIX>(hq_hs, mask, outp, ops, 0, 0, W, H, roi, tx0, ty0, tid, yuyv, uniform, sel);            \
      return;                                                                                                                  \
    }
  if (d.flags & kGeomYuyvIn) {
    constexpr bool yin = true;
    const int yuyv = flags | 16;                                       // bit 4: the frame operand arrives as YUYV (tile_vsum5_store)
    BSX_MT_POSITION
#include "mask_tile.inc"
  } else {
    constexpr bool yin = false;
    const int yuyv = flags;
    BSX_MT_POSITION
#include "mask_tile.inc"
  }
#undef BSX_MT_POSITION
#undef BSX_MT_FRAME
#undef BSX_MT_SLOT
#undef BSX_MT_MASK_SLOT
}

// outside_roi_geoms_k with the position's format as bit 4 of the flags outside_mixed_group reads (a filter-off YUYV position's strips are its frame, converted)
template <int = 0>
__global__ __launch_bounds__(kThreads) void outside_roi_geoms_fmt_k(const GeomClass* __restrict__ classes, const GeomDesc* __restrict__ desc, GeomSpans sp, int flags) {
  int g, w0, p0, p1, per;
  geom_span(sp, (int)blockIdx.x, &g, &w0, &p0, &p1, &per);
  const unsigned local = blockIdx.x - (unsigned)w0, pl = local / (unsigned)per, blk = local - pl * (unsigned)per;
  const GeomClass c = classes[g];
  const GeomDescRegs d = geom_desc(desc, p0 + (int)pl);
  outside_mixed_group(blk * kThreads + threadIdx.x, d.bg, d.flags, d.frame, d.out, c.W, c.H, c.roi, (flags & ~16) | ((d.flags & kGeomYuyvIn) ? 16 : 0));
}

// vg_geoms_k + vg_mixed_k<DIRECT, YIN> per position: vcam_tile.inc once per (form, format), one staging area for all four
template <int = 0>
__global__ __launch_bounds__(kThreads) void vg_geoms_fmt_k(const VgClass* __restrict__ vg, const GeomDesc* __restrict__ desc, GeomSpans sp, int per, int ntx, int opt) {
  __shared__ uint32_t s_px[kVLdsWords];
  const unsigned pn = blockIdx.x / (unsigned)per, tile_ = blockIdx.x - pn * (unsigned)per;
  const int g = geom_class_of_position(sp, (int)pn);
  const VgClass c = vg[g];                                            // (uniform index: scalar loads) — independent of the descriptor's
  const GeomDescRegs d = geom_desc(desc, (int)pn);
  const int W = c.W, H = c.H;
  const ResizeTab tab = geom_tab(c.tab);
  const uint8_t *const frames = d.frame, *const bg = d.bg, *const masks = d.mask;
  uint8_t* const out = d.out;
  if ((W & 3) == 0 && ((((uintptr_t)frames) | ((uintptr_t)masks)) & 3) == 0) opt |= kVcWords;      // launch_vg_mixed's rule (the same for both formats), per position
  constexpr bool SEL = true;
  constexpr long bg_stride = 0;
  [[maybe_unused]] const int* const slot_of = nullptr;
#define BSX_VT_OWN_LDS
#define BSX_VT_TILE tile_
#define BSX_VT_POS 0l                                                /* the position's own bases: index 0 of each */
#define BSX_VT_DESC(fl) fl = d.flags
  if (d.flags & kGeomYuyvIn) {
    constexpr bool YIN = true;
    if (c.direct) {
      constexpr bool DIRECT = true;
#include "vcam_tile.inc"
    } else {
      constexpr bool DIRECT = false;
#include "vcam_tile.inc"
    }
  } else {
    constexpr bool YIN = false;
    if (c.direct) {
      constexpr bool DIRECT = true;
#include "vcam_tile.inc"
    } else {
      constexpr bool DIRECT = false;
#include "vcam_tile.inc"
    }
  }
#undef BSX_VT_OWN_LDS
#undef BSX_VT_TILE
#undef BSX_VT_POS
#undef BSX_VT_DESC
}
}  // namespace

hipError_t launch_prep_geoms_fmt(const GeomClass* classes, const GeomDesc* desc, const GeomSpans& spans, float* input, uint32_t* input_u8, int inW, int inH,
                                 BilateralParams bp, int n, hipStream_t s) {
  if ((!input && !input_u8) || n <= 0) return hipErrorInvalidValue;
  const int ntx = (inW + 31) / 32, nty = (inH + 31) / 32, TW = (inW + ntx - 1) / ntx, TH = (inH + nty - 1) / nty;      // launch_prep_fused's tiles
  if ((unsigned long long)ntx * nty * (unsigned long long)n >= (1ull << 31)) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(ntx * nty) * (unsigned)n);
#define BSX_PG(O) prep_geoms_fmt_k<O><<<grid, kThreads, 0, s>>>(classes, desc, spans, input, input_u8, inW, inH, bp, TW, TH, ntx, nty, xcd_frames(n))
  if (input && input_u8) BSX_PG(3); else if (input_u8) BSX_PG(2); else BSX_PG(1);
#undef BSX_PG
  return hipGetLastError();
}

hipError_t launch_mask_blend_geoms_fmt(const GeomClass* classes, const GeomDesc* desc, const GeomSpans& tiles, unsigned xcd_mask, const GeomSpans& outside,
                                       const uint8_t* ofinal, int outW, int outH, uint8_t* tile_class, int n, hipStream_t s, int flags) {
  flags &= 1 | 8;
  if (n <= 0 || tiles.wg[kMaxGeoms] <= 0) return hipErrorInvalidValue;
  if (outside.wg[kMaxGeoms] > 0) outside_roi_geoms_fmt_k<><<<dim3((unsigned)outside.wg[kMaxGeoms]), kThreads, 0, s>>>(classes, desc, outside, flags);
  if (tile_class) tile_class_geoms_k<<<dim3((unsigned)n), kThreads, 0, s>>>(classes, desc, tiles, ofinal, outW, outH, tile_class);
  flags |= tile_debug_bits() & 128;
  mask_tile_geoms_fmt_k<><<<dim3((unsigned)tiles.wg[kMaxGeoms]), kThreads, 0, s>>>(classes, desc, tiles, xcd_mask, ofinal, outW, outH, tile_class, flags);
  return hipGetLastError();
}

hipError_t launch_vcam_geoms_fmt(const GeomClass* classes, const VgClass* vg, const GeomDesc* desc, const GeomSpans& tiles, unsigned xcd_mask, const uint8_t* ofinal,
                                 int outW, int outH, uint8_t* tile_class, int out_w, int out_h, int n, hipStream_t s, unsigned flags) {
  if (n <= 0 || tiles.wg[kMaxGeoms] <= 0 || out_w <= 0 || out_h <= 0 || (flags & ~1u) || ((flags & 1) && (out_w & 1))) return hipErrorInvalidValue;
  const int ntx = (out_w + kVW - 1) / kVW, nty = (out_h + kVH - 1) / kVH;
  if ((unsigned long long)ntx * nty * (unsigned long long)n >= (1ull << 31)) return hipErrorInvalidValue;
  launch_vcam_masks(classes, desc, tiles, xcd_mask, ofinal, outW, outH, tile_class, n, s);
  const bool owords = (flags & 1) || out_w % 4 == 0;                   // (every d_out is 4-byte aligned: checked by the caller)
  const int opt = (int)(flags & 1u) | (owords ? kVcOutWords : 0);
  vg_geoms_fmt_k<><<<dim3((unsigned)(ntx * nty) * (unsigned)n), kThreads, 0, s>>>(vg, desc, tiles, ntx * nty, ntx, opt);
  return hipGetLastError();
}

// ---- bsx_gaussian_blur_bgr_batch: n images, each of its own size, blur size and pixel format, in ONE launch ----------------------------------------------------------
// gauss_blur_k's body with everything it takes from its kernel arguments read per position: a ragged grid of 64 x 16 tiles (GeomSpans: the positions ordered by image
// size, per = tiles of one image), the position's BlurDesc by two uniform loads, its coefficient record from the context's device table by a uniform index — the
// words stay in SGPRs, as gauss_blur_k's kernel arguments do.  Decided per workgroup, on scalars:
//   * staging: the 4-pixel word path under gauss_blur_k's `xin` rule (rows dword aligned, the tile's source columns inside the image; sh = (-r) & 3), else the
//     reflecting byte path (sh = 0) — the coefficient record follows (two records per blur size, blur_coef_index);
//   * NT = ceil((ksize + 3 + sh) / 4): one of eight straight-line bodies (blur_passes<NT>), the way prep_geoms_k chooses its table mode;
//   * output: whole dwords from the packed LDS tile (MODE 1's form) where w % 4 == 0 and dst is 4-byte aligned, else byte stores from the vertical pass (MODE 0's);
//   * a YUYV position (kGeomYuyvIn) converts as it stages, yuyv_to_bgr_k's integers: on the word path a 4-pixel group is two whole macropixels (the planes start on
//     a multiple of 4 columns), on the byte path pixel gx takes U and V from the macropixel of gx & ~1 after the reflection;
//   * ksize 1 is the image itself (the conversion for a YUYV position): stored straight from the loaded pixels, no LDS.
// A template of one instance launched by the file's last launcher for the reason given above mask_geoms_k.
__host__ __device__ constexpr int blur_coef_index(int ksize, bool words) { return (ksize & ~1) | (words ? 1 : 0); }      // ksize odd, 1 .. 31: records 0 .. 31
namespace {
struct BlurDescRegs { const uint8_t* src; uint8_t* dst; int w, h, ksize; unsigned flags; };
__device__ __forceinline__ BlurDescRegs blur_desc(const BlurDesc* __restrict__ desc, int n) {
  const uint4* p = reinterpret_cast<const uint4*>(desc) + 2 * (size_t)n;
  const uint4 a = p[0], b = p[1];
  typedef __attribute__((address_space(1))) uint8_t* gp;
  BlurDescRegs d;
  d.src = (const uint8_t*)(gp)(((uint64_t)a.y << 32) | a.x);
  d.dst = (uint8_t*)(gp)(((uint64_t)a.w << 32) | a.z);
  d.w = (int)b.x; d.h = (int)b.y; d.ksize = (int)b.z; d.flags = b.w;
  return d;
}
// pixel (gx, gy) of a position's image as B | G << 8 | R << 16: byte loads, any alignment (vcam_frame_px with the format as a run-time, workgroup-uniform bit)
__device__ __forceinline__ uint32_t blur_src_px(const uint8_t* __restrict__ in, bool yin, int W, int gx, int gy) {
  if (yin) {
    const uint8_t* q = in + (unsigned)(gy * W + (gx & ~1)) * 2u;
    return yuv_tap_to_bgr((uint32_t)q[(gx & 1) * 2] | ((uint32_t)q[1] << 8) | ((uint32_t)q[3] << 16));
  }
  const uint8_t* p = in + (unsigned)(gy * W + gx) * 3u;
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
}
// gauss_blur_k's passes 2 and 3 for one NT, the coefficient words copied out of the record first (uniform address, constant offsets: scalar loads)
// USER: not read.  Each kernel that takes the passes names its own instances (blur_surfaces_k: 1): an instance inlined at one place only keeps blur_batch_k's code what
// it was (with two callers of one instance the compiler emitted another, longer blur_batch_k: tools/isa_same.py).
template <int NT, int USER = 0>
__device__ __forceinline__ void blur_passes(uint8_t* s_src, uint16_t* s_h, const GaussCoef* __restrict__ gc, int SH, bool owords, uint8_t* __restrict__ out, int W, int H,
                                            int x0, int y0) {
  static_assert(NT >= 2 && NT <= 9, "tap words of the horizontal pass");
  constexpr int NP = 2 * NT - 1;
  uint32_t c4[4][NT], c2[2][NP];
#pragma unroll
  for (int j = 0; j < 4; j++)
#pragma unroll
    for (int t = 0; t < NT; t++) c4[j][t] = gc->c4[j][t];
#pragma unroll
  for (int h = 0; h < 2; h++)
#pragma unroll
    for (int t = 0; t < NP; t++) c2[h][t] = gc->c2[h][t];
  __syncthreads();                                                    // the staged tile is complete (the coefficient loads above are in flight while the waves meet)
  // horizontal pass: item = (plane, source row, group of 4 output columns)
  for (int grp = threadIdx.x & 15, row = threadIdx.x >> 4, plane = 0; plane < 3;) {
    const uint32_t* rowp = reinterpret_cast<const uint32_t*>(s_src + (plane * kGSH + row) * kGSrcStride) + grp;
    uint32_t d[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) d[t] = rowp[t];                           // stays inside the 96-byte row: 4 * (15 + NT) <= 96
    uint32_t acc[4] = {0, 0, 0, 0};
#pragma unroll
    for (int t = 0; t < NT; t++) {
#pragma unroll
      for (int j = 0; j < 4; j++) acc[j] = __builtin_amdgcn_udot4(d[t], c4[j][t], acc[j], false);
    }
#pragma unroll
    for (int j = 0; j < 4; j++) s_h[gh_col(plane, 4 * grp + j) + row] = (uint16_t)acc[j];
    row += kGTH;
    if (row >= SH) { row -= SH; plane++; }
  }
  __syncthreads();
  // vertical pass: item = (plane, output column, pair of output rows)
  for (int i = threadIdx.x; i < 3 * kGTW * (kGTH / 2); i += kThreads) {
    const int m = i & (kGTH / 2 - 1), pc = i / (kGTH / 2), col = pc & (kGTW - 1), plane = pc / kGTW;
    const uint32_t* colp = reinterpret_cast<const uint32_t*>(s_h + gh_col(plane, col)) + m;
    uint32_t hd[NP];
#pragma unroll
    for (int t = 0; t < NP; t++) hd[t] = colp[t];                          // 2 (m + NP - 1) + 1 <= 47 < kGHStride
    uint32_t a0 = 0, a1 = 0;
#pragma unroll
    for (int t = 0; t < NP; t++) {
      a0 = __builtin_amdgcn_udot2(__builtin_bit_cast(us2v, hd[t]), __builtin_bit_cast(us2v, c2[0][t]), a0, false);
      a1 = __builtin_amdgcn_udot2(__builtin_bit_cast(us2v, hd[t]), __builtin_bit_cast(us2v, c2[1][t]), a1, false);
    }
    const uint8_t v0 = (uint8_t)min((a0 + (1u << 15)) >> 16, 255u), v1 = (uint8_t)min((a1 + (1u << 15)) >> 16, 255u);
    if (owords) {
      s_src[(2 * m) * kGOStride + 3 * col + plane] = v0;
      s_src[(2 * m + 1) * kGOStride + 3 * col + plane] = v1;
    } else {
      const int gx = x0 + col, gy = y0 + 2 * m;
      if (gx < W) {
        if (gy < H) out[(unsigned)(gy * W + gx) * 3u + plane] = v0;
        if (gy + 1 < H) out[(unsigned)((gy + 1) * W + gx) * 3u + plane] = v1;
      }
    }
  }
}

template <int = 0>
__global__ __launch_bounds__(kThreads) void blur_batch_k(const BlurDesc* __restrict__ desc, const GaussCoef* __restrict__ coef, GeomSpans sp, BlurTileCols cols) {
  __shared__ __attribute__((aligned(16))) uint8_t s_src[3 * kGSH * kGSrcStride];          // [plane][row][col]; whole-dword output: later the packed tile [row][kGOStride]
  __shared__ __attribute__((aligned(16))) uint16_t s_h[3 * kGHPlane];                     // [plane][col][row], gh_col()
  int g, w0, p0, p1, per;
  geom_span(sp, (int)blockIdx.x, &g, &w0, &p0, &p1, &per);
  const unsigned local = blockIdx.x - (unsigned)w0, pl = local / (unsigned)per, tile = local - pl * (unsigned)per;
  const BlurDescRegs d = blur_desc(desc, p0 + (int)pl);
  const int W = d.w, H = d.h, r = d.ksize >> 1;
  const bool yin = (d.flags & kGeomYuyvIn) != 0;
  const uint8_t* __restrict__ const in = d.src;
  uint8_t* __restrict__ const out = d.dst;
  // the class's tiles per image row travel with the spans (selected on SGPRs as geom_span selects, nothing loaded): the tile's coordinates do not wait for the
  // descriptor's width
  unsigned ntx = (unsigned)cols.ntx[0];
#pragma unroll
  for (int k = 1; k < kMaxGeoms; k++) if (g == k) ntx = (unsigned)cols.ntx[k];
  const unsigned ty = tile / ntx, tx = tile - ty * ntx;
  const int x0 = (int)tx * kGTW, y0 = (int)ty * kGTH;
  if (r == 0) {                                                       // ksize 1: the (converted) pixels themselves
    for (int i = threadIdx.x; i < kGTW * kGTH; i += kThreads) {
      const int gx = x0 + (i & (kGTW - 1)), gy = y0 + i / kGTW;
      if (gx < W && gy < H) {
        const uint32_t px = blur_src_px(in, yin, W, gx, gy);
        uint8_t* o = out + (unsigned)(gy * W + gx) * 3u;
        o[0] = (uint8_t)px; o[1] = (uint8_t)(px >> 8); o[2] = (uint8_t)(px >> 16);
      }
    }
    return;
  }
  const int SW = kGTW + 2 * r, SH = kGTH + 2 * r;                     // live part of the source tile
  // 1. stage + de-interleave (reflected at the image border): gauss_blur_k's two paths, the choice and its sh made here
  const bool rows4 = yin || (((W & 3) | (int)((uintptr_t)in & 3)) == 0);      // a YUYV image has an even width and a 4-byte aligned base (checked by the caller)
  const int shw = (-r) & 3, Gw = (SW + shw + 3) >> 2;
  const bool xin = rows4 && x0 - r - shw >= 0 && x0 - r - shw + 4 * Gw <= W;
  const int sh = xin ? shw : 0;
  if (xin) {                                                          // item = (row, group of 4 pixels) → one dword per plane
    const int G = Gw;
    int row = (int)threadIdx.x / G, grp = (int)threadIdx.x - row * G;
    const int dr = kThreads / G, dc = kThreads - dr * G;
    const unsigned xb = (unsigned)(x0 - r - sh);
    while (row < SH) {
      const int gy = reflect101_far(y0 - r + row, H);
      uint32_t pb, pg, pr;
      if (yin) {                                                      // two macropixels: Y0 U0 Y1 V0 | Y2 U1 Y3 V1
        const uint32_t* p = reinterpret_cast<const uint32_t*>(in + ((unsigned)(gy * W) + xb + 4u * (unsigned)grp) * 2u);
        const uint32_t q0 = p[0], q1 = p[1];
        int bu0, gu0, ru0, bu1, gu1, ru1;
        yuv_chroma((int)((q0 >> 8) & 255u) - 128, (int)(q0 >> 24) - 128, &bu0, &gu0, &ru0);
        yuv_chroma((int)((q1 >> 8) & 255u) - 128, (int)(q1 >> 24) - 128, &bu1, &gu1, &ru1);
        const int ya = yuv_luma(q0 & 255u), yb = yuv_luma((q0 >> 16) & 255u), yc = yuv_luma(q1 & 255u), yd = yuv_luma((q1 >> 16) & 255u);
        pb = (sat_pk2_shr20(ya + bu0, yb + bu0) & 0xffffu) | (sat_pk2_shr20(yc + bu1, yd + bu1) << 16);
        pg = (sat_pk2_shr20(ya + gu0, yb + gu0) & 0xffffu) | (sat_pk2_shr20(yc + gu1, yd + gu1) << 16);
        pr = (sat_pk2_shr20(ya + ru0, yb + ru0) & 0xffffu) | (sat_pk2_shr20(yc + ru1, yd + ru1) << 16);
      } else {
        const uint32_t* p = reinterpret_cast<const uint32_t*>(in + ((unsigned)(gy * W) + xb + 4u * (unsigned)grp) * 3u);
        const uint32_t d0 = p[0], d1 = p[1], d2 = p[2];               // B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3
        pb = __builtin_amdgcn_perm(d2, __builtin_amdgcn_perm(d1, d0, 0x00060300u), 0x05020100u);
        pg = __builtin_amdgcn_perm(d2, __builtin_amdgcn_perm(d1, d0, 0x00070401u), 0x06020100u);
        pr = __builtin_amdgcn_perm(d2, __builtin_amdgcn_perm(d1, d0, 0x00000502u), 0x07040100u);
      }
      uint32_t* o = reinterpret_cast<uint32_t*>(s_src + row * kGSrcStride) + grp;
      o[0] = pb; o[kGSH * kGSrcStride / 4] = pg; o[2 * kGSH * kGSrcStride / 4] = pr;
      grp += dc; row += dr;
      if (grp >= G) { grp -= G; row++; }
    }
  } else {
    int row = (int)threadIdx.x / SW, col = (int)threadIdx.x - row * SW;
    const int dr = kThreads / SW, dc = kThreads - dr * SW;
    while (row < SH) {
      const int gy = reflect101_far(y0 - r + row, H), gx = reflect101_far(x0 - r + col, W);
      const uint32_t px = blur_src_px(in, yin, W, gx, gy);
      s_src[(0 * kGSH + row) * kGSrcStride + col] = (uint8_t)px;
      s_src[(1 * kGSH + row) * kGSrcStride + col] = (uint8_t)(px >> 8);
      s_src[(2 * kGSH + row) * kGSrcStride + col] = (uint8_t)(px >> 16);
      col += dc; row += dr;
      if (col >= SW) { col -= SW; row++; }
    }
  }
  // 2. + 3. the passes: NT = ceil((ksize + 3 + sh) / 4), a workgroup-uniform choice between straight-line bodies (each begins with the barrier behind the staging)
  const bool owords = (((W & 3) | (int)((uintptr_t)out & 3)) == 0);
  const GaussCoef* __restrict__ const gc = coef + blur_coef_index(d.ksize, xin);
  switch ((d.ksize + sh + 6) >> 2) {
#define BSX_BB(NT) case NT: blur_passes<NT>(s_src, s_h, gc, SH, owords, out, W, H, x0, y0); break;
    BSX_BB(2) BSX_BB(3) BSX_BB(4) BSX_BB(5) BSX_BB(6) BSX_BB(7) BSX_BB(8) default: BSX_BB(9)
#undef BSX_BB
  }
  if (owords) {                                                       // this lane's 4-pixel group of the packed tile: three whole dwords
    __syncthreads();
    const int orow = threadIdx.x >> 4, ogx = x0 + 4 * (threadIdx.x & 15), ogy = y0 + orow;
    if (ogx < W && ogy < H) {
      const uint32_t* bp = reinterpret_cast<const uint32_t*>(s_src + orow * kGOStride + 12 * (threadIdx.x & 15));
      uint32_t* op = reinterpret_cast<uint32_t*>(out + (unsigned)(ogy * W + ogx) * 3u);
      op[0] = bp[0]; op[1] = bp[1]; op[2] = bp[2];
    }
  }
}
}  // namespace

// The device table bsx_gaussian_blur_bgr_batch uploads once: record blur_coef_index(ksize, words) for every odd ksize of 1 .. 31 and both staging paths.
size_t blur_coef_table_bytes() { return (size_t)(2 * kGMaxR + 2) * sizeof(GaussCoef); }
void blur_coef_table(GaussCoef* tab) {
  for (int k = 1; k <= 2 * kGMaxR + 1; k += 2)
    for (int words = 0; words < 2; words++) (void)gauss_coefficients(k, tab + blur_coef_index(k, words != 0), words ? (-(k / 2)) & 3 : 0);
}

hipError_t launch_blur_batch(const BlurDesc* desc, const GaussCoef* coef, const GeomSpans& spans, const BlurTileCols& cols, hipStream_t s) {
  if (!desc || !coef || spans.wg[kMaxGeoms] <= 0) return hipErrorInvalidValue;
  for (int g = 0; g < kMaxGeoms; g++) if (spans.per[g] > 0 && (cols.ntx[g] <= 0 || spans.per[g] % cols.ntx[g])) return hipErrorInvalidValue;
  blur_batch_k<><<<dim3((unsigned)spans.wg[kMaxGeoms]), kThreads, 0, s>>>(desc, coef, spans, cols);
  return hipGetLastError();
}

// ---- the geoms step for classes off the 4-pixel grid (kernels.hpp: launch_mask_blend_geoms_edge) -------------------------------------------------------------------
// tile_class_geoms_k, mask_tile_geoms_fmt_k and outside_roi_geoms_fmt_k with the 4-pixel groups of the composite anchored to the frame.  A lane's group at ROI-relative
// column gx = 128 tbx - (roi.x & 3) + 4 k is three aligned dwords of a frame whose width is a multiple of 4 (two for a YUYV frame), mirrors to an aligned group under
// a horizontal flip and holds whole YUYV pairs; it may reach up to three columns outside the ROI on either side.  Kernels of their own at the end of the file (the
// reason is given above mask_geoms_k), launched only for a call that touches such a class.
namespace {
// 0xFF in byte j where pixel gx + j of a group lies outside the ROI's columns [0, roi_w): those pixels have mask 255 by definition.  gx >= -3 and gx < roi_w.
__device__ __forceinline__ uint32_t edge_outside_bytes(int gx, int roi_w) {
  const int l = max(-gx, 0), r = min(roi_w - gx, 4);                  // the group's pixels inside the ROI are [l, r)
  return (l ? (1u << (8 * l)) - 1u : 0u) | (r < 4 ? 0xFFFFFFFFu << (8 * r) : 0u);
}
// tile_load_blend_operands<true, false, true> for one position's own images (index 0, no stride), every group the tile launch owns: those with a pixel inside the ROI.
// A filter-off position (sel = 2) has no background; a uniform-0 tile (frame only) still reads the background of a straddling group, whose pixels outside the ROI
// are the background's.
__device__ __forceinline__ void tile_load_blend_operands_edge(TileBlendOperands& o, const uint8_t* __restrict__ bg, const uint8_t* __restrict__ frame, int W, Rect4 roi,
                                                              int tx0, int ty0, int tid, int uniform, bool yin, int sel) {
  const int take = sel >= 0 ? sel : uniform;
  const int ly0 = tid / (kTW / 4), gx = tx0 + (tid % (kTW / 4)) * 4;
  const long pix0 = (long)(roi.y + ty0 + ly0) * W + roi.x + gx;        // frame coordinates: roi.x + gx is a multiple of 4 inside [0, W - 4] for every owned group
  const int fb = yin ? 2 : 3;
  const bool straddles = gx < 0 || gx + 3 >= roi.w;
  const bool need_a = take != 2 || (sel < 0 && straddles), need_b = take != 1;
  const uint8_t* const a0 = bg + pix0 * 3;
  const uint8_t* const b0 = frame + pix0 * fb;
#pragma unroll
  for (int i = 0; i < kTileItems; i++) {
    o.a[i][0] = o.a[i][1] = o.a[i][2] = 0;
    o.b[i][0] = o.b[i][1] = o.b[i][2] = 0;
    if (ty0 + ly0 + 8 * i < roi.h && gx < roi.w) {                     // (gx + 3 >= 0 always: tx0 >= -3)
      const uint32_t* ap = reinterpret_cast<const uint32_t*>(a0 + (long)(8 * i) * W * 3);
      const uint32_t* bp = reinterpret_cast<const uint32_t*>(b0 + (long)(8 * i) * W * fb);
      if (need_a) { o.a[i][0] = ap[0]; o.a[i][1] = ap[1]; o.a[i][2] = ap[2]; }
      if (need_b) {
        o.b[i][0] = __builtin_nontemporal_load(bp); o.b[i][1] = __builtin_nontemporal_load(bp + 1);
        if (!yin) o.b[i][2] = __builtin_nontemporal_load(bp + 2);
      }
    }
  }
}
// tile_vsum5_store<true, false, true> likewise: the mask bytes of the group's pixels outside the ROI become 255 in registers — so the blend gives them the background
// exactly ((a * 255 + b * 0) / 255 == a) — and only the bytes inside the ROI are stored: the persistent mask outside the ROI stays what reset made it.
__device__ __forceinline__ void tile_vsum5_store_edge(const uint16_t* hs, uint8_t* __restrict__ mask, uint8_t* __restrict__ outp, const TileBlendOperands& o, int W, int H,
                                                      Rect4 roi, int tx0, int ty0, int tid, int yuyv_flip, int uniform, int sel) {
  const int take = sel >= 0 ? sel : uniform;
  const int ly0 = tid / (kTW / 4), lx = (tid % (kTW / 4)) * 4;
  const int gx = tx0 + lx;
  if (gx >= roi.w) return;                                             // a group right of the ROI: the outside launch's
  const uint32_t outside = edge_outside_bytes(gx, roi.w);
  const int yuyv = yuyv_flip & 1;
  const bool fh = (yuyv_flip & 2) != 0, fv = (yuyv_flip & 4) != 0, yin = (yuyv_flip & 16) != 0;
  const int obpp = yuyv ? 2 : 3;
  uint8_t* const dst0 = mask + (long)(roi.y + ty0 + ly0) * W + roi.x + gx;
  const int oy0 = fv ? H - 1 - (roi.y + ty0 + ly0) : roi.y + ty0 + ly0, ox = fh ? W - 4 - (roi.x + gx) : roi.x + gx;
  const long orow = fv ? -(long)W : (long)W;
  uint8_t* const out0 = outp + ((long)oy0 * W + ox) * obpp;
#pragma unroll
  for (int i = 0; i < kTileItems; i++) {
    const int ly = ly0 + 8 * i, gy = ty0 + ly;
    if (gy >= roi.h) continue;
    uint32_t packed = uniform == 1 ? 0xFFFFFFFFu : 0u;
    if (!uniform) {
      uint2 acc = *reinterpret_cast<const uint2*>(&hs[ly * kTW + lx]);
#pragma unroll
      for (int r = 1; r < 5; r++) {
        const uint2 v = *reinterpret_cast<const uint2*>(&hs[(ly + r) * kTW + lx]);
        acc.x = __builtin_bit_cast(uint32_t, __builtin_bit_cast(us2, acc.x) + __builtin_bit_cast(us2, v.x));
        acc.y = __builtin_bit_cast(uint32_t, __builtin_bit_cast(us2, acc.y) + __builtin_bit_cast(us2, v.y));
      }
      const uint32_t m0 = (__umul24(acc.x & 0xffffu, 5243u) + 12u * 5243u) >> 17, m1 = (__umul24(acc.x >> 16, 5243u) + 12u * 5243u) >> 17;
      const uint32_t m2 = (__umul24(acc.y & 0xffffu, 5243u) + 12u * 5243u) >> 17, m3 = (__umul24(acc.y >> 16, 5243u) + 12u * 5243u) >> 17;
      packed = m0 | (m1 << 8) | (m2 << 16) | (m3 << 24);
    }
    packed |= outside;
    uint8_t* dst = dst0 + (long)(8 * i) * W;
    if (yuyv_flip & 8) { /* composite only (BSX_STEP_NO_MASK) */ }
    else if (outside == 0 && ((uintptr_t)dst & 3) == 0) *reinterpret_cast<uint32_t*>(dst) = packed;
    else for (int j = 0; j < 4; j++) if (!((outside >> (8 * j)) & 255u)) dst[j] = (uint8_t)(packed >> (8 * j));
    uint32_t* op = reinterpret_cast<uint32_t*>(out0 + (long)(8 * i) * orow * obpp);
    uint32_t o3[3];
    if (take == 1) { o3[0] = o.a[i][0]; o3[1] = o.a[i][1]; o3[2] = o.a[i][2]; }
    else if (take == 2 && (sel >= 0 || outside == 0)) tile_frame_bgr(o, i, yin, o3);
    else { uint32_t b3[3]; tile_frame_bgr(o, i, yin, b3); blend_quad(o.a[i], b3, packed, o3); }      // (a uniform-0 tile's straddling group: packed = outside)
    if (fh) reverse4px(o3);
    if (yuyv) {
      __builtin_nontemporal_store(yuyv_pair(o3[0] & 255u, (o3[0] >> 8) & 255u, (o3[0] >> 16) & 255u, o3[0] >> 24, o3[1] & 255u, (o3[1] >> 8) & 255u), op);
      __builtin_nontemporal_store(yuyv_pair((o3[1] >> 16) & 255u, o3[1] >> 24, o3[2] & 255u, (o3[2] >> 8) & 255u, (o3[2] >> 16) & 255u, o3[2] >> 24), op + 1);
    } else {
      __builtin_nontemporal_store(u3v{o3[0], o3[1], o3[2]}, reinterpret_cast<u3v*>(op));
    }
  }
}

// tile_class_geoms_k over the frame-anchored tile columns: the class byte of the tile mask_tile_geoms_edge_k works on
template <int = 0>
__global__ __launch_bounds__(kThreads) void tile_class_geoms_edge_k(const GeomClass* __restrict__ classes, const GeomDesc* __restrict__ desc, GeomSpans sp,
                                                                   const uint8_t* __restrict__ ofinal, int outW, int outH, uint8_t* __restrict__ tile_class) {
  const int n = blockIdx.x, g = geom_class_of_position(sp, n);
  const GeomClass c = classes[g];
  const int slot = geom_desc(desc, n).slot;
  uint8_t* const cls = tile_class + sp.wg[g] + (size_t)(n - sp.pos[g]) * (size_t)(c.ntx * c.nty);
  const ResizeTab tab = geom_tab(c.up);
  if (c.ntx > kClsMaxTx || tab.sh * c.ntx > kClsMaxItems) {           // out of the classifier's range (launch_tile_class): all general
    for (int t = threadIdx.x; t < c.ntx * c.nty; t += kThreads) cls[t] = 0;
    return;
  }
  const int tid = threadIdx.x, ntx = c.ntx, nty = c.nty;
  const Rect4 roi = c.roi;
#define BSX_CLS_FRAME ofinal + (long)slot * outW * outH + (long)c.in_roi.y * outW + c.in_roi.x
#define BSX_CLS_BYTE(t) cls[t]
#define BSX_CLS_SHIFT geom_edge_shift(roi)
#include "tile_class.inc"
#undef BSX_CLS_FRAME
#undef BSX_CLS_BYTE
#undef BSX_CLS_SHIFT
}

// mask_tile_geoms_fmt_k with tx0 = 128 tbx - (roi.x & 3) and the *_edge operands and stores: uniform-tile branch and mask_tile.inc once per format
template <int = 0>
__global__ __launch_bounds__(kThreads) void mask_tile_geoms_edge_k(const GeomClass* __restrict__ classes, const GeomDesc* __restrict__ desc, GeomSpans sp, unsigned xcd_mask,
                                                                  const uint8_t* __restrict__ ofinal, int outW, int outH, const uint8_t* __restrict__ tile_class, int flags) {
  __shared__ short col_c0[kHW], col_c1[kHW], col_a0[kHW], col_a1[kHW];
  __shared__ short row_r0[kHH], row_r1[kHH], row_b0[kHH], row_b1[kHH];
  __shared__ __attribute__((aligned(16))) uint16_t hq_hs[kMaxSrcRows * kHW > kHH * kTW ? kMaxSrcRows * kHW : kHH * kTW];
  __shared__ __attribute__((aligned(16))) uint8_t up[kHH * kHW + 8];
  uint16_t* const hq = hq_hs;
  uint16_t* const hs = hq_hs;
  uint8_t* const blk = up;
  const int tid = threadIdx.x;
  int g, w0, p0, p1, per;
  geom_span(sp, (int)blockIdx.x, &g, &w0, &p0, &p1, &per);
  unsigned f_, t_;
  xcd_frame_tile_at(blockIdx.x - (unsigned)w0, (unsigned)per, ((xcd_mask >> g) & 1u) ? (unsigned)(p1 - p0) : 0u, &f_, &t_);
  const int n = p0 + (int)f_;                                          // the position (descriptor index)
  int uniform = 0;
  if (tile_class) uniform = tile_class_byte((uintptr_t)tile_class + (size_t)w0 + (size_t)f_ * (size_t)per + (size_t)t_);
  const GeomClass c = classes[g];
  const GeomDescRegs d = geom_desc(desc, n);
  const int W = c.W, H = c.H;
  const Rect4 roi = c.roi, q = c.in_roi;
  const ResizeTab tab = geom_tab(c.up);
  const int tby = (int)t_ / c.ntx, tbx = (int)t_ - tby * c.ntx, tx0 = tbx * kTW - geom_edge_shift(roi), ty0 = tby * kTH;
  flags = (flags & ~16) | (int)(d.flags & (kMixFlipH | kMixFlipV));
  const int sel = (d.flags & kMixFilterOff) ? 2 : -1;
  TileBlendOperands ops;
  const uint8_t *const bg = d.bg, *const frames = d.frame;
  uint8_t *const mask = d.mask, *const outp = d.out;
#define BSX_MT_EDGE
#define BSX_MT_SLOT d.slot
#define BSX_MT_POSITION                                                                            \
    if (uniform) {                                                                                 \
      tile_load_blend_operands_edge(ops, bg, frames, W, roi, tx0, ty0, tid, uniform, yin, sel);    \
      tile_vsum5_store_edge(hq_hs, mask, outp, ops, W, H, roi, tx0, ty0, tid, yuyv, uniform, sel); \
      return;                                                                                      \
    }
  if (d.flags & kGeomYuyvIn) {
    constexpr bool yin = true;
    const int yuyv = flags | 16;                                       // bit 4: the frame operand arrives as YUYV (tile_vsum5_store_edge)
    BSX_MT_POSITION
#include "mask_tile.inc"
  } else {
    constexpr bool yin = false;
    const int yuyv = flags;
    BSX_MT_POSITION
#include "mask_tile.inc"
  }
#undef BSX_MT_POSITION
#undef BSX_MT_SLOT
#undef BSX_MT_EDGE
}

// outside_roi_geoms_fmt_k for the groups wholly outside the ROI
template <int = 0>
__global__ __launch_bounds__(kThreads) void outside_roi_geoms_edge_k(const GeomClass* __restrict__ classes, const GeomDesc* __restrict__ desc, GeomSpans sp, int flags) {
  int g, w0, p0, p1, per;
  geom_span(sp, (int)blockIdx.x, &g, &w0, &p0, &p1, &per);
  const unsigned local = blockIdx.x - (unsigned)w0, pl = local / (unsigned)per, blk = local - pl * (unsigned)per;
  const GeomClass c = classes[g];
  const GeomDescRegs d = geom_desc(desc, p0 + (int)pl);
  outside_mixed_group<true>(blk * kThreads + threadIdx.x, d.bg, d.flags, d.frame, d.out, c.W, c.H, c.roi, (flags & ~16) | ((d.flags & kGeomYuyvIn) ? 16 : 0));
}
}  // namespace

int geom_tile_cols(const Rect4& roi, bool edge) { return ((edge ? geom_edge_shift(roi) : 0) + roi.w + kTW - 1) / kTW; }
bool geom_class_edge_fusable(int W, const Rect4& roi, const ResizeTab& up, bool shifted_tiles_fit) {
  return (W % 4) == 0 && roi.w >= 8 && mask_tile_usable(up) && shifted_tiles_fit;      // (roi.w >= 8: the halo at column -5 reflects inside the ROI)
}

hipError_t launch_mask_blend_geoms_edge(const GeomClass* classes, const GeomDesc* desc, const GeomSpans& tiles, unsigned xcd_mask, const GeomSpans& outside,
                                        const uint8_t* ofinal, int outW, int outH, uint8_t* tile_class, int n, hipStream_t s, int flags) {
  flags &= 1 | 8;
  if (n <= 0 || tiles.wg[kMaxGeoms] <= 0) return hipErrorInvalidValue;
  if (outside.wg[kMaxGeoms] > 0) outside_roi_geoms_edge_k<><<<dim3((unsigned)outside.wg[kMaxGeoms]), kThreads, 0, s>>>(classes, desc, outside, flags);
  if (tile_class) tile_class_geoms_edge_k<><<<dim3((unsigned)n), kThreads, 0, s>>>(classes, desc, tiles, ofinal, outW, outH, tile_class);
  mask_tile_geoms_edge_k<><<<dim3((unsigned)tiles.wg[kMaxGeoms]), kThreads, 0, s>>>(classes, desc, tiles, xcd_mask, ofinal, outW, outH, tile_class, flags);
  return hipGetLastError();
}

// ---- bsx_step_batch_vcam_geoms_outs: several outputs per position, each of its own size, in ONE resize pass (kernels.hpp: VgOutGroup, OutSpans) --------------------
// vg_geoms_k / vg_geoms_fmt_k with a prologue of their own: the grid is ragged over up to 32 (class, size) groups of output records, so group record (capture size,
// table, form, tiles per row, option bits) and descriptor (the position's pointers and flags, `out` the record's) are read per workgroup where vg_geoms_k takes
// per, ntx and opt from its arguments.  The body is vcam_tile.inc, included as there.  Kernels of their own at the end of the file (the reason is given above
// mask_geoms_k): bsx_step_batch_vcam_geoms keeps launching vg_geoms_k.
static_assert(kVcYuyvOut == 1 && kVcOutWords == 16, "VgOutGroup::opt is written by the host (kernels.hpp)");
namespace {
// workgroup `id` of the ragged output grid: its group g, the group's first workgroup w0, first record r0 and workgroups per record — geom_span's compare chain over
// kMaxOutGroups spans (a compare and four selects on SGPRs per span, nothing loaded but the kernel arguments), cut short in steps of eight spans by the call's
// group count (a scalar branch): a call of up to 8 groups pays 7 steps, the simulcast of three classes x three sizes 15, a full call 31
__device__ __forceinline__ void out_span(const OutSpans& sp, int id, int* g, int* w0, int* r0, int* per) {
  *g = 0; *w0 = sp.wg[0]; *r0 = sp.rec[0]; *per = sp.per[0];
#pragma unroll
  for (int b = 0; b < kMaxOutGroups; b += 8) {
    if (b && sp.ng <= b) break;
#pragma unroll
    for (int k = b ? b : 1; k < b + 8; k++)
      if (id >= sp.wg[k]) { *g = k; *w0 = sp.wg[k]; *r0 = sp.rec[k]; *per = sp.per[k]; }
  }
}

template <int = 0>
__global__ __launch_bounds__(kThreads) void vg_outs_k(const VgOutGroup* __restrict__ groups, const GeomDesc* __restrict__ odesc, OutSpans sp) {
  int g, w0, r0, per;
  out_span(sp, (int)blockIdx.x, &g, &w0, &r0, &per);
  const unsigned local = blockIdx.x - (unsigned)w0, rl = local / (unsigned)per, tile_ = local - rl * (unsigned)per;
  const VgOutGroup G = groups[g];                                     // (uniform index: scalar loads) — independent of the descriptor's
  const GeomDescRegs d = geom_desc(odesc, r0 + (int)rl);
  const int W = G.c.W, H = G.c.H, ntx = G.ntx;
  int opt = G.opt;
  const ResizeTab tab = geom_tab(G.c.tab);
  const uint8_t *const frames = d.frame, *const bg = d.bg, *const masks = d.mask;
  uint8_t* const out = d.out;
  if ((W & 3) == 0 && ((((uintptr_t)frames) | ((uintptr_t)masks)) & 3) == 0) opt |= kVcWords;      // launch_vg_mixed's rule, per position
  constexpr bool SEL = true, YIN = false;
  constexpr long bg_stride = 0;
  [[maybe_unused]] const int* const slot_of = nullptr;
#define BSX_VT_TILE tile_
#define BSX_VT_POS 0l                                                /* the record's own bases: index 0 of each */
#define BSX_VT_DESC(fl) fl = d.flags
  if (G.c.direct) {
    constexpr bool DIRECT = true;
#include "vcam_tile.inc"
  } else {
    constexpr bool DIRECT = false;
#include "vcam_tile.inc"
  }
#undef BSX_VT_TILE
#undef BSX_VT_POS
#undef BSX_VT_DESC
}

// vg_outs_k for a call with at least one YUYV item: vg_geoms_fmt_k's choice per (form, format), one staging area for all four inclusions
template <int = 0>
__global__ __launch_bounds__(kThreads) void vg_outs_fmt_k(const VgOutGroup* __restrict__ groups, const GeomDesc* __restrict__ odesc, OutSpans sp) {
  __shared__ uint32_t s_px[kVLdsWords];
  int g, w0, r0, per;
  out_span(sp, (int)blockIdx.x, &g, &w0, &r0, &per);
  const unsigned local = blockIdx.x - (unsigned)w0, rl = local / (unsigned)per, tile_ = local - rl * (unsigned)per;
  const VgOutGroup G = groups[g];                                     // (uniform index: scalar loads) — independent of the descriptor's
  const GeomDescRegs d = geom_desc(odesc, r0 + (int)rl);
  const int W = G.c.W, H = G.c.H, ntx = G.ntx;
  int opt = G.opt;
  const ResizeTab tab = geom_tab(G.c.tab);
  const uint8_t *const frames = d.frame, *const bg = d.bg, *const masks = d.mask;
  uint8_t* const out = d.out;
  if ((W & 3) == 0 && ((((uintptr_t)frames) | ((uintptr_t)masks)) & 3) == 0) opt |= kVcWords;      // launch_vg_mixed's rule (the same for both formats), per position
  constexpr bool SEL = true;
  constexpr long bg_stride = 0;
  [[maybe_unused]] const int* const slot_of = nullptr;
#define BSX_VT_OWN_LDS
#define BSX_VT_TILE tile_
#define BSX_VT_POS 0l                                                /* the record's own bases: index 0 of each */
#define BSX_VT_DESC(fl) fl = d.flags
  if (d.flags & kGeomYuyvIn) {
    constexpr bool YIN = true;
    if (G.c.direct) {
      constexpr bool DIRECT = true;
#include "vcam_tile.inc"
    } else {
      constexpr bool DIRECT = false;
#include "vcam_tile.inc"
    }
  } else {
    constexpr bool YIN = false;
    if (G.c.direct) {
      constexpr bool DIRECT = true;
#include "vcam_tile.inc"
    } else {
      constexpr bool DIRECT = false;
#include "vcam_tile.inc"
    }
  }
#undef BSX_VT_OWN_LDS
#undef BSX_VT_TILE
#undef BSX_VT_POS
#undef BSX_VT_DESC
}
}  // namespace

// the ragged output grid as a launcher takes it: a group's span is whole records; past the last group every span is empty
static bool out_spans_ok(const OutSpans& outs, const VgOutGroup* groups, const GeomDesc* odesc, const GeomSpans& tiles, int n) {
  const int total = outs.wg[kMaxOutGroups];
  if (n <= 0 || tiles.wg[kMaxGeoms] <= 0 || total < 0 || outs.ng < 0 || outs.ng > kMaxOutGroups || (total > 0 && (!groups || !odesc || outs.ng == 0 || outs.wg[0] != 0)))
    return false;
  for (int k = 0; k < kMaxOutGroups; k++)
    if (k < outs.ng ? (outs.per[k] <= 0 || outs.wg[k + 1] <= outs.wg[k] || (outs.wg[k + 1] - outs.wg[k]) % outs.per[k]) : outs.wg[k] != total) return false;
  return true;
}

// the resize pass of BGR / YUYV records by `fmt` (named here, in the order fmt, plain: the order of a kernel's first use is its place in the device code)
static void (*const kVgOuts[2])(const VgOutGroup*, const GeomDesc*, OutSpans) = {vg_outs_fmt_k<>, vg_outs_k<>};

// ---- bsx_step_batch_vcam_geoms_outs_nv12: the same resize pass, every record written as NV12 into two pitched planes (kernels.hpp: VgNv12Rec) ----------------------
// vg_outs_k / vg_outs_fmt_k with vcam_tile.inc's NV12 form (BSX_VT_NV12: a lane's two groups are a row pair; Y and 2 x 2-subsampled chroma stored from the registers
// that hold the four pixels).  The record's second plane and its two pitches come from a table of their own, one 16-byte uniform load beside the descriptor's: GeomDesc
// keeps its layout.  G.opt's output bits are not read.  Kernels of their own at the end of the file, in a namespace of their own (the reason is given above
// mask_geoms_k): every earlier kernel's text is what it was.
static_assert(sizeof(VgNv12Rec) == 16, "vg_nv12_rec reads a record as one uint4");
namespace {
struct Nv12Regs { uint8_t* uv; int pitch_y, pitch_uv; };
__device__ __forceinline__ Nv12Regs vg_nv12_rec(const VgNv12Rec* __restrict__ rec, int n) {
  const uint4 v = reinterpret_cast<const uint4*>(rec)[n];
  typedef __attribute__((address_space(1))) uint8_t* gp;
  return Nv12Regs{(uint8_t*)(gp)(((uint64_t)v.y << 32) | v.x), (int)v.z, (int)v.w};
}

template <int = 0>
__global__ __launch_bounds__(kThreads) void vg_outs_nv12_k(const VgOutGroup* __restrict__ groups, const GeomDesc* __restrict__ odesc, const VgNv12Rec* __restrict__ nrec,
                                                           OutSpans sp) {
  int g, w0, r0, per;
  out_span(sp, (int)blockIdx.x, &g, &w0, &r0, &per);
  const unsigned local = blockIdx.x - (unsigned)w0, rl = local / (unsigned)per, tile_ = local - rl * (unsigned)per;
  const VgOutGroup G = groups[g];                                     // (uniform index: scalar loads) — independent of the descriptor's and the plane record's
  const GeomDescRegs d = geom_desc(odesc, r0 + (int)rl);
  const Nv12Regs nv = vg_nv12_rec(nrec, r0 + (int)rl);
  const int W = G.c.W, H = G.c.H, ntx = G.ntx;
  int opt = 0;
  const ResizeTab tab = geom_tab(G.c.tab);
  const uint8_t *const frames = d.frame, *const bg = d.bg, *const masks = d.mask;
  uint8_t *const out = d.out, *const out_uv = nv.uv;                  // the Y plane, the UV plane
  const int pitch_y = nv.pitch_y, pitch_uv = nv.pitch_uv;
  if ((W & 3) == 0 && ((((uintptr_t)frames) | ((uintptr_t)masks)) & 3) == 0) opt |= kVcWords;      // launch_vg_mixed's rule, per position
  constexpr bool SEL = true, YIN = false;
  constexpr long bg_stride = 0;
  [[maybe_unused]] const int* const slot_of = nullptr;
#define BSX_VT_NV12
#define BSX_VT_TILE tile_
#define BSX_VT_POS 0l                                                /* the record's own bases: index 0 of each */
#define BSX_VT_DESC(fl) fl = d.flags
  if (G.c.direct) {
    constexpr bool DIRECT = true;
#include "vcam_tile.inc"
  } else {
    constexpr bool DIRECT = false;
#include "vcam_tile.inc"
  }
#undef BSX_VT_TILE
#undef BSX_VT_POS
#undef BSX_VT_DESC
#undef BSX_VT_NV12
}

// vg_outs_nv12_k for a call with at least one YUYV item: vg_outs_fmt_k's choice per (form, format), one staging area for all four inclusions
template <int = 0>
__global__ __launch_bounds__(kThreads) void vg_outs_nv12_fmt_k(const VgOutGroup* __restrict__ groups, const GeomDesc* __restrict__ odesc,
                                                               const VgNv12Rec* __restrict__ nrec, OutSpans sp) {
  __shared__ uint32_t s_px[kVLdsWords];
  int g, w0, r0, per;
  out_span(sp, (int)blockIdx.x, &g, &w0, &r0, &per);
  const unsigned local = blockIdx.x - (unsigned)w0, rl = local / (unsigned)per, tile_ = local - rl * (unsigned)per;
  const VgOutGroup G = groups[g];                                     // (uniform index: scalar loads) — independent of the descriptor's and the plane record's
  const GeomDescRegs d = geom_desc(odesc, r0 + (int)rl);
  const Nv12Regs nv = vg_nv12_rec(nrec, r0 + (int)rl);
  const int W = G.c.W, H = G.c.H, ntx = G.ntx;
  int opt = 0;
  const ResizeTab tab = geom_tab(G.c.tab);
  const uint8_t *const frames = d.frame, *const bg = d.bg, *const masks = d.mask;
  uint8_t *const out = d.out, *const out_uv = nv.uv;                  // the Y plane, the UV plane
  const int pitch_y = nv.pitch_y, pitch_uv = nv.pitch_uv;
  if ((W & 3) == 0 && ((((uintptr_t)frames) | ((uintptr_t)masks)) & 3) == 0) opt |= kVcWords;      // launch_vg_mixed's rule (the same for both formats), per position
  constexpr bool SEL = true;
  constexpr long bg_stride = 0;
  [[maybe_unused]] const int* const slot_of = nullptr;
#define BSX_VT_NV12
#define BSX_VT_OWN_LDS
#define BSX_VT_TILE tile_
#define BSX_VT_POS 0l                                                /* the record's own bases: index 0 of each */
#define BSX_VT_DESC(fl) fl = d.flags
  if (d.flags & kGeomYuyvIn) {
    constexpr bool YIN = true;
    if (G.c.direct) {
      constexpr bool DIRECT = true;
#include "vcam_tile.inc"
    } else {
      constexpr bool DIRECT = false;
#include "vcam_tile.inc"
    }
  } else {
    constexpr bool YIN = false;
    if (G.c.direct) {
      constexpr bool DIRECT = true;
#include "vcam_tile.inc"
    } else {
      constexpr bool DIRECT = false;
#include "vcam_tile.inc"
    }
  }
#undef BSX_VT_OWN_LDS
#undef BSX_VT_TILE
#undef BSX_VT_POS
#undef BSX_VT_DESC
#undef BSX_VT_NV12
}

// bsx_bgr_to_nv12: one lane per block of 4 x 2 pixels (the 2-pixel block that ends a row of w % 4 == 2 included) — the two rows' yuyv_pair words, a Y dword per row
// and one UV dword, the arithmetic of the NV12 form of vcam_tile.inc.  WORDS: w % 4 == 0 and a 4-byte aligned source, three dwords per row; else bytes.
template <bool WORDS>
__global__ __launch_bounds__(kThreads) void bgr_to_nv12_k(const uint8_t* __restrict__ bgr, uint8_t* __restrict__ yp, int pitch_y, uint8_t* __restrict__ uvp, int pitch_uv,
                                                         int w, int h) {
  const unsigned gpr = ((unsigned)w + 3) / 4, i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= gpr * ((unsigned)h / 2)) return;
  const int r = (int)(i / gpr), x = 4 * (int)(i - (unsigned)r * gpr), cnt = min(4, w - x);
  const long n = blockIdx.y;
  const uint8_t* const src = bgr + n * (long)w * h * 3;
  uint32_t c[2], yw[2];
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const uint8_t* const p = src + ((long)(2 * r + j) * w + x) * 3;
    uint32_t p0, p1;
    if constexpr (WORDS) {
      const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
      const uint32_t a = q[0], b = q[1], e = q[2];
      p0 = yuyv_pair(a & 255u, (a >> 8) & 255u, (a >> 16) & 255u, a >> 24, b & 255u, (b >> 8) & 255u);
      p1 = yuyv_pair((b >> 16) & 255u, b >> 24, e & 255u, (e >> 8) & 255u, (e >> 16) & 255u, e >> 24);
    } else {
      p0 = yuyv_pair(p[0], p[1], p[2], p[3], p[4], p[5]);
      p1 = cnt == 4 ? yuyv_pair(p[6], p[7], p[8], p[9], p[10], p[11]) : p0;
    }
    yw[j] = __builtin_amdgcn_perm(p1, p0, 0x06040200u);
    c[j] = __builtin_amdgcn_perm(p1, p0, 0x07050301u);
  }
  const uint32_t uv = (c[0] & c[1]) + (((c[0] ^ c[1]) >> 1) & 0x7f7f7f7fu);      // per byte (a + b) / 2, truncating
  uint8_t* const y0 = yp + (n * (long)h + 2 * r) * pitch_y + x;
  uint8_t* const u0 = uvp + (n * (long)(h / 2) + r) * pitch_uv + x;
  if (cnt == 4) {
    *reinterpret_cast<uint32_t*>(y0) = yw[0]; *reinterpret_cast<uint32_t*>(y0 + pitch_y) = yw[1]; *reinterpret_cast<uint32_t*>(u0) = uv;
  } else {
    *reinterpret_cast<uint16_t*>(y0) = (uint16_t)yw[0]; *reinterpret_cast<uint16_t*>(y0 + pitch_y) = (uint16_t)yw[1]; *reinterpret_cast<uint16_t*>(u0) = (uint16_t)uv;
  }
}
}  // namespace

// ... of NV12 records, likewise
static void (*const kVgOutsNv12[2])(const VgOutGroup*, const GeomDesc*, const VgNv12Rec*, OutSpans) = {vg_outs_nv12_fmt_k<>, vg_outs_nv12_k<>};

hipError_t launch_bgr_to_nv12(const uint8_t* bgr, int w, int h, int n, uint8_t* y, int pitch_y, uint8_t* uv, int pitch_uv, hipStream_t s) {
  if (w <= 0 || h <= 0 || n <= 0 || ((w | h) & 1) || pitch_y < w || pitch_uv < w || ((pitch_y | pitch_uv) & 3) || (((uintptr_t)y | (uintptr_t)uv) & 3))
    return hipErrorInvalidValue;
  const long blocks = (long)((w + 3) / 4) * (h / 2);
  if (blocks >= (1l << 31)) return hipErrorInvalidValue;
  const bool words = (w & 3) == 0 && ((uintptr_t)bgr & 3) == 0;
  for (int n0 = 0; n0 < n; n0 += kMaxGridY) {
    const int nn = n - n0 < kMaxGridY ? n - n0 : kMaxGridY;
    const uint8_t* const src = bgr + (size_t)n0 * w * h * 3;
    uint8_t* const yp = y + (size_t)n0 * h * pitch_y;
    uint8_t* const up = uv + (size_t)n0 * (h / 2) * pitch_uv;
    if (words) bgr_to_nv12_k<true><<<dim3(blocks_for(blocks), nn), kThreads, 0, s>>>(src, yp, pitch_y, up, pitch_uv, w, h);
    else bgr_to_nv12_k<false><<<dim3(blocks_for(blocks), nn), kThreads, 0, s>>>(src, yp, pitch_y, up, pitch_uv, w, h);
  }
  return hipGetLastError();
}

// ---- bsx_step_batch_surfaces and bsx_nv12_to_bgr: the frame of a position is an NV12 surface (kernels.hpp: VgSurfRec) ------------------------------------------------
// A 4:2:0 frame differs from a 4:2:2 one only in where a pixel's U and V bytes lie: pixel (x, y) takes Y[y][x] and the pair UV[y >> 1][x & ~1 ..], and from there the
// integers are yuv_tap_to_bgr's / yuyv4_to_bgr3's.  prep_geoms_nv12_k is prep_geoms_k with prep_tile.inc's NV12 windows (BSX_PT_NV12), vg_outs_nv12in_k is
// vg_outs_nv12_k with vcam_tile.inc's frame read through vcam_surf_px / vcam_surf_group (BSX_VT_NV12IN).  A position's second plane and pitches come from a table of
// 16-byte records beside the descriptors, one uniform load; GeomDesc keeps its layout, an output record's descriptor names its position in pad[0].  Kernels of their
// own at the end of the file, in a namespace of their own (the reason is given above mask_geoms_k): every earlier kernel's text is what it was.
static_assert(sizeof(VgSurfRec) == 16, "vg_surf_rec reads a record as one uint4");
namespace {
struct VcSurf { const uint8_t* uv; int py, puv; };
__device__ __forceinline__ VcSurf vg_surf_rec(const VgSurfRec* __restrict__ rec, int n) {
  const uint4 v = reinterpret_cast<const uint4*>(rec)[n];
  typedef __attribute__((address_space(1))) uint8_t* gp;
  return VcSurf{(const uint8_t*)(gp)(((uint64_t)v.y << 32) | v.x), (int)v.z, (int)v.w};
}
// the surface's pixel (cx, cy) as B | G << 8 | R << 16: one Y byte and the chroma pair of its column (vcam_frame_px for a surface)
__device__ __forceinline__ uint32_t vcam_surf_frame_px(const uint8_t* __restrict__ fr, const VcSurf& sf, int cx, int cy) {
  const uint8_t* const c = sf.uv + (long)(cy >> 1) * sf.puv + (cx & ~1);
  return yuv_tap_to_bgr((uint32_t)fr[(long)cy * sf.py + cx] | ((uint32_t)c[0] << 8) | ((uint32_t)c[1] << 16));
}
// vcam_px<.., SEL = true> with the frame a surface
template <bool SEL>
__device__ __forceinline__ uint32_t vcam_surf_px(const uint8_t* __restrict__ fr, const VcSurf& sf, const uint8_t* __restrict__ bgp, const uint8_t* __restrict__ mk, int W,
                                                 int cx, int cy, bool off) {
  static_assert(SEL, "the surface step is a per-position form");
  const long p = (long)cy * W + cx;
  const uint32_t fw = vcam_surf_frame_px(fr, sf, cx, cy);               // (the frame's loads first, as in vcam_px)
  if (off) return fw & 0xffffffu;
  const uint8_t* a = bgp + p * 3;
  const uint32_t m = (uint32_t)mk[p] * 0x00010001u;
  return blend_word((uint32_t)a[0] | ((uint32_t)a[1] << 8) | ((uint32_t)a[2] << 16), fw, m, m);
}
// vcam_group<.., SEL = true> with the frame a surface.  words (W % 4 == 0, cx % 4 == 0, 4-byte aligned planes and pitches): one Y dword at cy * pitch_y + cx and one
// UV dword at (cy >> 1) * pitch_uv + cx are the group's two 4:2:2 words (Y0 U0 Y1 V0, Y2 U1 Y3 V1) after two v_perm_b32
template <bool SEL>
__device__ __forceinline__ void vcam_surf_group(const uint8_t* __restrict__ fr, const VcSurf& sf, const uint8_t* __restrict__ bgp, const uint8_t* __restrict__ mk, int W,
                                                int cx, int cy, bool words, uint32_t w[4], bool off) {
  if (words) {
    const long p = (long)cy * W + cx;
    const uint32_t yw = *reinterpret_cast<const uint32_t*>(fr + (long)cy * sf.py + cx), cw = *reinterpret_cast<const uint32_t*>(sf.uv + (long)(cy >> 1) * sf.puv + cx);
    uint32_t f3[3], o[3];
    yuyv4_to_bgr3(__builtin_amdgcn_perm(cw, yw, 0x05010400u), __builtin_amdgcn_perm(cw, yw, 0x07030602u), f3);
    if (off) { vcam_quad_words(f3, w); return; }
    const u3v av = *reinterpret_cast<const u3v*>(bgp + p * 3);
    const uint32_t a3[3] = {av.x, av.y, av.z};
    blend_quad(a3, f3, *reinterpret_cast<const uint32_t*>(mk + p), o);
    vcam_quad_words(o, w);
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; k++) w[k] = cx + k < W ? vcam_surf_px<SEL>(fr, sf, bgp, mk, W, cx + k, cy, off) : 0u;
}

// prep_geoms_k for positions that are all NV12 surfaces: every class of the call has the proper INTER_LINEAR table and W >= 4 (the host admits no other), so there
// is one body.  desc[f].frame is the Y plane, srec[f] the rest of the surface.
template <int OUT>
__global__ __launch_bounds__(kThreads) void prep_geoms_nv12_k(const GeomClass* __restrict__ classes, const GeomDesc* __restrict__ desc, const VgSurfRec* __restrict__ srec,
                                                             GeomSpans sp, float* __restrict__ input, uint32_t* __restrict__ input_u8, int inW, int inH, BilateralParams bp,
                                                             int TW, int TH, int ntx, int nty, int n_frames) {
  __shared__ float lut[768];
  __shared__ uint32_t tile[kPfS * kPfS];
  const int tid = threadIdx.x;
  unsigned f_, t_;
  xcd_frame_tile((unsigned)(ntx * nty), (unsigned)n_frames, &f_, &t_);
  const int g = geom_class_of_position(sp, (int)f_);
  const GeomClass c = classes[g];                                     // (uniform index: scalar loads) — independent of the descriptor's and the surface record's
  const uint8_t* const frames = geom_desc(desc, (int)f_).frame;
  const VcSurf sf = vg_surf_rec(srec, (int)f_);
  const uint8_t* const suv = sf.uv;
  const int pitch_y = sf.py, pitch_uv = sf.puv;
  const ResizeTab tab = geom_tab(c.down);
  const int W = c.W;
  const Rect4 roi = c.roi, q = c.in_roi;
  const long n = (long)f_;
  constexpr bool LINEAR = true, YIN = true;
#define BSX_PT_NV12
#include "prep_tile.inc"
#undef BSX_PT_NV12
}

// vg_outs_nv12_k with every position's frame a surface: odesc[r].frame is the Y plane of record r's position, srec[odesc[r].pad[0]] the rest of it
template <int = 0>
__global__ __launch_bounds__(kThreads) void vg_outs_nv12in_k(const VgOutGroup* __restrict__ groups, const GeomDesc* __restrict__ odesc, const VgNv12Rec* __restrict__ nrec,
                                                             const VgSurfRec* __restrict__ srec, OutSpans sp) {
  __shared__ uint32_t s_px[kVLdsWords];
  int g, w0, r0, per;
  out_span(sp, (int)blockIdx.x, &g, &w0, &r0, &per);
  const unsigned local = blockIdx.x - (unsigned)w0, rl = local / (unsigned)per, tile_ = local - rl * (unsigned)per;
  const VgOutGroup G = groups[g];                                     // (uniform index: scalar loads) — independent of the descriptor's and the plane record's
  const GeomDescRegs d = geom_desc(odesc, r0 + (int)rl);
  const Nv12Regs nv = vg_nv12_rec(nrec, r0 + (int)rl);
  const VcSurf surf = vg_surf_rec(srec, (int)reinterpret_cast<const uint4*>(odesc)[3 * (size_t)(r0 + (int)rl) + 2].z);      // pad[0]: the record's position
  const int W = G.c.W, H = G.c.H, ntx = G.ntx;
  int opt = 0;
  const ResizeTab tab = geom_tab(G.c.tab);
  const uint8_t *const frames = d.frame, *const bg = d.bg, *const masks = d.mask;
  uint8_t *const out = d.out, *const out_uv = nv.uv;                  // the Y plane, the UV plane of the OUTPUT
  const int pitch_y = nv.pitch_y, pitch_uv = nv.pitch_uv;
  if ((W & 3) == 0 && ((((uintptr_t)frames) | ((uintptr_t)masks) | ((uintptr_t)surf.uv) | (uintptr_t)(surf.py | surf.puv)) & 3) == 0) opt |= kVcWords;      // launch_vg_mixed's rule, per position, with the surface's second plane and pitches
  constexpr bool SEL = true, YIN = false;
  constexpr long bg_stride = 0;
  [[maybe_unused]] const int* const slot_of = nullptr;
#define BSX_VT_NV12
#define BSX_VT_NV12IN
#define BSX_VT_OWN_LDS
#define BSX_VT_TILE tile_
#define BSX_VT_POS 0l                                                /* the record's own bases: index 0 of each */
#define BSX_VT_DESC(fl) fl = d.flags
  if (G.c.direct) {
    constexpr bool DIRECT = true;
#include "vcam_tile.inc"
  } else {
    constexpr bool DIRECT = false;
#include "vcam_tile.inc"
  }
#undef BSX_VT_TILE
#undef BSX_VT_POS
#undef BSX_VT_DESC
#undef BSX_VT_OWN_LDS
#undef BSX_VT_NV12IN
#undef BSX_VT_NV12
}

// bsx_nv12_to_bgr: one lane per block of 4 x 2 pixels (the 2-pixel block that ends a row of w % 4 == 2 included) — a Y dword per row and one UV dword (16 bits each
// in the tail block: no byte at or past w of a row is read), per row the two 4:2:2 words of the block and yuyv4_to_bgr3.  WORDS: w % 4 == 0 and a 4-byte aligned
// destination, three dwords per row; else the 3 cnt bytes of a row one by one.
template <bool WORDS>
__global__ __launch_bounds__(kThreads) void nv12_to_bgr_k(const uint8_t* __restrict__ yp, int pitch_y, const uint8_t* __restrict__ uvp, int pitch_uv,
                                                         uint8_t* __restrict__ bgr, int w, int h) {
  const unsigned gpr = ((unsigned)w + 3) / 4, i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= gpr * ((unsigned)h / 2)) return;
  const int r = (int)(i / gpr), x = 4 * (int)(i - (unsigned)r * gpr), cnt = min(4, w - x);
  const long n = blockIdx.y;
  const uint8_t* const y0 = yp + (n * (long)h + 2 * r) * pitch_y + x;
  const uint8_t* const u0 = uvp + (n * (long)(h / 2) + r) * pitch_uv + x;
  uint32_t yw[2], cw;
  if (WORDS || cnt == 4) {
    yw[0] = *reinterpret_cast<const uint32_t*>(y0); yw[1] = *reinterpret_cast<const uint32_t*>(y0 + pitch_y); cw = *reinterpret_cast<const uint32_t*>(u0);
  } else {
    yw[0] = *reinterpret_cast<const uint16_t*>(y0); yw[1] = *reinterpret_cast<const uint16_t*>(y0 + pitch_y); cw = *reinterpret_cast<const uint16_t*>(u0);
  }
#pragma unroll
  for (int j = 0; j < 2; j++) {
    uint32_t b3[3];
    yuyv4_to_bgr3(__builtin_amdgcn_perm(cw, yw[j], 0x05010400u), __builtin_amdgcn_perm(cw, yw[j], 0x07030602u), b3);
    uint8_t* const o = bgr + ((n * (long)h + 2 * r + j) * w + x) * 3;
    if constexpr (WORDS) {
      *reinterpret_cast<u3v*>(o) = u3v{b3[0], b3[1], b3[2]};
    } else {
#pragma unroll
      for (int b = 0; b < 12; b++)
        if (b < 3 * cnt) o[b] = (uint8_t)(b3[b >> 2] >> (8 * (b & 3)));
    }
  }
}
}  // namespace

bool prep_nv12_fusable(int W, int H, const ResizeTab& tab) { return tab.mode == 0 && ((W | H) & 1) == 0 && W >= 4; }

hipError_t launch_prep_geoms_nv12(const GeomClass* classes, const GeomDesc* desc, const VgSurfRec* srec, const GeomSpans& spans, float* input, uint32_t* input_u8, int inW,
                                  int inH, BilateralParams bp, int n, hipStream_t s) {
  if ((!input && !input_u8) || n <= 0 || !srec) return hipErrorInvalidValue;
  const int ntx = (inW + 31) / 32, nty = (inH + 31) / 32, TW = (inW + ntx - 1) / ntx, TH = (inH + nty - 1) / nty;      // launch_prep_fused's tiles
  if ((unsigned long long)ntx * nty * (unsigned long long)n >= (1ull << 31)) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(ntx * nty) * (unsigned)n);
#define BSX_PG(O) prep_geoms_nv12_k<O><<<grid, kThreads, 0, s>>>(classes, desc, srec, spans, input, input_u8, inW, inH, bp, TW, TH, ntx, nty, xcd_frames(n))
  if (input && input_u8) BSX_PG(3); else if (input_u8) BSX_PG(2); else BSX_PG(1);
#undef BSX_PG
  return hipGetLastError();
}

// the resize pass by the form of the records and of the frames: nrec NULL — BGR / YUYV records (vg_outs_k); nrec — NV12 records (vg_outs_nv12_k); srec with nrec — the
// frames are NV12 surfaces too (vg_outs_nv12in_k, which has no fmt form: no position is YUYV).  fmt: some position's frame is YUYV (the *_fmt_k kernels)
hipError_t launch_vcam_geoms_outs(const GeomClass* classes, const VgOutGroup* groups, const GeomDesc* odesc, const VgNv12Rec* nrec, const VgSurfRec* srec,
                                  const OutSpans& outs, const GeomDesc* desc, const GeomSpans& tiles, unsigned xcd_mask, const uint8_t* ofinal, int outW, int outH,
                                  uint8_t* tile_class, int n, hipStream_t s, bool fmt) {
  const int total = outs.wg[kMaxOutGroups];
  if (!out_spans_ok(outs, groups, odesc, tiles, n) || (srec && (fmt || (total > 0 && !nrec)))) return hipErrorInvalidValue;
  launch_vcam_masks(classes, desc, tiles, xcd_mask, ofinal, outW, outH, tile_class, n, s);
  if (total <= 0) return hipGetLastError();
  const dim3 grid((unsigned)total);
  if (srec) vg_outs_nv12in_k<><<<grid, kThreads, 0, s>>>(groups, odesc, nrec, srec, outs);
  else if (nrec) kVgOutsNv12[fmt ? 0 : 1]<<<grid, kThreads, 0, s>>>(groups, odesc, nrec, outs);
  else kVgOuts[fmt ? 0 : 1]<<<grid, kThreads, 0, s>>>(groups, odesc, outs);
  return hipGetLastError();
}

hipError_t launch_nv12_to_bgr(const uint8_t* y, int pitch_y, const uint8_t* uv, int pitch_uv, int w, int h, int n, uint8_t* bgr, hipStream_t s) {
  if (w <= 0 || h <= 0 || n <= 0 || ((w | h) & 1) || pitch_y < w || pitch_uv < w || ((pitch_y | pitch_uv) & 3) || (((uintptr_t)y | (uintptr_t)uv) & 3))
    return hipErrorInvalidValue;
  const long blocks = (long)((w + 3) / 4) * (h / 2);
  if (blocks >= (1l << 31)) return hipErrorInvalidValue;
  const bool words = (w & 3) == 0 && ((uintptr_t)bgr & 3) == 0;
  for (int n0 = 0; n0 < n; n0 += kMaxGridY) {
    const int nn = n - n0 < kMaxGridY ? n - n0 : kMaxGridY;
    const uint8_t* const yp = y + (size_t)n0 * h * pitch_y;
    const uint8_t* const up = uv + (size_t)n0 * (h / 2) * pitch_uv;
    uint8_t* const dst = bgr + (size_t)n0 * w * h * 3;
    if (words) nv12_to_bgr_k<true><<<dim3(blocks_for(blocks), nn), kThreads, 0, s>>>(yp, pitch_y, up, pitch_uv, dst, w, h);
    else nv12_to_bgr_k<false><<<dim3(blocks_for(blocks), nn), kThreads, 0, s>>>(yp, pitch_y, up, pitch_uv, dst, w, h);
  }
  return hipGetLastError();
}

// ---- bsx_gaussian_blur_surfaces_batch: n NV12 surfaces, each of its own size, pitches and blur size, in ONE launch ------------------------------------------------------
// blur_batch_k with another staging pass: the ragged grid, the tile (64 x 16, de-interleaved byte planes in LDS), the coefficient table and blur_passes<NT> are its
// own; a position's BlurSurfDesc comes by three uniform loads and stays in SGPRs.  Pixel (x, y) of a surface takes Y[y][x] and the pair UV[y >> 1][x & ~1 ..], the
// integers from there are yuv_tap_to_bgr's (vcam_surf_frame_px).  Decided per workgroup, on scalars:
//   * staging: the word path under blur_batch_k's `xin` rule with rows4 always true (planes and pitches are dword aligned whatever w is) and the bound on the WIDTH,
//     x0 - r - sh + 4 Gw <= W, never on the pitch: bytes [w, pitch) of a row are not read.  An item is (row, 4-pixel group): one Y dword at gy * pitch_y + xb + 4 grp
//     and one UV dword (U0 V0 U1 V1) at (gy >> 1) * pitch_uv + xb + 4 grp, gy the row after reflect101_far — xb is a multiple of 4, so the dword holds the group's two
//     whole chroma pairs — into yuv_luma / yuv_chroma / sat_pk2_shr20 as blur_batch_k's YUYV word path: one dword per LDS plane.  Else the reflecting byte path
//     (sh = 0, its own coefficient record): pixel (gx, gy) after BOTH reflections, its chroma row (gy >> 1) that of the reflected row;
//   * NT, the output form (dwords from the packed tile where w % 4 == 0 and dst is 4-byte aligned, else byte stores from the vertical pass) and ksize 1 (the converted
//     pixels, stored without LDS) as in blur_batch_k.
// Offsets into the planes and into dst are 32-bit: the host refuses a plane of 2^31 bytes or more and w * h * 3 >= 2^31 (picture_batch_plan.hpp).
// A template of one instance in a namespace of its own at the end of the file, launched by the file's last launcher, for the reason given above mask_geoms_k: every
// earlier kernel's text is what it was.
namespace {
struct BlurSurfRegs { const uint8_t* y; const uint8_t* uv; uint8_t* dst; int py, puv, w, h, ksize; };
__device__ __forceinline__ BlurSurfRegs blur_surf_desc(const BlurSurfDesc* __restrict__ desc, int n) {
  const uint4* p = reinterpret_cast<const uint4*>(desc) + 3 * (size_t)n;
  const uint4 a = p[0], b = p[1], c = p[2];
  typedef __attribute__((address_space(1))) uint8_t* gp;
  BlurSurfRegs d;
  d.y = (const uint8_t*)(gp)(((uint64_t)a.y << 32) | a.x);
  d.uv = (const uint8_t*)(gp)(((uint64_t)a.w << 32) | a.z);
  d.dst = (uint8_t*)(gp)(((uint64_t)b.y << 32) | b.x);
  d.py = (int)b.z; d.puv = (int)b.w;
  d.w = (int)c.x; d.h = (int)c.y; d.ksize = (int)c.z;
  return d;
}
// pixel (gx, gy) of a position's surface as B | G << 8 | R << 16: vcam_surf_frame_px with 32-bit offsets
__device__ __forceinline__ uint32_t blur_surf_px(const BlurSurfRegs& d, int gx, int gy) {
  const uint8_t* const c = d.uv + (unsigned)((gy >> 1) * d.puv + (gx & ~1));
  return yuv_tap_to_bgr((uint32_t)d.y[(unsigned)(gy * d.py + gx)] | ((uint32_t)c[0] << 8) | ((uint32_t)c[1] << 16));
}

template <int = 0>
__global__ __launch_bounds__(kThreads) void blur_surfaces_k(const BlurSurfDesc* __restrict__ desc, const GaussCoef* __restrict__ coef, GeomSpans sp, BlurTileCols cols) {
  __shared__ __attribute__((aligned(16))) uint8_t s_src[3 * kGSH * kGSrcStride];          // [plane][row][col]; whole-dword output: later the packed tile [row][kGOStride]
  __shared__ __attribute__((aligned(16))) uint16_t s_h[3 * kGHPlane];                     // [plane][col][row], gh_col()
  int g, w0, p0, p1, per;
  geom_span(sp, (int)blockIdx.x, &g, &w0, &p0, &p1, &per);
  const unsigned local = blockIdx.x - (unsigned)w0, pl = local / (unsigned)per, tile = local - pl * (unsigned)per;
  const BlurSurfRegs d = blur_surf_desc(desc, p0 + (int)pl);
  const int W = d.w, H = d.h, r = d.ksize >> 1;
  uint8_t* __restrict__ const out = d.dst;
  unsigned ntx = (unsigned)cols.ntx[0];                               // (selected on SGPRs, as in blur_batch_k)
#pragma unroll
  for (int k = 1; k < kMaxGeoms; k++) if (g == k) ntx = (unsigned)cols.ntx[k];
  const unsigned ty = tile / ntx, tx = tile - ty * ntx;
  const int x0 = (int)tx * kGTW, y0 = (int)ty * kGTH;
  if (r == 0) {                                                       // ksize 1: the converted pixels themselves
    for (int i = threadIdx.x; i < kGTW * kGTH; i += kThreads) {
      const int gx = x0 + (i & (kGTW - 1)), gy = y0 + i / kGTW;
      if (gx < W && gy < H) {
        const uint32_t px = blur_surf_px(d, gx, gy);
        uint8_t* o = out + (unsigned)(gy * W + gx) * 3u;
        o[0] = (uint8_t)px; o[1] = (uint8_t)(px >> 8); o[2] = (uint8_t)(px >> 16);
      }
    }
    return;
  }
  const int SW = kGTW + 2 * r, SH = kGTH + 2 * r;                     // live part of the source tile
  // 1. stage + convert + de-interleave (reflected at the surface's border)
  const int shw = (-r) & 3, Gw = (SW + shw + 3) >> 2;
  const bool xin = x0 - r - shw >= 0 && x0 - r - shw + 4 * Gw <= W;
  const int sh = xin ? shw : 0;
  if (xin) {                                                          // item = (row, group of 4 pixels) → one dword per plane
    const int G = Gw;
    int row = (int)threadIdx.x / G, grp = (int)threadIdx.x - row * G;
    const int dr = kThreads / G, dc = kThreads - dr * G;
    const unsigned xb = (unsigned)(x0 - r - sh);
    while (row < SH) {
      const int gy = reflect101_far(y0 - r + row, H);
      const uint32_t yw = *reinterpret_cast<const uint32_t*>(d.y + ((unsigned)(gy * d.py) + xb + 4u * (unsigned)grp));              // Y0 Y1 Y2 Y3
      const uint32_t cw = *reinterpret_cast<const uint32_t*>(d.uv + ((unsigned)((gy >> 1) * d.puv) + xb + 4u * (unsigned)grp));     // U0 V0 U1 V1
      int bu0, gu0, ru0, bu1, gu1, ru1;
      yuv_chroma((int)(cw & 255u) - 128, (int)((cw >> 8) & 255u) - 128, &bu0, &gu0, &ru0);
      yuv_chroma((int)((cw >> 16) & 255u) - 128, (int)(cw >> 24) - 128, &bu1, &gu1, &ru1);
      const int ya = yuv_luma(yw & 255u), yb = yuv_luma((yw >> 8) & 255u), yc = yuv_luma((yw >> 16) & 255u), yd = yuv_luma(yw >> 24);
      const uint32_t pb = (sat_pk2_shr20(ya + bu0, yb + bu0) & 0xffffu) | (sat_pk2_shr20(yc + bu1, yd + bu1) << 16);
      const uint32_t pg = (sat_pk2_shr20(ya + gu0, yb + gu0) & 0xffffu) | (sat_pk2_shr20(yc + gu1, yd + gu1) << 16);
      const uint32_t pr = (sat_pk2_shr20(ya + ru0, yb + ru0) & 0xffffu) | (sat_pk2_shr20(yc + ru1, yd + ru1) << 16);
      uint32_t* o = reinterpret_cast<uint32_t*>(s_src + row * kGSrcStride) + grp;
      o[0] = pb; o[kGSH * kGSrcStride / 4] = pg; o[2 * kGSH * kGSrcStride / 4] = pr;
      grp += dc; row += dr;
      if (grp >= G) { grp -= G; row++; }
    }
  } else {
    int row = (int)threadIdx.x / SW, col = (int)threadIdx.x - row * SW;
    const int dr = kThreads / SW, dc = kThreads - dr * SW;
    while (row < SH) {
      const int gy = reflect101_far(y0 - r + row, H), gx = reflect101_far(x0 - r + col, W);
      const uint32_t px = blur_surf_px(d, gx, gy);
      s_src[(0 * kGSH + row) * kGSrcStride + col] = (uint8_t)px;
      s_src[(1 * kGSH + row) * kGSrcStride + col] = (uint8_t)(px >> 8);
      s_src[(2 * kGSH + row) * kGSrcStride + col] = (uint8_t)(px >> 16);
      col += dc; row += dr;
      if (col >= SW) { col -= SW; row++; }
    }
  }
  // 2. + 3. blur_batch_k's passes: NT = ceil((ksize + 3 + sh) / 4) (each body copies its coefficient words out first, then the barrier behind the staging)
  const bool owords = (((W & 3) | (int)((uintptr_t)out & 3)) == 0);
  const GaussCoef* __restrict__ const gc = coef + blur_coef_index(d.ksize, xin);
  switch ((d.ksize + sh + 6) >> 2) {
#define BSX_BS(NT) case NT: blur_passes<NT, 1>(s_src, s_h, gc, SH, owords, out, W, H, x0, y0); break;
    BSX_BS(2) BSX_BS(3) BSX_BS(4) BSX_BS(5) BSX_BS(6) BSX_BS(7) BSX_BS(8) default: BSX_BS(9)
#undef BSX_BS
  }
  if (owords) {                                                       // this lane's 4-pixel group of the packed tile: three whole dwords
    __syncthreads();
    const int orow = threadIdx.x >> 4, ogx = x0 + 4 * (threadIdx.x & 15), ogy = y0 + orow;
    if (ogx < W && ogy < H) {
      const uint32_t* bp = reinterpret_cast<const uint32_t*>(s_src + orow * kGOStride + 12 * (threadIdx.x & 15));
      uint32_t* op = reinterpret_cast<uint32_t*>(out + (unsigned)(ogy * W + ogx) * 3u);
      op[0] = bp[0]; op[1] = bp[1]; op[2] = bp[2];
    }
  }
}
}  // namespace

hipError_t launch_blur_surfaces(const BlurSurfDesc* desc, const GaussCoef* coef, const GeomSpans& spans, const BlurTileCols& cols, hipStream_t s) {
  if (!desc || !coef || spans.wg[kMaxGeoms] <= 0) return hipErrorInvalidValue;
  for (int g = 0; g < kMaxGeoms; g++) if (spans.per[g] > 0 && (cols.ntx[g] <= 0 || spans.per[g] % cols.ntx[g])) return hipErrorInvalidValue;
  blur_surfaces_k<><<<dim3((unsigned)spans.wg[kMaxGeoms]), kThreads, 0, s>>>(desc, coef, spans, cols);
  return hipGetLastError();
}

// ---- bsx_resize_surfaces_batch: n NV12 surfaces, each of its own size and pitches, resized to BGR images of their OWN sizes in ONE launch -----------------------------
// resize_bgr_batch_k's form over a ragged grid: the workgroup finds its destination-size class and its position from the spans (geom_span: compares on SGPRs), the
// class's (dw, dh) from the kernel arguments, the position's ResizeSurfDesc by five uniform loads that stay in SGPRs.  A lane makes FOUR adjacent pixels of one
// output row with sample_linear<3>'s integers; the copy stores the converted pixels themselves, the 2x2 area mean is the linear form on (2 dx, 2 dy) with
// coefficients (1024, 1024) — ((b * ((p * a) >> 4)) >> 16 summed over the rows, + 2, >> 2 gives (p00 + p01 + p10 + p11 + 2) >> 2 exactly.  A tap is yuv_tap_to_bgr(Y | U << 8 | V << 16) as vcam_surf_frame_px makes it — the conversion clamps, so it comes before the fixed point.
// Loads of one output pixel and source row, all bounded by sw and never by the pitch:
//   * Y: the taps' columns sx and sx1 = sx + 1 are one 16-bit load; where the table clamps sx1 onto sx (the right edge) the 16 bits are those of columns
//     max(sx - 1, 0) and the next one;
//   * UV: one 32-bit load at column min(sx & ~1, sw - 4) — an even left column has both taps on one chroma pair, an odd one takes two adjacent pairs, U0 V0 U1 V1
//     (sx + 2 <= sw - 1 there: sw is even); a surface 2 pixels wide has one pair, 16 bits;
//   * the lower row's taps are the upper row's where the rows clamp onto one another, and its chroma words are the upper row's where both rows lie in one chroma row
//     (an even upper row): nothing is loaded twice that the lane already holds.
// Offsets into the planes and into dst are 32-bit from uniform bases: the host refuses a plane of 2^31 bytes or more and dw * dh * 3 >= 2^31
// (picture_batch_plan.hpp).  No LDS: at a down-scale of 2 or more the taps of neighbouring outputs do not overlap.
// A template of one instance in a namespace of its own at the end of the file, launched by the file's last launcher, for the reason given above mask_geoms_k: every
// earlier kernel's text is what it was.
namespace {
struct ResizeSurfRegs { const uint8_t* y; const uint8_t* uv; uint8_t* dst; const int* xofs; const short* xa; const int* yofs; const short* ya; int py, puv, sw, sh, mode; };
__device__ __forceinline__ ResizeSurfRegs resize_surf_desc(const ResizeSurfDesc* __restrict__ desc, int n) {
  const uint4* p = reinterpret_cast<const uint4*>(desc) + 5 * (size_t)n;
  const uint4 a = p[0], b = p[1], c = p[2], e = p[3], f = p[4];
  ResizeSurfRegs d;
  d.y = as_global((const uint8_t*)(((uint64_t)a.y << 32) | a.x));
  d.uv = as_global((const uint8_t*)(((uint64_t)a.w << 32) | a.z));
  d.dst = as_global((uint8_t*)(((uint64_t)b.y << 32) | b.x));
  d.xofs = as_global((const int*)(((uint64_t)b.w << 32) | b.z));
  d.xa = as_global((const short*)(((uint64_t)c.y << 32) | c.x));
  d.yofs = as_global((const int*)(((uint64_t)c.w << 32) | c.z));
  d.ya = as_global((const short*)(((uint64_t)e.y << 32) | e.x));
  d.py = (int)e.z; d.puv = (int)e.w;
  d.sw = (int)f.x; d.sh = (int)f.y; d.mode = (int)f.z;
  return d;
}
struct __attribute__((packed, aligned(1))) RsU16 { uint16_t v; };
struct __attribute__((packed, aligned(2))) RsU32 { uint32_t v; };
// Y of the taps at columns sx and (two ? sx + 1 : sx) of the row at byte offset `row`: Y0 | Y1 << 8
__device__ __forceinline__ uint32_t resize_surf_luma2(const ResizeSurfRegs& d, unsigned row, int sx, bool two) {
  const int xb = two ? sx : max(sx - 1, 0);
  const uint32_t w = reinterpret_cast<const RsU16*>(d.y + (row + (unsigned)xb))->v;
  const uint32_t y0 = sx != xb ? w >> 8 : w & 255u;
  return y0 | ((two ? w >> 8 : y0) << 8);
}
// the chroma pairs of the same two taps, of the chroma row at byte offset `row`: U0 | V0 << 8 | U1 << 16 | V1 << 24
__device__ __forceinline__ uint32_t resize_surf_chroma2(const ResizeSurfRegs& d, unsigned row, int sx, bool two) {
  const int e = sx & ~1;
  if (d.sw < 4) {                                                     // (uniform) sw == 2: the row's one pair
    const uint32_t c = *reinterpret_cast<const uint16_t*>(d.uv + row);
    return c | (c << 16);
  }
  const int cb = min(e, d.sw - 4);
  const uint32_t w = reinterpret_cast<const RsU32*>(d.uv + (row + (unsigned)cb))->v;
  const uint32_t c0 = e != cb ? w >> 16 : w & 0xffffu;
  return c0 | ((two && (sx & 1) ? w >> 16 : c0) << 16);
}

// one lane's group of the copy (sw == dw, sh == dh): nothing to interpolate, so one conversion per pixel instead of four — the group's pixels are one Y dword and one
// UV dword (U0 V0 U1 V1: x is a multiple of 4, rows and planes are dword aligned), converted as yuyv4_to_bgr3 converts two YUYV words; a row's last group where
// sw % 4 == 2 is two pixels of one chroma pair, 16 bits of each plane
__device__ __forceinline__ void resize_surf_copy(const ResizeSurfRegs& d, int dw, int x, int dy) {
  uint8_t* const o = d.dst + (unsigned)(dy * dw + x) * 3u;
  const unsigned yo = (unsigned)(dy * d.py) + (unsigned)x, co = (unsigned)((dy >> 1) * d.puv) + (unsigned)x;
  if (x + 4 > dw) {
    const uint32_t yw = *reinterpret_cast<const uint16_t*>(d.y + yo), cw = *reinterpret_cast<const uint16_t*>(d.uv + co);
    const uint32_t p0 = yuv_tap_to_bgr((yw & 255u) | (cw << 8)), p1 = yuv_tap_to_bgr((yw >> 8) | (cw << 8));
    o[0] = (uint8_t)p0; o[1] = (uint8_t)(p0 >> 8); o[2] = (uint8_t)(p0 >> 16);
    o[3] = (uint8_t)p1; o[4] = (uint8_t)(p1 >> 8); o[5] = (uint8_t)(p1 >> 16);
    return;
  }
  const uint32_t yw = *reinterpret_cast<const uint32_t*>(d.y + yo), cw = *reinterpret_cast<const uint32_t*>(d.uv + co);
  uint32_t w[3];
  yuyv4_to_bgr3((yw & 255u) | ((cw & 255u) << 8) | ((yw & 0xff00u) << 8) | ((cw & 0xff00u) << 16),
                ((yw >> 16) & 255u) | ((cw >> 8) & 0xff00u) | ((yw >> 8) & 0xff0000u) | (cw & 0xff000000u), w);
  if ((dw & 3) == 0 && ((uintptr_t)d.dst & 3) == 0) {                 // (uniform)
    uint32_t* const ow = reinterpret_cast<uint32_t*>(o);
    ow[0] = w[0]; ow[1] = w[1]; ow[2] = w[2];
    return;
  }
#pragma unroll
  for (int i = 0; i < 12; i++) o[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
}
// one lane's group: output pixels x .. x + 3 of row dy of a dw-wide destination.  TAB: the table's taps and coefficients (mode 0); else the 2x2 area mean as the
// linear form described above.  An instance each instead of a mode test per pixel: with the test inside the unrolled loop the compiler (ROCm 7.2, clang 22) left the
// coefficients of pixels 1 .. 3 of the area mode unset.
template <bool TAB>
__device__ __forceinline__ void resize_surf_group(const ResizeSurfRegs& d, int dw, int x, int dy) {
  int sy0, sy1, b0, b1;
  if constexpr (TAB) {
    const int sy = d.yofs[dy];
    sy0 = min(max(sy, 0), d.sh - 1); sy1 = min(max(sy + 1, 0), d.sh - 1);
    b0 = d.ya[2 * dy]; b1 = d.ya[2 * dy + 1];
  } else {
    sy0 = 2 * dy; sy1 = sy0 + 1;
    b0 = b1 = 1024;
  }
  int sx[4], a0[4], a1[4];
  bool two[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int dx = min(x + k, dw - 1);                                // (a row's last group repeats its last pixel; the stores below leave the repeats out)
    if constexpr (TAB) { sx[k] = d.xofs[dx]; two[k] = sx[k] + 1 < d.sw; a0[k] = d.xa[2 * dx]; a1[k] = d.xa[2 * dx + 1]; }
    else { sx[k] = 2 * dx; two[k] = true; a0[k] = a1[k] = 1024; }
  }
  uint32_t yw0[4], cw0[4], yw1[4], cw1[4];
  const unsigned yr0 = (unsigned)(sy0 * d.py), cr0 = (unsigned)((sy0 >> 1) * d.puv);
#pragma unroll
  for (int k = 0; k < 4; k++) { yw0[k] = resize_surf_luma2(d, yr0, sx[k], two[k]); cw0[k] = resize_surf_chroma2(d, cr0, sx[k], two[k]); }
#pragma unroll
  for (int k = 0; k < 4; k++) { yw1[k] = yw0[k]; cw1[k] = cw0[k]; }
  if (sy1 != sy0) {
    const unsigned yr1 = (unsigned)(sy1 * d.py);
#pragma unroll
    for (int k = 0; k < 4; k++) yw1[k] = resize_surf_luma2(d, yr1, sx[k], two[k]);
    if ((sy1 >> 1) != (sy0 >> 1)) {
      const unsigned cr1 = (unsigned)((sy1 >> 1) * d.puv);
#pragma unroll
      for (int k = 0; k < 4; k++) cw1[k] = resize_surf_chroma2(d, cr1, sx[k], two[k]);
    }
  }
  int v[12];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t t00 = yuv_tap_to_bgr((yw0[k] & 255u) | ((cw0[k] & 0xffffu) << 8)), t01 = yuv_tap_to_bgr((yw0[k] >> 8) | ((cw0[k] >> 16) << 8));
    const uint32_t t10 = yuv_tap_to_bgr((yw1[k] & 255u) | ((cw1[k] & 0xffffu) << 8)), t11 = yuv_tap_to_bgr((yw1[k] >> 8) | ((cw1[k] >> 16) << 8));
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const int h0 = (int)((t00 >> (8 * c)) & 255u) * a0[k] + (int)((t01 >> (8 * c)) & 255u) * a1[k];
      const int h1 = (int)((t10 >> (8 * c)) & 255u) * a0[k] + (int)((t11 >> (8 * c)) & 255u) * a1[k];
      v[3 * k + c] = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
    }
  }
  uint8_t* const o = d.dst + (unsigned)(dy * dw + x) * 3u;
  if ((dw & 3) == 0 && ((uintptr_t)d.dst & 3) == 0) {                 // (uniform: the class's width, the descriptor's pointer)
    uint32_t w[3];
#pragma unroll
    for (int j = 0; j < 3; j++) w[j] = (uint32_t)v[4 * j] | ((uint32_t)v[4 * j + 1] << 8) | ((uint32_t)v[4 * j + 2] << 16) | ((uint32_t)v[4 * j + 3] << 24);
    uint32_t* const ow = reinterpret_cast<uint32_t*>(o);
    ow[0] = w[0]; ow[1] = w[1]; ow[2] = w[2];
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if (x + k >= dw) break;
    o[3 * k] = (uint8_t)v[3 * k]; o[3 * k + 1] = (uint8_t)v[3 * k + 1]; o[3 * k + 2] = (uint8_t)v[3 * k + 2];
  }
}

template <int = 0>
__global__ __launch_bounds__(kThreads) void resize_surfaces_k(const ResizeSurfDesc* __restrict__ desc, GeomSpans sp, ResizeDstSizes sz) {
  int g, w0, p0, p1, per;
  geom_span(sp, (int)blockIdx.x, &g, &w0, &p0, &p1, &per);
  const unsigned local = blockIdx.x - (unsigned)w0, pl = local / (unsigned)per, blk = local - pl * (unsigned)per;
  int dw = sz.dw[0], dh = sz.dh[0];                                   // (selected on SGPRs)
#pragma unroll
  for (int k = 1; k < kMaxGeoms; k++) if (g == k) { dw = sz.dw[k]; dh = sz.dh[k]; }
  const unsigned gpr = ((unsigned)dw + 3u) / 4u, grp = blk * kThreads + threadIdx.x;
  if (grp >= gpr * (unsigned)dh) return;
  const ResizeSurfRegs d = resize_surf_desc(desc, p0 + (int)pl);
  const int dy = (int)(grp / gpr), x = (int)(grp - (unsigned)dy * gpr) * 4;
  if (d.mode == 0) resize_surf_group<true>(d, dw, x, dy);             // (uniform)
  else if (d.mode == 1) resize_surf_copy(d, dw, x, dy);
  else resize_surf_group<false>(d, dw, x, dy);
}
}  // namespace

hipError_t launch_resize_surfaces(const ResizeSurfDesc* desc, const GeomSpans& spans, const ResizeDstSizes& sizes, hipStream_t s) {
  if (!desc || spans.wg[kMaxGeoms] <= 0) return hipErrorInvalidValue;
  for (int g = 0; g < kMaxGeoms; g++)
    if (spans.per[g] > 0 && (sizes.dw[g] <= 0 || sizes.dh[g] <= 0 || (long)spans.per[g] != resize_surf_blocks(sizes.dw[g], sizes.dh[g]))) return hipErrorInvalidValue;
  resize_surfaces_k<><<<dim3((unsigned)spans.wg[kMaxGeoms]), kThreads, 0, s>>>(desc, spans, sizes);
  return hipGetLastError();
}

}  // namespace bsx
