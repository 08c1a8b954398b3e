// The body of the kernels that composite at the virtual camera's geometry (kernels_img.hip: vcam_blend_resize_k, SEL = false; vg_mixed_k, SEL = true; and
// vg_geoms_k, SEL = true with every operand per position), included INSIDE each kernel: one output tile of one position.  It is shared as text and not as a device
// function because the dense kernel has to stay the code it was: with the body in an inlined function the compiler schedules and allocates the same statements
// differently.  The including kernel provides the names
//   frames, bg, bg_stride, masks, slot_of, out, W, H, tab, ntx, opt   and   constexpr bool DIRECT, YIN, SEL
// and three expressions, the way mask_tile.inc takes BSX_MT_FRAME: BSX_VT_TILE, the workgroup's tile inside the output image; BSX_VT_POS, the position n that
// indexes frames, masks and out (0 where these are the position's own bases); and BSX_VT_DESC(fl), the statement that fetches position n's descriptor.
// SEL: position n's background, its own flip bits (fl) and its filter switch come from its descriptor (BSX_VT_DESC: in vg_mixed_k one 16-byte uniform load from the
// MixDesc table that travels in `bg`), its mask is slot slot_of[n]'s (NULL: slot n); all of it is workgroup-uniform, so the tile's footprint below is the
// workgroup's own.  Filter off: the composite is the frame (vcam_px / vcam_group with `off`); a background that is not 4-byte aligned takes the byte form for its
// stream alone.
// BSX_VT_NV12 (vg_outs_nv12_k, vg_outs_nv12_fmt_k; undefined, the text is what it was): the tile is written as NV12 into two pitched planes.  The includer also
// provides out_uv, pitch_y, pitch_uv (`out` is the Y plane; dw and dh even).  A lane's two 4-pixel groups are vertically adjacent — rows 2 (tid / 16) and
// 2 (tid / 16) + 1 of the tile instead of tid / 16 and tid / 16 + 16 — so it holds both rows of its 2 x 2 chroma blocks: per row one Y dword, per pair one UV dword
// (16 bits each for the 2-pixel group that ends a row of out_w % 4 == 2), the chroma bytes those of yuyv_pair, averaged over the two rows as it averages two pixels.
// BSX_VT_NV12IN (vg_outs_nv12in_k, with SEL true and YIN false; undefined, the text is what it was): the position's frame is an NV12 surface — `frames` is its Y
// plane, the includer also provides `surf` (VcSurf: the UV plane and the two pitches), and the frame's pixels and 4-pixel groups are read by vcam_surf_px /
// vcam_surf_group.  Background, mask, taps and stores are unchanged.
// BSX_VT_OWN_LDS (vg_geoms_fmt_k, which includes the body once per frame format): the includer declares s_px itself, one staging area for all of its inclusions.
#ifdef BSX_VT_NV12IN
#define BSX_VT_GROUP(...) vcam_surf_group<SEL>(fr, surf, __VA_ARGS__)
#define BSX_VT_PX(...) vcam_surf_px<SEL>(fr, surf, __VA_ARGS__)
#else
#define BSX_VT_GROUP(...) vcam_group<YIN, SEL>(fr, __VA_ARGS__)
#define BSX_VT_PX(...) vcam_px<YIN, SEL>(fr, __VA_ARGS__)
#endif
#ifndef BSX_VT_OWN_LDS
  __shared__ uint32_t s_px[DIRECT ? 1 : kVLdsWords];
#endif
  const int tid = threadIdx.x, ty = (int)(BSX_VT_TILE) / ntx, tx = (int)(BSX_VT_TILE) - ty * ntx;
  const long n = BSX_VT_POS;
  const int dw = tab.dw, dh = tab.dh;
  const int dx0 = tx * kVW, dy0 = ty * kVH, dx1 = min(dx0 + kVW, dw) - 1, dy1 = min(dy0 + kVH, dh) - 1;
  [[maybe_unused]] bool off = false;
  [[maybe_unused]] long slot = n;
  if constexpr (SEL) {                                               // position n's descriptor: background, flips, filter switch; its mask is its slot's
    unsigned fl;
    BSX_VT_DESC(fl);
    off = (fl & kMixFilterOff) != 0;
    opt |= (int)(fl & (kMixFlipH | kMixFlipV));
    if (!off && ((uintptr_t)bg & 3u)) opt &= ~kVcWords;
    if (slot_of) slot = slot_of[n];
  }
  const bool fh = (opt & kVcFlipH) != 0, fv = (opt & kVcFlipV) != 0;
  const uint8_t* fr = frames + n * (long)W * H * (YIN ? 2 : 3);
  const uint8_t* bgp = bg + (SEL ? 0l : n * bg_stride);
  const uint8_t* mk = masks + (SEL ? slot : n) * (long)W * H;
  int gx0 = 0, cy_lo = 0, rw = 0;                                   // LDS image: composite rows cy_lo.., columns gx0.., rw words per row
  if constexpr (!DIRECT) {
    const int fx_lo = tab.xofs[dx0], fx_hi = min(tab.xofs[dx1] + 1, W - 1);
    const int fy_lo = min(max(tab.yofs[dy0], 0), H - 1), fy_hi = min(max(tab.yofs[dy1] + 1, 0), H - 1);
    const int cx_lo = fh ? W - 1 - fx_hi : fx_lo, cx_hi = fh ? W - 1 - fx_lo : fx_hi;
    cy_lo = fv ? H - 1 - fy_hi : fy_lo;
    gx0 = cx_lo & ~3;
    const int ng = ((cx_hi - gx0) >> 2) + 1, items = (fy_hi - fy_lo + 1) * ng;     // rows * ng * 4 <= kVLdsWords: vcam_tile_fits
    rw = 4 * ng;
    const bool words = (opt & kVcWords) != 0;
    // the staging loop, once per value of the filter switch: with `off` a literal the loop of a filtered stream is the dense kernel's — its three loads go out
    // back to back — where a run-time test inside the loop leaves the frame's load waiting behind the mask's (measured: docs/design/05d-image-kernels.md)
#define BSX_VG_STAGE(OFF)                                                                    \
    for (int i = tid; i < items; i += kThreads) {                                            \
      const int r = i / ng, g = i - r * ng;                                                  \
      uint32_t w[4];                                                                         \
      BSX_VT_GROUP(bgp, mk, W, gx0 + 4 * g, cy_lo + r, words, w, OFF);                       \
      *reinterpret_cast<uint4*>(s_px + r * rw + 4 * g) = make_uint4(w[0], w[1], w[2], w[3]); \
    }
    if constexpr (SEL) {
      if (off) { BSX_VG_STAGE(true) } else { BSX_VG_STAGE(false) }
    } else {
      BSX_VG_STAGE(false)
    }
#undef BSX_VG_STAGE
    __syncthreads();
  }
#ifndef BSX_VT_NV12
  const bool yout = (opt & kVcYuyvOut) != 0, owords = (opt & kVcOutWords) != 0;
#else
  uint32_t nv_c = 0;                                                 // the chroma bytes (Ca0, Cb0, Ca1, Cb1) of the pair's upper row, kept for the lower one
#endif
#pragma unroll
  for (int j = 0; j < 2; j++) {
#ifndef BSX_VT_NV12
    const int gi = tid + j * kThreads, ry = gi / (kVW / 4), dy = dy0 + ry, dx = dx0 + 4 * (gi - ry * (kVW / 4));
#else
    const int ry = 2 * (tid / (kVW / 4)) + j, dy = dy0 + ry, dx = dx0 + 4 * (tid % (kVW / 4));      // dy0 and dh even: both rows of a pair are inside, or neither
#endif
    if (dy > dy1 || dx > dx1) continue;
    const int sy = tab.yofs[dy], b0 = tab.ya[2 * dy], b1 = tab.ya[2 * dy + 1];
    int y0 = min(max(sy, 0), H - 1), y1 = min(max(sy + 1, 0), H - 1);
    if (fv) { y0 = H - 1 - y0; y1 = H - 1 - y1; }
    const int cnt = min(4, dx1 - dx + 1);
    uint32_t q[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int d = min(dx + k, dx1);                                // past the tile's last column: the last pixel again (never stored)
      const int a0 = tab.xa[2 * d], a1 = tab.xa[2 * d + 1];
      int x0 = tab.xofs[d], x1 = min(x0 + 1, W - 1);
      if (fh) { x0 = W - 1 - x0; x1 = W - 1 - x1; }
      uint32_t t00, t01, t10, t11;
      if constexpr (DIRECT) {
#define BSX_VG_TAPS(OFF)                                                                                                 \
        t00 = BSX_VT_PX(bgp, mk, W, x0, y0, OFF); t01 = BSX_VT_PX(bgp, mk, W, x1, y0, OFF); \
        t10 = BSX_VT_PX(bgp, mk, W, x0, y1, OFF); t11 = BSX_VT_PX(bgp, mk, W, x1, y1, OFF);
        if constexpr (SEL) {                                         // (once per value of the filter switch, as the staging loop)
          if (off) { BSX_VG_TAPS(true) } else { BSX_VG_TAPS(false) }
        } else {
          BSX_VG_TAPS(false)
        }
#undef BSX_VG_TAPS
      } else {
        const int r0 = (y0 - cy_lo) * rw - gx0, r1 = (y1 - cy_lo) * rw - gx0;
        t00 = s_px[r0 + x0]; t01 = s_px[r0 + x1]; t10 = s_px[r1 + x0]; t11 = s_px[r1 + x1];
      }
      q[k] = vcam_lerp(t00, t01, t10, t11, a0, a1, b0, b1, 0) | (vcam_lerp(t00, t01, t10, t11, a0, a1, b0, b1, 8) << 8) |
             (vcam_lerp(t00, t01, t10, t11, a0, a1, b0, b1, 16) << 16);
    }
#ifdef BSX_VT_NV12
    {                                                                // dw even: cnt is 2 or 4, whole pairs; every address below is a multiple of 4
      const uint32_t p0 = yuyv_pair(q[0] & 255u, (q[0] >> 8) & 255u, q[0] >> 16, q[1] & 255u, (q[1] >> 8) & 255u, q[1] >> 16);
      const uint32_t p1 = yuyv_pair(q[2] & 255u, (q[2] >> 8) & 255u, q[2] >> 16, q[3] & 255u, (q[3] >> 8) & 255u, q[3] >> 16);
      const uint32_t yw = __builtin_amdgcn_perm(p1, p0, 0x06040200u), cw = __builtin_amdgcn_perm(p1, p0, 0x07050301u);
      uint8_t* const yp = out + (n * (long)dh + dy) * pitch_y + dx;
      if (cnt == 4) *reinterpret_cast<uint32_t*>(yp) = yw;
      else *reinterpret_cast<uint16_t*>(yp) = (uint16_t)yw;
      if (j == 0) {
        nv_c = cw;
      } else {
        const uint32_t uv = (nv_c & cw) + (((nv_c ^ cw) >> 1) & 0x7f7f7f7fu);      // per byte (a + b) / 2, truncating
        uint8_t* const up = out_uv + (n * (long)(dh >> 1) + (dy >> 1)) * pitch_uv + dx;
        if (cnt == 4) *reinterpret_cast<uint32_t*>(up) = uv;
        else *reinterpret_cast<uint16_t*>(up) = (uint16_t)uv;
      }
    }
#else
    const long o = n * (long)dw * dh + (long)dy * dw + dx;
    if (yout) {                                                      // dw even: cnt is 2 or 4, whole pairs
      const uint32_t p0 = yuyv_pair(q[0] & 255u, (q[0] >> 8) & 255u, q[0] >> 16, q[1] & 255u, (q[1] >> 8) & 255u, q[1] >> 16);
      const uint32_t p1 = yuyv_pair(q[2] & 255u, (q[2] >> 8) & 255u, q[2] >> 16, q[3] & 255u, (q[3] >> 8) & 255u, q[3] >> 16);
      uint8_t* op = out + o * 2;
      if (owords && cnt == 4) *reinterpret_cast<VcW2*>(op) = VcW2{p0, p1};
      else if (owords) *reinterpret_cast<uint32_t*>(op) = p0;
      else {
#pragma unroll
        for (int b = 0; b < 4; b++) { op[b] = (uint8_t)(p0 >> (8 * b)); if (cnt == 4) op[4 + b] = (uint8_t)(p1 >> (8 * b)); }
      }
    } else {
      uint8_t* op = out + o * 3;
      if (owords && cnt == 4) {
        *reinterpret_cast<u3v*>(op) = u3v{q[0] | (q[1] << 24), (q[1] >> 8) | (q[2] << 16), (q[2] >> 16) | (q[3] << 8)};
      } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
          if (k < cnt) { op[3 * k] = (uint8_t)q[k]; op[3 * k + 1] = (uint8_t)(q[k] >> 8); op[3 * k + 2] = (uint8_t)(q[k] >> 16); }
      }
    }
#endif
  }
#undef BSX_VT_GROUP
#undef BSX_VT_PX
