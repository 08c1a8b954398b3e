// prep_tile.inc — the body of prep_fused_k (kernels_img.hip) from the tile coordinates on, included by the kernel itself and by prep_geoms_tile (the per-position form
// of bsx_step_batch_geoms).  An include, like vcam_tile.inc, and not a device function: as a force-inlined function the same statements compiled to a different
// instruction schedule of prep_fused_k (the kernel-argument loads moved), and the dense step's launch must stay the parent's code.  The includer provides: the
// template constants OUT, LINEAR, YIN; lut, tile (the LDS arrays), tid, t_ (the tile of the canvas), n (long: the output slot of the network input); frames, W, H,
// roi, input, input_u8, inW, inH, q, tab, bp, TW, TH, ntx; and BSX_PREP_FRAME, the index of the frame inside `frames`.
// BSX_PT_NV12 (prep_geoms_nv12_k, with LINEAR and YIN true; undefined, the text is what it was): the frame is an NV12 surface — `frames` is its Y plane, the includer
// also provides suv (the interleaved UV plane), pitch_y and pitch_uv.  A sample's two taps are adjacent Y bytes and the chroma pairs of their columns, so the one
// 8-byte window per source row becomes a 4-byte Y window and a 4-byte UV window (the same 16 bytes of load data per sample), both addressed by the FRAME's column
// and row: the chroma of frame pixel (x, y) is UV[y >> 1][x & ~1 ..], whatever the parity of roi.x and roi.y.
  const int tby = (int)t_ / ntx, tbx = (int)t_ - tby * ntx;
  const int tx0 = tbx * TW, ty0 = tby * TH;
  const int SW = TW + 2 * kCanvasPad, total = SW * (TH + 2 * kCanvasPad);
  [[maybe_unused]] constexpr int FB = YIN ? 2 : 3;                                       // bytes per frame pixel
#ifdef BSX_PT_NV12
  [[maybe_unused]] const uint8_t* src = frames;                            // (named by the discarded non-linear body only: the surface is addressed by frame column and row)
#else
  const uint8_t* src = frames + BSX_PREP_FRAME * (long)W * H * FB + ((long)roi.y * W + roi.x) * FB;
#endif
  const unsigned msw = 0xFFFFFFFFu / (unsigned)SW + 1u;                    // i / SW for i < 2^16
  constexpr int kItems = (kPfS * kPfS + kThreads - 1) / kThreads;
  // the colour-weight table of the bilateral filter: requested with the kernel's first loads (round 5) — staged where it is first used, behind the resize phase, its
  // three loads per lane were one more memory round trip in front of the second barrier
  float lut_v[3];
#pragma unroll
  for (int k = 0; k < 3; k++) lut_v[k] = bp.color_lut[tid + k * kThreads];
  if constexpr (LINEAR) {
    // INTER_LINEAR: everything that depends only on the tile COLUMN (reflected canvas x → source byte offset, coefficient pair, where the two taps sit inside the
    // 8 bytes loaded) or only on the tile ROW (source row offsets, coefficient pair) is worked out once per column / row by the first lanes and kept in LDS; an item
    // is then two table reads, four loads and arithmetic.  Two dependent memory round trips per LANE (tables, then all of its <= kItems samples at once) instead of
    // two per SAMPLE — in the per-sample form (sample_linear inside `if (inside)`) the compiler waits for each sample before it starts the next.
    // 8 source bytes [offc, offc + 8) cover both taps: offc = min(3 sx, row_bytes - 8) never reads past the image row; the taps are bytes s0.. and s1.. of them
    // (s1 = s0 + 3, or s0 where cv::resize clamps the second tap onto the first), pulled out by v_perm_b32 with per-column selectors.  Same integers as sample_linear.
    __shared__ int4 colT[kPfS], rowT[kPfS];                                // {offc | -1, a0 | a1 << 16, sel0, sel1}, {o0 | -1, o1, b0, b1}
#ifdef BSX_PT_NV12
    // NV12: colT.x is the Y window's first FRAME column wy = min(roi.x + sx, W - 4) — four Y bytes that hold both taps and end at or before byte W of the row; the UV
    // window starts at wy & ~1, which is (roi.x + sx) & ~1 or, pulled back with the Y window, W - 4: the taps' chroma pairs are bytes 0-1 or 2-3 of it.  A tap's
    // selector: its Y byte of the Y dword, U and V of the UV dword (bytes 4-7 of the pair).  rowT holds the two Y row offsets, rowU the two UV row offsets (source
    // rows sy0 and sy1 may share one chroma row).
    __shared__ int2 rowU[kPfS];
    const int SHt = TH + 2 * kCanvasPad;
#else
    const int rowlim = (W - roi.x) * FB, SHt = TH + 2 * kCanvasPad;
#endif
    if (tid < SW) {
      const int dx = reflect101(tx0 + tid - kCanvasPad, inW) - q.x;
      int4 e = make_int4(-1, 0, 0, 0);
      if (dx >= 0 && dx < q.w) {
        const int sx = tab.xofs[dx], same = sx + 1 > tab.sw - 1;
        const int a0 = tab.xa[2 * dx], a1 = tab.xa[2 * dx + 1];
#ifdef BSX_PT_NV12
        const int f0 = roi.x + sx, f1 = same ? f0 : f0 + 1, wy = min(f0, W - 4), wu = wy & ~1, c0 = 4 + (f0 & ~1) - wu, c1 = 4 + (f1 & ~1) - wu;
        e = make_int4(wy, (a0 & 0xffff) | (a1 << 16), 0x0c000000 | ((c0 + 1) << 16) | (c0 << 8) | (f0 - wy), 0x0c000000 | ((c1 + 1) << 16) | (c1 << 8) | (f1 - wy));
#else
        if constexpr (YIN) {
          // the 8 bytes from the macropixel of tap 0 hold both taps' macropixels (tap 1 = pixel sx + 1 sits in the same or in the next one; the window is pulled
          // back by 4 where it would pass the row end — tap 1 is then in tap 0's macropixel).  Selector of a tap: its Y, its macropixel's U and V.
          const int p1 = same ? sx : sx + 1, mb = (sx >> 1) * 4, offc = max(min(mb, rowlim - 8), 0), m0 = mb - offc, m1 = (p1 >> 1) * 4 - offc;
          const int y0 = m0 + 2 * (sx & 1), y1 = m1 + 2 * (p1 & 1);
          e = make_int4(offc, (a0 & 0xffff) | (a1 << 16), 0x0c000000 | ((m0 + 3) << 16) | ((m0 + 1) << 8) | y0, 0x0c000000 | ((m1 + 3) << 16) | ((m1 + 1) << 8) | y1);
        } else {
          const int offb = sx * 3, offc = max(min(offb, rowlim - 8), 0), s0 = offb - offc, s1 = same ? s0 : s0 + 3;
          e = make_int4(offc, (a0 & 0xffff) | (a1 << 16), 0x0c000000 | ((s0 + 2) << 16) | ((s0 + 1) << 8) | s0, 0x0c000000 | ((s1 + 2) << 16) | ((s1 + 1) << 8) | s1);
        }
#endif
      }
      colT[tid] = e;
    } else if (tid >= 64 && tid < 64 + SHt) {
      const int ly = tid - 64, dy = reflect101(ty0 + ly - kCanvasPad, inH) - q.y;
      int4 e = make_int4(-1, 0, 0, 0);
#ifdef BSX_PT_NV12
      int2 u = make_int2(0, 0);
#endif
      if (dy >= 0 && dy < q.h) {
        const int sy = tab.yofs[dy], sy0 = min(max(sy, 0), tab.sh - 1), sy1 = min(max(sy + 1, 0), tab.sh - 1);
#ifdef BSX_PT_NV12
        e = make_int4((roi.y + sy0) * pitch_y, (roi.y + sy1) * pitch_y, tab.ya[2 * dy], tab.ya[2 * dy + 1]);
        u = make_int2(((roi.y + sy0) >> 1) * pitch_uv, ((roi.y + sy1) >> 1) * pitch_uv);
#else
        e = make_int4(sy0 * W * FB, sy1 * W * FB, tab.ya[2 * dy], tab.ya[2 * dy + 1]);
#endif
      }
      rowT[ly] = e;
#ifdef BSX_PT_NV12
      rowU[ly] = u;
#endif
    }
    __syncthreads();
    uint32_t lo0[kItems], hi0[kItems], lo1[kItems], hi1[kItems];
#pragma unroll
    for (int k = 0; k < kItems; k++) {                                     // every load of the lane is requested here
      const int i = min(tid + k * kThreads, total - 1), ly = (int)__umulhi((unsigned)i, msw), lx = i - ly * SW;
      const int co = max(colT[lx].x, 0), o0 = max(rowT[ly].x, 0), o1 = rowT[ly].y;
#ifdef BSX_PT_NV12
      struct __attribute__((packed, aligned(1))) U4 { uint32_t v; };            // the Y window: any alignment; the UV window starts on an even byte
      struct __attribute__((packed, aligned(2))) C4 { uint32_t v; };
      const int2 u = rowU[ly];
      lo0[k] = reinterpret_cast<const U4*>(frames + (unsigned)(o0 + co))->v; hi0[k] = reinterpret_cast<const C4*>(suv + (unsigned)(u.x + (co & ~1)))->v;
      lo1[k] = reinterpret_cast<const U4*>(frames + (unsigned)(o1 + co))->v; hi1[k] = reinterpret_cast<const C4*>(suv + (unsigned)(u.y + (co & ~1)))->v;
#else
      struct __attribute__((packed, aligned(1))) U8 { uint64_t v; };            // ONE 8-byte load per source row (byte-aligned: global_load_dwordx2), not two 4-byte ones
      const uint64_t q0 = reinterpret_cast<const U8*>(src + (unsigned)(o0 + co))->v, q1 = reinterpret_cast<const U8*>(src + (unsigned)(o1 + co))->v;
      lo0[k] = (uint32_t)q0; hi0[k] = (uint32_t)(q0 >> 32);
      lo1[k] = (uint32_t)q1; hi1[k] = (uint32_t)(q1 >> 32);
#endif
    }
#pragma unroll
    for (int k = 0; k < kItems; k++) {
      const int i = tid + k * kThreads;
      if (i < total) {
        const int ly = (int)__umulhi((unsigned)i, msw), lx = i - ly * SW;
        const int4 c = colT[lx], r = rowT[ly];
        const int a0 = (short)(c.y & 0xffff), a1 = c.y >> 16, b0 = r.z, b1 = r.w;
        uint32_t t00 = __builtin_amdgcn_perm(hi0[k], lo0[k], (uint32_t)c.z), t01 = __builtin_amdgcn_perm(hi0[k], lo0[k], (uint32_t)c.w);   // row 0: tap 0 / tap 1 as B | G << 8 | R << 16
        uint32_t t10 = __builtin_amdgcn_perm(hi1[k], lo1[k], (uint32_t)c.z), t11 = __builtin_amdgcn_perm(hi1[k], lo1[k], (uint32_t)c.w);   // row 1
        if constexpr (YIN) { t00 = yuv_tap_to_bgr(t00); t01 = yuv_tap_to_bgr(t01); t10 = yuv_tap_to_bgr(t10); t11 = yuv_tap_to_bgr(t11); }      // (the taps arrived as Y | U << 8 | V << 16)
        uint32_t v = 0;                                                    // the model canvas outside in_roi (the bars) is 0
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
          const int h0 = (int)((t00 >> (8 * ch)) & 255u) * a0 + (int)((t01 >> (8 * ch)) & 255u) * a1;
          const int h1 = (int)((t10 >> (8 * ch)) & 255u) * a0 + (int)((t11 >> (8 * ch)) & 255u) * a1;
          const int o = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
          v |= (uint32_t)o << (8 * (2 - ch));                              // BGR2RGB
        }
        tile[ly * kPfS + lx] = (c.x >= 0 && r.x >= 0) ? v : 0u;
      }
    }
  } else
#pragma unroll
  for (int k = 0; k < kItems; k++) {
    const int i = tid + k * kThreads;
    if (i < total) {
      const int ly = (int)__umulhi((unsigned)i, msw), lx = i - ly * SW;
      const int dx = reflect101(tx0 + lx - kCanvasPad, inW) - q.x, dy = reflect101(ty0 + ly - kCanvasPad, inH) - q.y;
      uint32_t v = 0;                                                      // the model canvas outside in_roi (the bars) is 0
      if (dx >= 0 && dx < q.w && dy >= 0 && dy < q.h) {
        int bgr[3];
        sample_linear<3>(src, (long)W * 3, tab, dx, dy, bgr);
        v = (uint32_t)bgr[2] | ((uint32_t)bgr[1] << 8) | ((uint32_t)bgr[0] << 16);  // BGR2RGB
      }
      tile[ly * kPfS + lx] = v;
    }
  }
#pragma unroll
  for (int k = 0; k < 3; k++) lut[tid + k * kThreads] = lut_v[k];
  __syncthreads();
  const int lx = tid & 31, x = tx0 + lx;
  if (lx >= TW || x >= inW) return;
  // two pixels of the lane (rows ly and ly + 8) per pass, their sums in the two halves of packed registers: v_pk_mul_f32 / v_pk_add_f32 do both pixels' multiply
  // (add) of a channel in one instruction — 9 instead of 13 VALU instructions per pixel and tap, the same IEEE operations in the same order (no contraction).
  typedef float f2 __attribute__((ext_vector_type(2)));
  static_assert(kBilPix % 2 == 0, "pixel pairs");
#pragma unroll 1
  for (int it = 0; it < kBilPix; it += 2) {
    const int lyA = (tid >> 5) + 8 * it, lyB = lyA + 8;                   // row B may lie outside the tile: it reads rows < kPfS of the LDS tile and is not stored
    if (lyA >= TH || ty0 + lyA >= inH) return;
    const uint32_t* ta = tile + (lyA + kCanvasPad) * kPfS + (lx + kCanvasPad);      // the centre pixel; tap (dy, dx) at ta[dy * kPfS + dx]
    const uint32_t* tb = ta + 8 * kPfS;
    const uint32_t cA0 = ta[0], cB0 = tb[0];
    f2 sr = {0.f, 0.f}, sg = {0.f, 0.f}, sb = {0.f, 0.f}, ws = {0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 13; k++) {
      const uint32_t cA = ta[kTapY[k] * kPfS + kTapX[k]], cB = tb[kTapY[k] * kPfS + kTapX[k]];
      f2 w = {lut[__builtin_amdgcn_sad_u8(cA, cA0, 0u)], lut[__builtin_amdgcn_sad_u8(cB, cB0, 0u)]};
      w = w * (f2)(bp.space_w[k]);
      const f2 rr = {(float)(cA & 255), (float)(cB & 255)}, gg = {(float)((cA >> 8) & 255), (float)((cB >> 8) & 255)}, bb = {(float)((cA >> 16) & 255), (float)((cB >> 16) & 255)};
      sr = sr + rr * w;
      sg = sg + gg * w;
      sb = sb + bb * w;
      ws = ws + w;
    }
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int y = ty0 + lyA + 8 * h;
      if (h == 1 && (lyB >= TH || y >= inH)) break;
      const unsigned p = (unsigned)(y * inW + x);
      const float wi = __fdiv_rn(1.f, ws[h]);
      int qr = __float2int_rn(__fmul_rn(sr[h], wi)), qg = __float2int_rn(__fmul_rn(sg[h], wi)), qb = __float2int_rn(__fmul_rn(sb[h], wi));
      qr = min(max(qr, 0), 255); qg = min(max(qg, 0), 255); qb = min(max(qb, 0), 255);
      if (OUT & 1) {
        float* o = input + (n * (long)inW * inH + p) * 3;
        o[0] = __fadd_rn(__fmul_rn((float)qr, bp.scale), bp.offset);
        o[1] = __fadd_rn(__fmul_rn((float)qg, bp.scale), bp.offset);
        o[2] = __fadd_rn(__fmul_rn((float)qb, bp.scale), bp.offset);
      }
      if (OUT & 2) input_u8[n * (long)inW * inH + p] = (uint32_t)qr | ((uint32_t)qg << 8) | ((uint32_t)qb << 16);
    }
  }
