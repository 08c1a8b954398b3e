// tile_class.inc — the body of tile_class_k (kernels_img.hip), included by the kernel itself and by tile_class_geoms_k (the per-position form of
// bsx_step_batch_geoms); an include for the reason prep_tile.inc is one.  The includer provides tid, outW, tab, roi, ntx, nty and two expressions: BSX_CLS_FRAME,
// the frame's model-resolution state at in_roi's origin, and BSX_CLS_BYTE(t), the class byte of its tile t; optionally BSX_CLS_SHIFT, the columns (0-3) by which the
// first tile column starts left of the ROI.
  __shared__ uint8_t f255[kClsMaxItems], f0[kClsMaxItems];
  __shared__ int cmn[kClsMaxTx], cmx[kClsMaxTx];
  if (tid < ntx) {
#ifdef BSX_CLS_SHIFT                       /* tile columns anchored to the frame's 4-pixel groups (tile_class_geoms_edge_k): the tile mask_tile.inc works on */
    const int tx0 = tid * kTW - (BSX_CLS_SHIFT);
#else
    const int tx0 = tid * kTW;
#endif
    const int gx_lo = max(tx0 - 2, 0), gx_hi = min(tx0 + kTW + 1, roi.w - 1);
    cmn[tid] = tab.xofs[gx_lo]; cmx[tid] = min(tab.xofs[gx_hi] + 1, tab.sw - 1);
  }
  __syncthreads();
  const uint8_t* const fr = BSX_CLS_FRAME;
  struct __attribute__((packed, aligned(1))) U4 { uint32_t v; };
  const int items = tab.sh * ntx;
  for (int i = tid; i < items; i += kThreads) {
    const int r = i / ntx, tbx = i - r * ntx, c0 = cmn[tbx], len = cmx[tbx] - c0 + 1;
    const uint8_t* p = fr + (unsigned)(r * outW + c0);
    uint32_t a = 0xFFFFFFFFu, o = 0u;
    if (len >= 4) {
#pragma unroll 4
      for (int k = 0; k + 4 <= len; k += 4) { const uint32_t w = reinterpret_cast<const U4*>(p + k)->v; a &= w; o |= w; }
      const uint32_t w = reinterpret_cast<const U4*>(p + len - 4)->v;      // the last four bytes (overlapping the loop's: AND / OR do not care)
      a &= w; o |= w;
    } else {
      for (int k = 0; k < len; k++) { const uint32_t w = p[k] * 0x01010101u; a &= w; o |= w; }
    }
    f255[i] = a == 0xFFFFFFFFu; f0[i] = o == 0u;
  }
  __syncthreads();
  for (int t = tid; t < ntx * nty; t += kThreads) {
    const int tby = t / ntx, tbx = t - tby * ntx, ty0 = tby * kTH;
    const int gy_lo = max(ty0 - 2, 0), gy_hi = min(ty0 + kTH + 1, roi.h - 1);
    const int smin = min(max(tab.yofs[gy_lo], 0), tab.sh - 1), smax = min(max(tab.yofs[gy_hi] + 1, 0), tab.sh - 1);
    int all255 = 1, all0 = 1;
    for (int r = smin; r <= smax; r++) { all255 &= f255[r * ntx + tbx]; all0 &= f0[r * ntx + tbx]; }
    BSX_CLS_BYTE(t) = (uint8_t)(all255 ? 1 : (all0 ? 2 : 0));
  }
