// mask_tile.inc — the general path of mask_tile_k (kernels_img.hip): everything behind its uniform-tile branch, from the extents of the source block to phase 5.
// Included by the kernel itself and by mask_tile_geoms_k (the per-position form of bsx_step_batch_geoms); an include for the reason prep_tile.inc is one.  The
// includer provides: the template or constexpr constants BLEND, WH, MIX, yin, early_bg; bg, bg_stride, frames, mask, outp (the composite's operands and where the
// mask and the composite go), ofinal, outW, outH, q, tab, roi, W, H, tx0, ty0, tid, yuyv, sel, ops; the LDS arrays col_c0, col_c1, col_a0, col_a1, row_r0, row_r1,
// row_b0, row_b1, hq, hs, up, blk; and three expressions: BSX_MT_FRAME, the index of the frame inside `frames` / `outp`; BSX_MT_SLOT, the frame's state slot
// inside `ofinal` — evaluated where `ms` is formed, behind the four table reads; and BSX_MT_MASK_SLOT, the index of the frame's mask inside `mask` — expanded
// behind `const int ms`, the slot formed from BSX_MT_SLOT, which it may name.
// With BSX_MT_EDGE defined (mask_tile_geoms_edge_k: a class whose ROI is off the 4-pixel grid) the tile's columns are anchored to the frame's 4-pixel groups: tx0 =
// 128 tbx - (roi.x & 3), so the first tile starts up to three columns LEFT of the ROI (its halo at -5 reflects at the ROI's bound like every halo column), and the
// composite's operands and stores are the *_edge forms, which own every group that intersects the ROI.  Positions are then single images: bg_stride 0, index 0.
  // extents of the source block: xofs / yofs are monotonic, so the extreme destination rows / columns give them
  // (requesting these four scalar table reads together with the class byte — one scalar round trip instead of two in front of the general path — measured: no
  //  difference on any configuration, profiles/r05e)
  const int gy_lo = max(ty0 - 2, 0), gy_hi = min(ty0 + kTH + 1, roi.h - 1);
  const int gx_lo = max(tx0 - 2, 0), gx_hi = min(tx0 + kTW + 1, roi.w - 1);
  const int smin = min(max(tab.yofs[gy_lo], 0), tab.sh - 1), smax = min(max(tab.yofs[gy_hi] + 1, 0), tab.sh - 1);
  const int cmin = tab.xofs[gx_lo], cmax = min(tab.xofs[gx_hi] + 1, tab.sw - 1);
  const int nsr = smax - smin + 1, ncol = cmax - cmin + 1;
  const int ms = BSX_MT_SLOT;      // the frame's state slot, formed only here: in front of the class byte's load it lengthens the chain every tile waits on (mask_tile_k)
  const uint8_t* const base = ofinal + (long)ms * outW * outH + (long)(q.y + smin) * outW + q.x + cmin;
  // (a) raw block: 12 rows x 64 columns in three loads per lane cover the usual 5x up-scale; anything larger loops below
  uint32_t raw[3];
  const int br = tid >> 6, bc = tid & 63;
#pragma unroll
  for (int j = 0; j < 3; j++) { raw[j] = 0; if (br + 4 * j < nsr && bc < ncol) raw[j] = base[(unsigned)((br + 4 * j) * outW + bc)]; }
  // (b) this lane's table entries
  int t_s = 0, t_a0 = 0, t_a1 = 0;
  if (tid < kHW) {
    const int gx = reflect101(min(tx0 + tid - 2, roi.w + 1), roi.w);
    t_s = tab.xofs[gx]; t_a0 = tab.xa[2 * gx]; t_a1 = tab.xa[2 * gx + 1];
  } else if (tid >= 192 && tid < 192 + kHH) {
    const int gy = reflect101(min(ty0 + (tid - 192) - 2, roi.h + 1), roi.h);
    t_s = tab.yofs[gy]; t_a0 = tab.ya[2 * gy]; t_a1 = tab.ya[2 * gy + 1];
  }
  // (c) composite operands (a shared background requested early is already on its way)
#ifdef BSX_MT_EDGE
  tile_load_blend_operands_edge(ops, bg, frames, W, roi, tx0, ty0, tid, 0, yin, sel);
#else
  tile_load_blend_operands<BLEND, WH, MIX>(ops, bg, bg_stride, frames, BSX_MT_FRAME, W, H, roi, tx0, ty0, tid, 0, early_bg ? 2 : 3, yin, sel);
#endif
  // 1. block and tables into LDS
#pragma unroll
  for (int j = 0; j < 3; j++) if (br + 4 * j < nsr && bc < ncol) blk[(br + 4 * j) * ncol + bc] = (uint8_t)raw[j];
  if (nsr > 12 || ncol > 64)
    for (int r = br; r < nsr; r += 4)
      for (int cc = bc; cc < ncol; cc += 64)
        if (r >= 12 || cc >= 64) blk[r * ncol + cc] = base[(unsigned)(r * outW + cc)];
  if (tid < kHW) {
    col_c0[tid] = (short)(t_s - cmin); col_c1[tid] = (short)(min(t_s + 1, tab.sw - 1) - cmin);
    col_a0[tid] = (short)t_a0; col_a1[tid] = (short)t_a1;
  } else if (tid >= 192 && tid < 192 + kHH) {
    const int r = tid - 192;
    row_r0[r] = (short)(min(max(t_s, 0), tab.sh - 1) - smin); row_r1[r] = (short)(min(max(t_s + 1, 0), tab.sh - 1) - smin);
    row_b0[r] = (short)t_a0; row_b1[r] = (short)t_a1;
  }
  __syncthreads();
  // 2. horizontal pass of the block rows: hq[r][x] = (S0*a0 + S1*a1) >> 4, all 132 columns, k = r * 132 + x walks without a division
  for (int r = tid / kHW, x = tid % kHW; r < nsr;) {
    hq[r * kHW + x] = (uint16_t)((blk[r * ncol + col_c0[x]] * col_a0[x] + blk[r * ncol + col_c1[x]] * col_a1[x]) >> 4);
    x += kThreads % kHW; r += kThreads / kHW;
    if (x >= kHW) { x -= kHW; r++; }
  }
  __syncthreads();
  tile_vertical_pass(hq, up, row_r0, row_r1, 0, row_b0, row_b1, tid);                             // 3.
  __syncthreads();
  tile_hsum5(up, hs, tid);                                                                       // 4.
  __syncthreads();
#ifdef BSX_MT_EDGE
  tile_vsum5_store_edge(hs, mask, outp, ops, W, H, roi, tx0, ty0, tid, yuyv, 0, sel);                                                // 5.
#else
  tile_vsum5_store<BLEND, WH, MIX>(hs, mask, outp, ops, BSX_MT_FRAME, BSX_MT_MASK_SLOT, W, H, roi, tx0, ty0, tid, yuyv, 0, sel);   // 5.
#endif
