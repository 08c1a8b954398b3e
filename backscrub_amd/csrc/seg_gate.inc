// seg_gate.inc — the gate prologue in four parts, each stated once.  seg_gate (kernels_seg.hip: seg_k2_k, seg_tail_k, seg_gate_k) includes them back to back; k3's
// per-frame form (bsx_seg_k3f) runs parts 2 and 3 with its own first loads and part 2 again, from LDS, behind its phase B.  An include for the reason mask_tile.inc
// is one: with the FC layer alone as a function the tile kernels' code moved (tools/isa_same.py).  The includer provides gt, w, tid, and BSX_GATE_PART selects:
//   1  the names: s_gate / s_mean / s_hid in the scratch block BSX_GATE_SCR, the staging area's layout (ps, w1, b1, w2, b2) at BSX_GATE_STAGE, the lane's (c, slice)
//   2  first kSegThreads lanes: slice sum of pooled tensor BSX_GATE_K from its partial sums BSX_GATE_SRC(k) ([n][16], global memory or LDS) → ps[BSX_GATE_K][slice][c]
//   3  first kSegThreads lanes: both FC layers' weights and biases into the staging area
//   4  behind a barrier: means → FC → [FC] → s_gate, with barriers of its own.  BSX_GATE_FC_LANE: the lane is one of the kSegThreads the FC decomposition is over.
//      BSX_GATE_FC_CAPTURE: how the FC lambda takes tid — `&` in seg_gate, as its lambda always did; `tid` in the per-frame form, whose FC layer was a function with tid
//      by value.  It decides when the optimiser sees through the lambda, and each kernel's code moves under the other's form.  Undefines the operands.
#if BSX_GATE_PART == 1
  float* s_gate = BSX_GATE_SCR + kScrGate;
  float* s_mean = BSX_GATE_SCR + kScrGate + 16;
  float* s_hid = BSX_GATE_SCR + kScrGate + 48;
  const SegFc &f1 = gt.fc[0], &f2 = gt.fc[1];
  const int w1n = f1.Cin * f1.Cout, w2n = gt.n_fc == 2 ? f2.Cin * f2.Cout : 0;
  float* ps = BSX_GATE_STAGE;             // [2 parts][16 slices][16 channels] slice sums (every pooled tensor here has 16 channels)
  float* w1 = ps + 512;
  float* b1 = w1 + w1n;
  float* w2 = b1 + f1.Cout;
  float* b2 = w2 + w2n;
  const int c = tid & 15, slice = tid >> 4;
#elif BSX_GATE_PART == 2
    {
      const float* src = BSX_GATE_SRC(BSX_GATE_K);
      float s = 0.f;
#pragma unroll 4
      for (int i = slice; i < gt.part[BSX_GATE_K].n; i += 16) s += src[(unsigned)(i * 16 + c)];
      ps[BSX_GATE_K * 256 + slice * 16 + c] = s;
    }
#undef BSX_GATE_K
#elif BSX_GATE_PART == 3
  {
    const float* g1 = w + f1.w_off;
    const float* g2 = w + f2.w_off;
    for (int i = tid; i < w1n; i += kSegThreads) w1[i] = g1[(unsigned)i];
    for (int i = tid; i < w2n; i += kSegThreads) w2[i] = g2[(unsigned)i];
    if (tid < f1.Cout) b1[tid] = (w + f1.b_off)[(unsigned)tid];
    if (gt.n_fc == 2 && tid < f2.Cout) b2[tid] = (w + f2.b_off)[(unsigned)tid];
  }
#elif BSX_GATE_PART == 4
  const int Cm = gt.sum_parts ? 16 : 16 * gt.n_parts;
  if (tid < Cm) {
    float m = 0.f;
    for (int k = 0; k < gt.n_parts; k++) {
      if (!gt.sum_parts && (tid >> 4) != k) continue;
      float s = 0.f;
#pragma unroll
      for (int sl = 0; sl < 16; sl++) s += ps[k * 256 + sl * 16 + (tid & 15)];
      m += s / gt.part[k].hw;
    }
    s_mean[tid] = m;
  }
  __syncthreads();
  // FC layers: lane = (output, slice of the inputs) — 8 consecutive lanes share an output and meet through DPP.  (One lane per output walked
  // its whole weight row with a stride of Cin floats: every lane on the same two LDS banks, a 16-way conflict per step, 2 us per layer.)
  auto fc = [BSX_GATE_FC_CAPTURE](const SegFc& f, const float* x, const float* wl, const float* bl, float* y) {
    const int out = tid >> 3, ks = tid & 7, kper = f.Cin >> 3;               // Cin is 16 or 32 (checked by the planner)
    float acc = 0.f;
    if (out < f.Cout)
      for (int j = 0; j < kper; j++) acc = fmaf(x[ks * kper + j], wl[out * f.Cin + ks * kper + j], acc);
    acc += dpp_quad(acc, 1);
    acc += dpp_quad(acc, 2);
    acc += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, acc), 0x141, 0xf, 0xf, true));   // row_half_mirror: both quads of the 8
    if (out < f.Cout && ks == 0) y[out] = sg_act(acc + bl[out], f.act);
  };
  if (BSX_GATE_FC_LANE) fc(f1, s_mean, w1, b1, gt.n_fc == 1 ? s_gate : s_hid);
  __syncthreads();
  if (gt.n_fc == 2) {
    if (BSX_GATE_FC_LANE) fc(f2, s_hid, w2, b2, s_gate);
    __syncthreads();
  }
#undef BSX_GATE_SCR
#undef BSX_GATE_STAGE
#undef BSX_GATE_SRC
#undef BSX_GATE_FC_LANE
#undef BSX_GATE_FC_CAPTURE
#endif
#undef BSX_GATE_PART
