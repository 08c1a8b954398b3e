// seg_k3_rows.inc — k3's output rows of one tile, every fourth from BSX_K3R_FIRST: t = z + act(dw3x3(z)) on the MFMA's own lanes, lo = pw2(t), the store, and the lane's
// `sum` of what it stored.  The row loop of seg_k3_k and of phase B of bsx_seg_k3f (kernels_seg.hip); an include for the reason seg_gated_row.inc is one.  The includer
// provides: d, r0, c0, li, cq4, coz, wd, bias_d, cl_dw, cl_2, wr, bias2, lo_out, sum, H16; and three macros: BSX_K3R_FIRST, the first tile row of this wave;
// BSX_K3R_Z and BSX_K3R_ZRW, the base and the floats per row of a z block whose row BSX_K3R_ZROW(py) + fy holds the row above (fy = 0), at and below tile row py.
      for (int py = BSX_K3R_FIRST; py < d.TR && r0 + py < d.H2; py += 4) {
        const f4v zc = ldv(BSX_K3R_Z + (BSX_K3R_ZROW(py) + 1) * BSX_K3R_ZRW + coz[1]);
        const float4 dv = clamp4(tof4(dw3x3(BSX_K3R_Z, BSX_K3R_ZRW, BSX_K3R_ZROW(py), coz, wd) + bias_d), cl_dw);
        const f4acc acc = mma16(f4add(dv, tof4(zc)), wr);                  // dw epilogue: activation, then + residual z; straight into pw2
        float4 v = acc_quad(acc);
        if (li < d.TC && c0 + li < d.W2) {
          v = as_stored<H16>(clamp4(f4add(v, bias2), cl_2));
          stg4<H16>(lo_out, (unsigned)(((r0 + py) * d.W2 + c0 + li) * 16 + cq4), v);
          sum = f4add(sum, v);
        }
      }
#undef BSX_K3R_FIRST
#undef BSX_K3R_Z
#undef BSX_K3R_ZRW
#undef BSX_K3R_ZROW
