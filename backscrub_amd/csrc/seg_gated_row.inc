// seg_gated_row.inc — one 16-column row of z = act(pw1(skip * g + up(lo))), zero outside the image: the loop body of gated_compute (seg_k3_k, seg_tail_k) and of phase A
// of bsx_seg_k3f (kernels_seg.hip).  An include, not a function, for the reason mask_tile.inc is one: each kernel keeps the token stream it had, and with it its code
// (tools/isa_same.py).  The includer provides: iy, the row's image row (wave-uniform), and H, HL, hs, half_pixel; the lane's column constants xo0, xo1 (col_l offsets
// of its interpolation pair inside a staged row), dx and ecol_in; gv, wr, bias, cl; and three macros: BSX_GR_LO_ROW(y), the staged low-resolution row y;
// BSX_GR_SKIP, the lane's skip operand of the row; BSX_GR_STORE(v), the store of the lane's z quad.
    const bool row_in = iy >= 0 && iy < H;                           // scalar
    int y0, y1;
    float dy;
    up_axis(min(max(iy, 0), H - 1), hs, half_pixel, HL, &y0, &y1, &dy);
    const float* l0 = BSX_GR_LO_ROW(y0);
    const float* l1 = BSX_GR_LO_ROW(y1);
    const float4 ta = ld4(l0 + xo0), tb = ld4(l1 + xo0), tc = ld4(l0 + xo1), td = ld4(l1 + xo1);
    const float w00 = (1.f - dy) * (1.f - dx), w10 = dy * (1.f - dx), w01 = (1.f - dy) * dx, w11 = dy * dx;
    const float4 sk = BSX_GR_SKIP;
    float4 a;
    a.x = fmaf(sk.x, gv.x, fmaf(td.x, w11, fmaf(tc.x, w01, fmaf(tb.x, w10, ta.x * w00))));
    a.y = fmaf(sk.y, gv.y, fmaf(td.y, w11, fmaf(tc.y, w01, fmaf(tb.y, w10, ta.y * w00))));
    a.z = fmaf(sk.z, gv.z, fmaf(td.z, w11, fmaf(tc.z, w01, fmaf(tb.z, w10, ta.z * w00))));
    a.w = fmaf(sk.w, gv.w, fmaf(td.w, w11, fmaf(tc.w, w01, fmaf(tb.w, w10, ta.w * w00))));
    const f4acc acc = mma16(a, wr);
    float4 v = acc_quad(acc);
    v = (ecol_in && row_in) ? clamp4(f4add(v, bias), cl) : f4zero();
    BSX_GR_STORE(v);
#undef BSX_GR_LO_ROW
#undef BSX_GR_SKIP
#undef BSX_GR_STORE
