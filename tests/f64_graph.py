"""Float64 evaluation of a .tflite graph with PyTorch CPU — TEST INFRASTRUCTURE, independent of the oracle twice over: the file is parsed by the Python reader
(backscrub_amd/tflite_io.py, not the oracle's C++ parser) and every operator is a PyTorch float64 op (not the oracle's loops).  Used by the decision-margin audit
(tests/test_oracle_nn.py) as the "exact" network: |oracle_f32 - f64| measures the rounding error of the oracle's f32 restatement, and — TFLite's real runtime path
(XNNPACK) being another f32 evaluation of the same graph with another summation order — is the yardstick for how far the real reference's logits can be from the
oracle's.  Semantics per SURVEY.md §8(c) (TFLite reference kernels): SAME padding with the extra pixel at the bottom / right, half-pixel / align-corners bilinear,
Convolution2DTransposeBias 2x2 stride 2 = conv_transpose2d."""
import numpy as np
import torch
import torch.nn.functional as F

from backscrub_amd import tflite_io as T


def _same_pad(inp, k, s, d):
    out = -(-inp // s)
    total = max(0, (out - 1) * s + (k - 1) * d + 1 - inp)
    return total // 2, total - total // 2


def _act(y, act):
    return {0: y, 1: F.relu(y), 3: torch.clamp(y, 0, 6)}[act]


def _nchw(a):
    return a.permute(0, 3, 1, 2)


def _nhwc(a):
    return a.permute(0, 2, 3, 1)


def _resize(x, oh, ow, align, half, dtype=torch.float64):
    """TFLite RESIZE_BILINEAR (reference kernel) in float64: in = (o + 0.5) * scale - 0.5 (half_pixel) or o * (in - 1) / (out - 1) (align_corners);
    lo = max(floor, 0), hi = min(ceil, in - 1), fraction from the un-clamped floor."""
    n, h, w, c = x.shape

    def axis(o, i):
        idx = torch.arange(o, dtype=dtype)
        if align and o > 1:
            src = idx * ((i - 1) / (o - 1))
        elif half:
            src = (idx + 0.5) * (i / o) - 0.5
        else:
            src = idx * (i / o)
        fl = torch.floor(src)
        lo = torch.clamp(fl, min=0).long()
        hi = torch.clamp(torch.ceil(src), max=i - 1).long()
        hi = torch.maximum(hi, torch.zeros_like(hi))
        return lo, hi, src - fl
    y0, y1, fy = axis(oh, h)
    x0, x1, fx = axis(ow, w)
    fy = fy.view(1, oh, 1, 1)
    fx = fx.view(1, 1, ow, 1)
    top = x[:, y0][:, :, x0] * (1 - fx) + x[:, y0][:, :, x1] * fx
    bot = x[:, y1][:, :, x0] * (1 - fx) + x[:, y1][:, :, x1] * fx
    return top * (1 - fy) + bot * fy


def _constants(m, dtype):
    val = {}
    for i, t in enumerate(m.tensors):
        if t.data is not None:
            val[i] = torch.from_numpy(np.asarray(t.data).astype(np.float64)).to(dtype) if t.type != T.TENSOR_I32 else torch.from_numpy(np.asarray(t.data))
    return val


def _eval(op, val, dtype=torch.float64):
    """value of op.outputs[0] from the values of its inputs in `val`"""
    i = op.inputs
    name = op.name
    if name == "DEQUANTIZE":
        return val[i[0]]                                         # f16 constant → exact in f32 and f64
    if name in ("CONV_2D", "DEPTHWISE_CONV_2D"):
        x = _nchw(val[i[0]])
        w = val[i[1]]
        b = val[i[2]] if len(i) > 2 and i[2] >= 0 else None
        if name == "CONV_2D":
            wt, groups = w.permute(0, 3, 1, 2), 1
        else:
            wt, groups = w.permute(3, 0, 1, 2), x.shape[1]
        kh, kw = wt.shape[2], wt.shape[3]
        sh, sw, dh, dw = op.opts["stride_h"], op.opts["stride_w"], op.opts["dil_h"], op.opts["dil_w"]
        if op.opts["padding"] == 0:
            pt, pb = _same_pad(x.shape[2], kh, sh, dh)
            pl, pr = _same_pad(x.shape[3], kw, sw, dw)
            x = F.pad(x, (pl, pr, pt, pb))
        return _nhwc(_act(F.conv2d(x, wt.contiguous(), b, stride=(sh, sw), dilation=(dh, dw), groups=groups), op.opts["act"]))
    if name == "FULLY_CONNECTED":
        x = val[i[0]]
        y = F.linear(x.reshape(-1, x.shape[-1]), val[i[1]], val[i[2]] if len(i) > 2 and i[2] >= 0 else None)
        return _act(y.reshape(tuple(x.shape[:-1]) + (y.shape[-1],)) if op.opts.get("keep_num_dims") else y, op.opts["act"])
    if name == "AVERAGE_POOL_2D":
        x = val[i[0]]
        assert op.opts["filter_h"] == x.shape[1] and op.opts["filter_w"] == x.shape[2]
        return x.mean((1, 2), keepdim=True)
    if name in ("ADD", "MUL"):
        a, b = val[i[0]], val[i[1]]
        return _act(a + b if name == "ADD" else a * b, op.opts["act"])
    if name == "RELU":
        return F.relu(val[i[0]])
    if name == "RELU6":
        return torch.clamp(val[i[0]], 0, 6)
    if name == "HARD_SWISH":
        v = val[i[0]]
        return v * torch.clamp(v + 3, 0, 6) / 6
    if name == "LOGISTIC":
        return torch.sigmoid(val[i[0]])
    if name == "CONCATENATION":
        return torch.cat([val[k] for k in i], dim=op.opts["axis"] if op.opts["axis"] >= 0 else op.opts["axis"] + 4)
    if name == "RESIZE_BILINEAR":
        oh, ow = [int(v) for v in val[i[1]].reshape(-1)]
        return _resize(val[i[0]], oh, ow, bool(op.opts["align_corners"]), bool(op.opts["half_pixel_centers"]), dtype)
    if op.code == 32:                                             # Convolution2DTransposeBias: 2x2 stride 2, SAME → no overlap
        x = _nchw(val[i[0]])
        w = val[i[1]].permute(3, 0, 1, 2)                         # [O,kh,kw,I] → [I,O,kh,kw]
        return _nhwc(F.conv_transpose2d(x, w.contiguous(), val[i[2]], stride=2))
    raise AssertionError("operator %s has no float64 mirror" % name)


def run(path, x_nhwc, dtype=torch.float64, model=None):
    """x_nhwc: [1,H,W,3] float (the f32 network input, exactly as the oracle's prep produced it) → dict tensor index → float64 torch tensor (NHWC) for every tensor.
    dtype=torch.float32 runs the same operators on PyTorch's f32 CPU kernels: an f32 evaluation independent of the oracle and of the GPU (the "stand-in device" of
    tests/test_f64_forced_host.py)."""
    m = model or T.load(path)
    val = _constants(m, dtype)
    val[m.inputs[0]] = torch.from_numpy(np.asarray(x_nhwc, dtype=np.float64)).to(dtype)
    for op in m.ops:
        val[op.outputs[0]] = _eval(op, val, dtype)
    return val, m


# ------------------------------------------------------------------------------------------------------------------------------
# Forced evaluation: every STORED tensor of an f32 execution against a float64 evaluation of its own operator group
# ------------------------------------------------------------------------------------------------------------------------------
ULP = 2.0 ** -23        # "an ulp" of a tensor = 2^-23 times its largest magnitude
BAR_FACTOR = 8.0        # three bits of headroom for a different summation order
BAR_FLOOR_ULPS = 4.0    # tensors the oracle happens to round almost exactly


def _as64(a, like):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).reshape(like.shape)


def run_forced(path, x_nhwc, device, model=None):
    """Walk the operators in file order in float64.  After the value v of an output o that is in `device` (tensor index → array of an f32 execution: the GPU's,
    the oracle's, a stand-in's) is computed: local_err[o] = max|v - device[o]|, scale[o] = max|v|, and the walk CONTINUES WITH device[o] widened to float64.
    Every stored tensor is thereby compared with a float64 evaluation of exactly the operators between it and the nearest stored tensors upstream, fed with the
    execution's own values: one kernel's (or one fused launch's) rounding, which does not grow with depth — for any cut set, interiors of fused launches included.
    Returns (local_err, scale, m)."""
    m = model or T.load(path)
    val = _constants(m, torch.float64)
    val[m.inputs[0]] = torch.from_numpy(np.asarray(x_nhwc, dtype=np.float64))
    local_err, scale = {}, {}
    for op in m.ops:
        o = op.outputs[0]
        v = _eval(op, val)
        if o in device and op.name != "DEQUANTIZE":
            d = _as64(device[o], v)
            local_err[o] = float((v - d).abs().max())
            scale[o] = float(v.abs().max())
            v = d
        val[o] = v
    return local_err, scale, m


def bar(local_oracle, scale):
    """what a stored tensor's local error may be: 8 x max(the oracle's own local error on that operator group and input, four f32 ulps of the tensor's magnitude)"""
    return BAR_FACTOR * max(local_oracle, BAR_FLOOR_ULPS * ULP * scale)


def producers(m):
    return {op.outputs[0]: op for op in m.ops}


def audit(path, x_nhwc, device, oracle, exact=None, model=None):
    """The per-tensor table of an execution `device` (tensor index → array) on network input x_nhwc, with the oracle's tensors `oracle` (index → array) as the
    yardstick: for every tensor that is in both and that an operator produces, a dict with
      t, op, shape, local (max|f64 of the group - device|), local_oracle (the same for the oracle, over the SAME cut set), scale, bar, ratio (local / (bar / 8):
      the tensor passes up to ratio 8), acc (max|device - unforced f64|: the accumulated error), acc_ulps (in ulps of the tensor's magnitude), acc_oracle, finite.
    `exact`: the unforced float64 run (run(path, x)[0]) when the caller already has it."""
    m = model or T.load(path)
    prod = producers(m)
    cut = sorted(t for t in device if t in oracle and t in prod and prod[t].name != "DEQUANTIZE")
    dev = {t: device[t] for t in cut}
    loc_d, scale, _ = run_forced(path, x_nhwc, dev, m)
    loc_o, _, _ = run_forced(path, x_nhwc, {t: oracle[t] for t in cut}, m)
    if exact is None:
        exact = run(path, x_nhwc, model=m)[0]
    rows = []
    for t in cut:
        e = exact[t]
        d = _as64(dev[t], e)
        b = bar(loc_o[t], scale[t])
        acc = float((d - e).abs().max())
        mag = max(float(e.abs().max()), 1e-300)
        rows.append({"t": t, "op": prod[t].name, "shape": tuple(e.shape), "local": loc_d[t], "local_oracle": loc_o[t],
                     "scale": scale[t], "bar": b, "ratio": loc_d[t] / (b / BAR_FACTOR) if b > 0 else (0.0 if loc_d[t] == 0 else float("inf")),
                     "acc": acc, "acc_ulps": acc / (ULP * mag), "acc_oracle": float((_as64(oracle[t], e) - e).abs().max()),
                     "finite": bool(np.isfinite(np.asarray(dev[t])).all())})
    return rows


def failing(rows):
    """tensors of an audit table over the bar (NaN-safe: a non-finite error fails)"""
    return [r["t"] for r in rows if not (r["local"] <= r["bar"])]


def format_table(rows):
    out = ["%5s %-18s %-20s %11s %11s %7s %11s %9s" % ("t", "op", "shape", "local", "loc.oracle", "ratio", "accum.", "acc ulps")]
    for r in rows:
        out.append("%5d %-18s %-20s %11.3e %11.3e %7.2f %11.3e %9.1f%s" % (r["t"], r["op"], "x".join(map(str, r["shape"])), r["local"], r["local_oracle"], r["ratio"],
                                                                           r["acc"], r["acc_ulps"], "" if r["local"] <= r["bar"] and r["finite"] else "   <<<< OVER THE BAR"))
    return "\n".join(out)


def summary(rows):
    """(audited tensors, worst local ratio, its tensor, worst accumulated error in ulps, its tensor)"""
    if not rows:
        return 0, 0.0, -1, 0.0, -1
    w = max(rows, key=lambda r: r["ratio"])
    a = max(rows, key=lambda r: r["acc_ulps"])
    return len(rows), w["ratio"], w["t"], a["acc_ulps"], a["t"]


def audit_frames(W, H):
    """The five camera frames every audit runs on: a synthetic scene, uniform noise, all black, all white, black with one 6x6 white square."""
    from backscrub_amd import synth
    black = np.zeros((H, W, 3), np.uint8)
    dot = black.copy()
    dot[H // 2 - 3:H // 2 + 3, W // 2 - 3:W // 2 + 3] = 255
    return [("synthetic", synth.frame(W, H, 2)), ("noise", synth.random_u8((H, W, 3), 23)), ("black", black), ("white", np.full((H, W, 3), 255, np.uint8)), ("dot", dot)]


def oracle_tensors(model, tensors=None):
    """the oracle's tensors after an inference, by file index (Ctx.model() / Model of oracle_py): those with data of their declared shape"""
    out = {}
    for t in (range(model.n_tensors) if tensors is None else tensors):
        shp = model.shape(t)
        a = model.tensor(t)
        if a.size and int(np.prod(shp)) == a.size:
            out[t] = a
    return out


def read_stored(mg, n_tensors, stream):
    """what the library's read-back entry serves for one stream: tensor index → flat f32 array, for every file tensor it does not refuse"""
    out = {}
    for t in range(n_tensors):
        try:
            out[t] = mg.graph_tensor(t, stream)
        except RuntimeError as e:            # BsxError
            if "bsx_debug_tensor:" not in str(e):    # only the entry's own refusal (it names why the path never writes the tensor) means "not stored"
                raise
    return out
