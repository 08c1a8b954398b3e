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


def _linear(op, x, w, b):
    """the linear part (no fused activation) of CONV_2D, DEPTHWISE_CONV_2D, FULLY_CONNECTED and Convolution2DTransposeBias on activations x with weights w, bias b"""
    name = op.name
    if name in ("CONV_2D", "DEPTHWISE_CONV_2D"):
        x = _nchw(x)
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
        return _nhwc(F.conv2d(x, wt.contiguous(), b, stride=(sh, sw), dilation=(dh, dw), groups=groups))
    if name == "FULLY_CONNECTED":
        y = F.linear(x.reshape(-1, x.shape[-1]), w, b)
        return y.reshape(tuple(x.shape[:-1]) + (y.shape[-1],)) if op.opts.get("keep_num_dims") else y
    assert op.code == 32                                          # Convolution2DTransposeBias: 2x2 stride 2, SAME → no overlap
    y = _nhwc(F.conv_transpose2d(_nchw(x), w.permute(3, 0, 1, 2).contiguous(), b, stride=2))        # [O,kh,kw,I] → [I,O,kh,kw]
    # the operator's own extent under SAME: stride * (in - 1) + k - pad, pad = max(0, k - (in - 1) % stride - 1) — 1 for an odd input, 0 for an even one; the
    # operator's offset is pad / 2 = 0, so the full result is cropped at the bottom and right
    kh, kw = int(w.shape[1]), int(w.shape[2])
    oh = 2 * (x.shape[1] - 1) + kh - max(0, kh - (x.shape[1] - 1) % 2 - 1)
    ow = 2 * (x.shape[2] - 1) + kw - max(0, kw - (x.shape[2] - 1) % 2 - 1)
    return y[:, :oh, :ow]


def f16(a):
    """round-to-nearest-even half of a float64 tensor, widened back to float64 (numpy's conversion: one rounding, straight from float64; overflow → inf)"""
    with np.errstate(over="ignore"):
        return torch.from_numpy(a.detach().numpy().astype(np.float64).astype(np.float16).astype(np.float64))


def _sliced(a, sl, fn):
    if sl is True:
        return fn(a)
    out = a.clone()
    out[..., sl[0]:sl[1]] = fn(a[..., sl[0]:sl[1]])
    return out


def _w16(w, sl):
    return _sliced(w, sl, lambda t: t.to(torch.float16).to(t.dtype) if t.dtype != torch.float64 else f16(t))      # (weights are f32 values: one rounding either way)


def _x16(x, sl):
    return _sliced(x, sl, lambda t: t.to(torch.float16).to(t.dtype) if t.dtype != torch.float64 else f16(t))


def _masked(w, sl):
    """|w| over the input channels whose operands are rounded, zero elsewhere"""
    if sl is True:
        return w.abs()
    out = torch.zeros_like(w)
    out[..., sl[0]:sl[1]] = w[..., sl[0]:sl[1]].abs()
    return out


def _eval(op, val, dtype=torch.float64, w16=None, x16=False):
    """value of op.outputs[0] from the values of its inputs in `val`.  w16 (True, or a (lo, hi) slice of the input channels): the weights of this CONV_2D are
    rounded to half first; x16: its activations over the same channels too."""
    i = op.inputs
    name = op.name
    if name == "DEQUANTIZE":
        return val[i[0]]                                         # f16 constant → exact in f32 and f64
    if name in ("CONV_2D", "DEPTHWISE_CONV_2D", "FULLY_CONNECTED") or op.code == 32:
        w = val[i[1]]
        x = val[i[0]]
        if w16 and name == "CONV_2D":                            # an operator whose MFMA operands are halves (operand_rounding_rule): f16(w) is exact and known on the host
            w = _w16(w, w16)
            if x16:                                              # the stand-in device of tests/test_f64_forced_host.py rounds the activation operand as well
                x = _x16(x, w16)
        y = _linear(op, x, w, val[i[2]] if len(i) > 2 and i[2] >= 0 else None)
        return y if op.code == 32 else _act(y, op.opts["act"])
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


# ------------------------------------------------------------------------------------------------------------------------------
# Reduced-precision executions: tensors STORED as halves (f32 arithmetic), and convolutions whose MFMA OPERANDS are halves (f32 accumulate)
# ------------------------------------------------------------------------------------------------------------------------------
# (a) half storage.  The device computes an f32 value within B32 (the bar above) of the forced float64 value v and rounds it to the nearest-even half.  Rounding
#     is monotone, so the stored half d satisfies f16(v - B32) <= d <= f16(v + B32), elementwise, with no further tolerance; and d is finite (an overflow past
#     65504 is a finding).
# (b) half operands.  An allowance tensor is carried beside the value: zero at the network input and behind every stored tensor (the device's own value is fed
#     on), pushed through each operator to first order (|w| for the linear ones, x1.5 for hard-swish, x0.25 for the logistic, the product rule for MUL, the
#     operator itself for resize / pool / concat / add), and an operator that rounds its operands evaluates with f16(w) and adds
#         2^-11 conv(|f16(w)|, |x| + allowance_in) + 2^-25 conv(|f16(w)|, 1)
#     for the rounding of the activation operand (the second term: half subnormals).  A tensor passes when |d - v| <= B32 + allowance elementwise; a half-stored
#     one when (a) holds with B32 + allowance in place of B32.
HALF_EPS = 2.0 ** -11          # relative rounding error of a half (normal range)
HALF_SUB = 2.0 ** -25          # absolute rounding error of a half in its subnormal range
OPERAND_MODES = ("fast", "fast16")
GEMM_MIN_ROWS = 8192

_STEP_RE = r"^\s*(\d+) (\w+)\s+(\S.*?)\s+in (\d+)x(\d+)x(\d+) -> out (\d+)x(\d+)x(\d+) .* t(-?\d+)->t(\d+)$"


def operand_rounding_rule(plan, m, mode, n):
    """Which operators round their operands to half — THE one statement of it, read from launch_step (kernels_nn.hip), a function of the plan's step lines, the
    BSX_F16_GEMM mode and the stepped batch size n:
      * the expand (1x1) of every fused expand + depthwise pair the plan announces;
      * every 1x1 convolution launch_step sends to pw_gemm_f16s_k: n * OH * OW >= 8192 rows, Cin % 4 == 0, Cin >= 8, cout_pad % 16 == 0 — except the one inside
        the fused head kernel (f32 throughout).
    The step line does not print cout_pad.  The planner pads a 1x1 convolution's Cout to its channel tile, 16 or 32 (plan.cpp), so launch_step's `cout_pad % 16 == 0`
    and `cout_pad >= 16` hold for every pwconv step and are no clause below; its `k16_pad > 0` (half weights exist: the Cin clauses again, and more than 4 pixels per
    frame) is the OH * OW clause.  Where this names an operator the device does not round, that operator gets an allowance it has not earned — the loose side; the
    audit record lists the operators named, and on the audited graphs they are the ones launch_step rounds.
    Returns {output tensor of the file's CONV_2D: True, or the (lo, hi) slice of its input channels the step covers (a concat branch folded into a per-frame bias is
    computed by an f32 kernel)}.  An operator this forgets gets no allowance and fails the audit."""
    if mode not in OPERAND_MODES:
        return {}
    import re
    lines = plan.split("\n")
    steps, expands = {}, set()
    head_fused = False
    last = None
    for line in lines:
        mm = re.match(_STEP_RE, line)
        if mm:
            last = int(mm.group(1))
            steps[last] = {"kind": mm.group(2), "label": mm.group(3), "Cin": int(mm.group(6)), "OH": int(mm.group(7)), "OW": int(mm.group(8)), "Cout": int(mm.group(9)),
                           "in0": int(mm.group(10)), "out": int(mm.group(11))}
        elif "^ fused with steps 1 and 2" in line:
            head_fused = True
        elif re.search(r"\^ fused with step \d+ \(expand", line):
            expands.add(last)
    prod = producers(m)
    rule = {}
    for i, st in sorted(steps.items()):
        if st["kind"] != "pwconv" or (head_fused and i <= 2):
            continue
        gemm = n * st["OH"] * st["OW"] >= GEMM_MIN_ROWS and st["Cin"] % 4 == 0 and st["Cin"] >= 8 and st["OH"] * st["OW"] > 4
        if not (i in expands or gemm):
            continue
        mm = re.match(r"conv#(\d+)", st["label"])
        assert mm, "step %d (%s) names no convolution of the file" % (i, st["label"])
        op = m.ops[int(mm.group(1))]
        assert op.name == "CONV_2D", (i, st["label"], op.name)
        cin_file = int(m.tensors[op.inputs[1]].shape[3])
        sl = True
        if cin_file != st["Cin"]:                                 # the step covers one branch of a concatenation
            cat = prod[op.inputs[0]]
            assert cat.name == "CONCATENATION" and st["in0"] in cat.inputs, (i, st["label"])
            lo = 0
            for t in cat.inputs:
                if t == st["in0"]:
                    break
                lo += int(m.tensors[t].shape[3])
            sl = (lo, lo + st["Cin"])
        rule[op.outputs[0]] = sl
    return rule


def moved_convs(plan, m):
    """The graph rewrite "1x1 convolution moved below its resize" as the plan's step lines state it: a step `conv#C@lo` whose output is a synthetic tensor S (an index
    past the file's tensors) followed by `resize#R'` from S to the file convolution's output Y.  The device stores S, not the file's resize output: in a 16-bit storage
    mode S is rounded where the file has no tensor at all, so the audit has to see it.  Returns {S: (C, R, Y)} (operator indices of the file) for the plain ones
    (S = CONV_C applied to the input of RESIZE_R; a variant with a folded multiply is not stored by any path and is left out)."""
    import re
    steps = [(mm.group(2), mm.group(3), int(mm.group(10)), int(mm.group(11))) for mm in re.finditer(_STEP_RE, plan, re.M)]
    out = {}
    for (kind, label, _, s_out), (kind2, label2, in2, y) in zip(steps, steps[1:]):
        a, b = re.fullmatch(r"conv#(\d+)@lo", label), re.fullmatch(r"resize#(\d+)'", label2)
        if kind == "pwconv" and kind2 == "resize" and a and b and in2 == s_out and s_out >= len(m.tensors):
            c, r = m.ops[int(a.group(1))], m.ops[int(b.group(1))]
            assert c.name == "CONV_2D" and r.name == "RESIZE_BILINEAR" and c.inputs[0] == r.outputs[0] and c.outputs[0] == y and c.opts["act"] == 0, (label, label2)
            out[s_out] = (int(a.group(1)), int(b.group(1)), y)
    return out


def _allow(op, val, al, w16):
    """first-order bound on |device value - float64 value| of op.outputs[0] given the bounds `al` of its inputs (absent = zero) — None while everything is zero"""
    i, name = op.inputs, op.name
    a = [al.get(k) for k in i]
    if name in ("CONV_2D", "DEPTHWISE_CONV_2D", "FULLY_CONNECTED") or op.code == 32:
        w, x = val[i[1]], val[i[0]]
        out = None
        if w16 and name == "CONV_2D":
            wr = _masked(_w16(w, w16), w16)
            out = HALF_EPS * _linear(op, x.abs() + (a[0] if a[0] is not None else 0.0), wr, None) + HALF_SUB * _linear(op, torch.ones_like(x), wr, None)
            w = _w16(w, w16)
        if a[0] is not None:
            lin = _linear(op, a[0], w.abs(), None)
            out = lin if out is None else out + lin
        return out                                                # relu / relu6 (the fused activations): unchanged
    if name in ("RELU", "RELU6"):
        return a[0]
    if name == "HARD_SWISH":
        return None if a[0] is None else 1.5 * a[0]
    if name == "LOGISTIC":
        return None if a[0] is None else 0.25 * a[0]
    if name == "ADD":
        if a[0] is None or a[1] is None:
            return a[0] if a[1] is None else a[1] + torch.zeros_like(val[i[0]] + val[i[1]])
        return a[0] + a[1]
    if name == "MUL":
        if a[0] is None and a[1] is None:
            return None
        z = torch.zeros_like(val[i[0]] * val[i[1]])
        return z + (val[i[1]].abs() * a[0] if a[0] is not None else 0.0) + (val[i[0]].abs() * a[1] if a[1] is not None else 0.0)
    if name == "AVERAGE_POOL_2D":
        return None if a[0] is None else a[0].mean((1, 2), keepdim=True)
    if name == "CONCATENATION":
        if all(k is None for k in a):
            return None
        return torch.cat([k if k is not None else torch.zeros_like(val[t]) for k, t in zip(a, i)], dim=op.opts["axis"] if op.opts["axis"] >= 0 else op.opts["axis"] + 4)
    if name == "RESIZE_BILINEAR":
        if a[0] is None:
            return None
        oh, ow = [int(v) for v in val[i[1]].reshape(-1)]
        return _resize(a[0], oh, ow, bool(op.opts["align_corners"]), bool(op.opts["half_pixel_centers"]))
    if name == "DEQUANTIZE":
        return None
    raise AssertionError("operator %s has no allowance rule" % name)


def run_forced_reduced(path, x_nhwc, device, rounding=None, model=None, moved=None):
    """run_forced for a reduced-precision execution.  rounding: operand_rounding_rule's result.  Returns {t: (v, allowance or None, d)} for the tensors of `device`
    (float64 tensors: the forced value, the first-order operand allowance, the device's value) — the walk continues with d, allowance zero.
    moved: moved_convs' result; a synthetic tensor S of it that is in `device` is compared with the convolution applied to the resize's INPUT, and the walk
    continues with the resize of the device's S in place of the file convolution's output."""
    m = model or T.load(path)
    rounding = rounding or {}
    at_conv = {c: (s_, r) for s_, (c, r, _) in (moved or {}).items() if s_ in device}
    val = _constants(m, torch.float64)
    val[m.inputs[0]] = torch.from_numpy(np.asarray(x_nhwc, dtype=np.float64))
    al, out = {}, {}
    for k, op in enumerate(m.ops):
        o = op.outputs[0]
        r = rounding.get(o)
        if k in at_conv:
            s_, rz = at_conv[k]
            assert not rounding, "a moved convolution under an operand-rounding mode"
            rop = m.ops[rz]
            vs = _linear(op, val[rop.inputs[0]], val[op.inputs[1]], val[op.inputs[2]] if len(op.inputs) > 2 and op.inputs[2] >= 0 else None)
            ds = _as64(device[s_], vs)
            out[s_] = (vs, None, ds)
            oh, ow = [int(q) for q in val[rop.inputs[1]].reshape(-1)]
            val[o] = _resize(ds, oh, ow, bool(rop.opts["align_corners"]), bool(rop.opts["half_pixel_centers"]))
            continue
        v = _eval(op, val, w16=r)
        a = _allow(op, val, al, r) if (rounding and op.name != "DEQUANTIZE") else None
        if o in device and op.name != "DEQUANTIZE":
            d = _as64(device[o], v)
            out[o] = (v, a, d)
            v, a = d, None
        val[o] = v
        if a is not None:
            al[o] = a
    return out, m


def audit_reduced(path, x_nhwc, device, oracle, half=(), rounding=None, exact=None, model=None, bar_scale=1.0, moved=None):
    """The per-tensor table of a reduced-precision execution.  half: the tensors of `device` that were stored as halves.  Per tensor of the cut set (as audit()):
      t, op, shape, half, b32 (bar_scale x the f32 bar), allow (largest operand allowance), outside (elements outside their interval / bound: must be 0), first (flat
      index of the first one, -1), worst (max |d - v| / (B32 + allowance); a half-stored tensor may exceed 1 by its storage rounding), local, local_oracle, scale,
      acc (max |device - unforced float64|), finite."""
    m = model or T.load(path)
    prod = producers(m)
    moved = {s_: v for s_, v in (moved or {}).items() if s_ in device}      # (a moved convolution has no tensor in the oracle: its B32 is the floor alone, the stricter choice)
    cut = sorted(t for t in device if t in oracle and t in prod and prod[t].name != "DEQUANTIZE")
    dev = {t: device[t] for t in cut + sorted(moved)}
    walk, _ = run_forced_reduced(path, x_nhwc, dev, rounding, m, moved)
    loc_o, _, _ = run_forced(path, x_nhwc, {t: oracle[t] for t in cut}, m)
    if exact is None:
        exact = run(path, x_nhwc, model=m)[0]
    exact = dict(exact)
    for s_, (c, r, _) in moved.items():
        cop = m.ops[c]
        exact[s_] = _linear(cop, exact[m.ops[r].inputs[0]], exact[cop.inputs[1]], exact[cop.inputs[2]] if len(cop.inputs) > 2 and cop.inputs[2] >= 0 else None)
        loc_o[s_] = 0.0
    names = {t: prod[t].name for t in cut}
    names.update({s_: "CONV_2D@lo" for s_ in moved})
    cut = sorted(cut + sorted(moved))
    rows = []
    for t in cut:
        v, a, d = walk[t]
        scale = float(v.abs().max())
        b32 = bar_scale * bar(loc_o[t], scale)
        tol = b32 + a if a is not None else torch.full_like(v, b32)
        err = (d - v).abs()
        finite = bool(torch.isfinite(d).all())
        if t in half:
            bad = ~((d >= f16(v - tol)) & (d <= f16(v + tol)))     # (NaN-safe: a NaN is outside)
        else:
            bad = ~(err <= tol)
        idx = torch.nonzero(bad.reshape(-1))
        ratio = torch.where(tol > 0, err / tol, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
        rows.append({"t": t, "op": names[t], "shape": tuple(v.shape), "half": t in half, "b32": b32, "allow": float(a.max()) if a is not None else 0.0,
                     "outside": int(idx.numel()), "first": int(idx[0]) if idx.numel() else -1, "worst": float(ratio.max()), "local": float(err.max()),
                     "local_oracle": loc_o[t], "scale": scale, "acc": float((d - exact[t]).abs().max()), "finite": finite})
    return rows


def failing_reduced(rows):
    return [r["t"] for r in rows if r["outside"] or not r["finite"]]


def format_table_reduced(rows):
    out = ["%5s %-18s %-20s %4s %11s %11s %11s %9s %9s %9s %11s" % ("t", "op", "shape", "f16", "B32", "allowance", "local", "worst", "outside", "first", "accum.")]
    for r in rows:
        out.append("%5d %-18s %-20s %4s %11.3e %11.3e %11.3e %9.3g %9d %9d %11.3e%s" % (
            r["t"], r["op"], "x".join(map(str, r["shape"])), "f16" if r["half"] else "f32", r["b32"], r["allow"], r["local"], r["worst"], r["outside"], r["first"], r["acc"],
            "   <<<< OUTSIDE" if r["outside"] or not r["finite"] else ""))
    return "\n".join(out)


def not_half_representable(a):
    """how many values of an f32 array a half cannot hold (what shows that a tensor read back as f32 really is one)"""
    a = np.asarray(a, dtype=np.float32)
    with np.errstate(over="ignore"):
        return int((a.astype(np.float16).astype(np.float32) != a).sum())


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
        if not 0 <= t < model.n_tensors:          # (a rewrite's synthetic tensor: the oracle evaluates the file as it is)
            continue
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
