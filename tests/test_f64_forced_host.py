"""The per-tensor bar of the layer audit (tests/f64_graph.py: run_forced / audit), proven fair and sharp on the host.

The GPU audit (tests/test_gpu_layers.py) passes a stored tensor t when

    local_err_dev[t] <= 8 * max(local_err_oracle[t], 4 * 2^-23 * scale[t])

where local_err is the distance from a float64 evaluation of the operators between t and the nearest stored tensors upstream, fed with the execution's own values.
Nothing here runs on a GPU: the "device" is an f32 evaluation that is independent of both the oracle and the HIP kernels — f64_graph's operators on PyTorch's f32
CPU kernels.
  fairness   that stand-in stays below HALF the bar on every model fixture, on the five inputs the GPU test uses, for two cut sets (every tensor; every 12th + output)
  sharpness  one channel of one stored tensor scaled by 1 + 2^-16 fails at that tensor, fails at every direct consumer the change moves by more than its bar, and
             fails nowhere else — in particular at no tensor upstream
  edges      a border row, a border column or one corner pixel replaced by its inward neighbour fails on the noise input
"""
import functools
import os

import numpy as np
import pytest

import deeplab_size_cases as D
from conftest import reference_model_path, synthetic_model_path
from model_size_cases import BY_NAME, CASES as SIZE_CASES, model_file

torch = pytest.importorskip("torch")

import f64_graph as G  # noqa: E402

W, H = 640, 480
SHIPPED = ["lite", "full", "mlkit", "lite-synthetic", "full-synthetic", "mlkit-synthetic", "deeplab-synthetic"]
# the Meet / MLKit graphs at other input sizes (tests/model_size_cases.py) and the three smallest DeepLab graphs (tests/deeplab_size_cases.py: 33x33 and 9x9 have
# dilations that reach past their maps, 65x97 is not square): the bar must be fair there too
MODELS = SHIPPED + [c.name for c in SIZE_CASES] + D.HOST_PROOF
INPUTS = ["synthetic", "noise", "black", "white", "dot"]
_SIZED = {}


@pytest.fixture(scope="module", autouse=True)
def _sized_models(tmp_path_factory):
    _SIZED["dir"] = tmp_path_factory.mktemp("sized_models")


def _path(model):
    if model in BY_NAME:
        return model_file(BY_NAME[model], _SIZED["dir"])
    if model in D.BY_NAME:
        return D.model_file(D.BY_NAME[model], _SIZED["dir"])
    key, _, syn = model.partition("-")
    return synthetic_model_path(key) if syn else reference_model_path(key)


@functools.lru_cache(maxsize=None)
def _ctx(model):
    from oracle import oracle_py
    oracle_py.build()
    return oracle_py.Ctx(_path(model), W, H)


@functools.lru_cache(maxsize=4)
def _case(model, inp):
    """(path, network input, oracle tensors, unforced f64 tensors, parsed model, f32 stand-in tensors by index) of one model on one of the five inputs"""
    path = _path(model)
    oc = _ctx(model)
    if inp == "noise tensor":                # f32 noise over the model's normalised range as the NETWORK input: no letter-box borders, no 8-bit grid
        lo = -1.0 if model.startswith("deeplab") else 0.0
        x = np.random.default_rng(5).uniform(lo, 1.0, (1, oc.inH, oc.inW, oc.inC)).astype(np.float32)
        oc.model().invoke(x[0])
    else:
        x = oc.prep(dict(G.audit_frames(W, H))[inp])[None]
        oc.infer()
    ot = G.oracle_tensors(oc.model())
    exact, m = G.run(path, x)
    f32, _ = G.run(path, x, dtype=torch.float32, model=m)
    prod = G.producers(m)
    dev = {t: f32[t].numpy() for t in prod if prod[t].name != "DEQUANTIZE"}
    return path, x, ot, exact, m, dev


@pytest.mark.parametrize("model", MODELS)
def test_the_f32_stand_in_passes_at_half_the_bar(model):
    """Fairness: an honest f32 evaluation in another summation order must pass with room to spare, else the bar would fail correct kernels.  An input on which the
    stand-in itself exceeded half the bar (ratio 4 of 8) would not be usable for the GPU audit: all five stay in."""
    if not os.path.exists(_path(model)):
        pytest.fail("model fixture %s is missing" % _path(model))
    worst = (0.0, None)
    for inp in INPUTS:
        path, x, ot, exact, m, dev = _case(model, inp)
        every = sorted(dev)
        for cutname, cut in (("every tensor", every), ("every 12th + output", sorted(set(every[::12] + [m.outputs[0]])))):
            rows = G.audit(path, x, {t: dev[t] for t in cut}, ot, exact, m)
            n, ratio, at, acc, acc_at = G.summary(rows)
            print("%-18s %-9s %-20s %3d tensors, worst local ratio %.2f at t%d, worst accumulated error %.0f ulps at t%d" % (model, inp, cutname, n, ratio, at, acc, acc_at))
            assert n == len(cut), "the oracle lacks %d tensors of the cut set" % (len(cut) - n)
            assert all(r["finite"] for r in rows)
            assert ratio <= G.BAR_FACTOR / 2, "%s / %s / %s: the f32 stand-in is at %.2f of the floor at t%d (the bar is at 8, half of it at 4)\n%s" % (
                model, inp, cutname, ratio, at, G.format_table(rows))
            worst = max(worst, (ratio, "%s/%s t%d" % (inp, cutname, at)))
    print("%s: worst ratio of the stand-in %.2f (%s)" % (model, worst[0], worst[1]))


def _kind(op, m):
    if op.name == "CONV_2D":
        w = m.tensors[op.inputs[1]].shape
        return "regular convolution" if w[1] * w[2] > 1 else "1x1 convolution"
    if op.code == 32:
        return "Convolution2DTransposeBias"
    return {"DEPTHWISE_CONV_2D": "depthwise", "AVERAGE_POOL_2D": "pooled mean", "FULLY_CONNECTED": "fully connected", "LOGISTIC": "logistic gate",
            "RESIZE_BILINEAR": "bilinear resize", "ADD": "residual add", "CONCATENATION": "concatenation"}.get(op.name)


# the kinds each architecture's file contains (MLKit's gates are 1x1 convolutions, its decoder pools a sum instead of a concatenation; DeepLab has no gate)
KINDS = {
    "lite": ["regular convolution", "depthwise", "1x1 convolution", "pooled mean", "fully connected", "logistic gate", "bilinear resize",
             "Convolution2DTransposeBias", "residual add", "concatenation"],
    "mlkit": ["regular convolution", "depthwise", "1x1 convolution", "pooled mean", "logistic gate", "bilinear resize", "Convolution2DTransposeBias", "residual add"],
    "deeplab-synthetic": ["regular convolution", "depthwise", "1x1 convolution", "pooled mean", "bilinear resize", "residual add", "concatenation"],
}


@pytest.mark.parametrize("model", list(KINDS))
def test_a_2_to_the_minus_16_change_of_one_channel_fails_there_and_downstream_only(model):
    """Sharpness.  Per operator kind: the first tensor of that kind (file order, synthetic frame first, then noise) on which the mutation is above the tensor's own
    bar — 2^-16 of its largest channel > bar + the stand-in's local error there, a choice made from the oracle's figures — gets that channel scaled by 1 + 2^-16.
    Then: every tensor passed before; the mutated tensor fails; every direct consumer that the change moves (in float64) by more than its bar plus its own local
    error fails; nothing else fails, so nothing upstream.
    This is narrower than "fails at that tensor and at its direct consumers" in two stated ways.  A consumer that reads the channel through a small weight moves by
    less than its own bar and cannot fail: it is required to fail only when its float64 movement exceeds bar + local error (then it must, by the triangle
    inequality).  And a tensor whose yardstick — the oracle's own f32 rounding, e.g. of a sequential pool — is coarser than 2^-16 is passed over for the next of
    its kind; the tensors passed over are printed per kind."""
    found, skipped = {}, {}
    for inp in ("synthetic", "noise"):
        path, x, ot, exact, m, dev = _case(model, inp)
        base = {r["t"]: r for r in G.audit(path, x, dev, ot, exact, m)}
        assert not G.failing(base.values()), "unmutated run fails at %s" % G.failing(base.values())
        consumers = {}
        for op in m.ops:
            for i in op.inputs:
                consumers.setdefault(i, []).append(op)
        order = [op.outputs[0] for op in m.ops]
        for op in m.ops:
            kind, t = _kind(op, m), op.outputs[0]
            if kind is None or kind in found or t not in dev:
                continue
            a = dev[t]
            mag = np.abs(a).reshape(-1, a.shape[-1]).max(0)
            c = int(mag.argmax())                                    # the largest channel: at least a quarter of the tensor's magnitude by construction
            assert mag[c] >= 0.25 * np.abs(a).max()
            if not 2.0 ** -16 * mag[c] > base[t]["bar"] + base[t]["local"]:
                skipped.setdefault(kind, []).append("t%d/%s" % (t, inp))  # the yardstick itself (the oracle's f32 pool) is coarser than 2^-16 here: try the next of the kind
                continue
            b = a.copy()
            b[..., c] *= np.float32(1 + 2.0 ** -16)
            mut = dict(dev)
            mut[t] = b
            rows = G.audit(path, x, mut, ot, exact, m)
            fails = G.failing(rows)
            must = []
            for cop in consumers.get(t, []):
                o = cop.outputs[0]
                def at(d):
                    val = dict(exact)                                # constants and de-quantised weights; every activation it reads comes from d
                    val.update({i: torch.from_numpy(d[i].astype(np.float64)) for i in cop.inputs if i in d})
                    return G._eval(cop, val)
                moved = float((at(mut) - at(dev)).abs().max())
                if moved > base[o]["bar"] + base[o]["local"]:
                    must.append(o)
            direct = [cop.outputs[0] for cop in consumers.get(t, [])]
            upstream = [u for u in fails if order.index(u) < order.index(t)]
            print("%-18s %-27s t%-3d channel %-3d on %-9s: failed at %s; direct consumers %s, of which moved past their bar %s; upstream failures %s" % (
                model, kind, t, c, inp, fails, direct, must, upstream))
            assert t in fails, "%s t%d: the mutated tensor passes" % (kind, t)
            assert not upstream, "%s t%d: upstream tensors %s fail" % (kind, t, upstream)
            assert set(must) <= set(fails), "%s t%d: consumers %s were moved past their bar and pass" % (kind, t, sorted(set(must) - set(fails)))
            assert set(fails) <= {t} | set(direct), "%s t%d: tensors %s fail that do not read it" % (kind, t, sorted(set(fails) - {t} - set(direct)))
            found[kind] = t
    for kind in KINDS[model]:
        print("%-18s %-27s mutated t%s; passed over before it (2^-16 of the largest channel below bar + local error): %s" % (model, kind, found.get(kind), skipped.get(kind, [])))
    missing = [k for k in KINDS[model] if k not in found]
    assert not missing, "no tensor of kind %s on which 2^-16 is above the bar" % missing


EDGE_FAULTS = ("last row", "last column", "first row", "first column", "corner pixel")


def _edge_fault(a, what):
    b = a.copy()
    if what == "last row":
        b[:, -1] = b[:, -2]
    elif what == "last column":
        b[:, :, -1] = b[:, :, -2]
    elif what == "first row":
        b[:, 0] = b[:, 1]
    elif what == "first column":
        b[:, :, 0] = b[:, :, 1]
    else:
        b[:, -1, -1] = b[:, -2, -2]
    return b


@pytest.mark.parametrize("model", ["lite", "mlkit", "deeplab-synthetic", "lite-16x16", "lite-104x168", "deeplab-65x97"])
def test_a_border_row_column_or_corner_taken_from_its_neighbour_fails(model):
    """Edges: what a kernel gets wrong at a SAME-padding edge or a tile edge.  On a noise network input (uniform f32 over the normalised range), in the stem's
    output, in the first stride-2 depthwise output, in the largest tensor of the decoder and in the network output: the last and first row, the last and first
    column, then one corner pixel replaced by the inward neighbour.  In the stem's and the stride-2 depthwise's output all five must fail, unconditionally.  In the
    other two a replacement that moves the tensor by less than its bar cannot fail and is reported (MLKit's output on noise is a saturated sigmoid)."""
    path, x, ot, exact, m, dev = _case(model, "noise tensor")
    base = G.audit(path, x, dev, ot, exact, m)
    assert not G.failing(base)
    rows0, checked = {r["t"]: r for r in base}, {}
    spatial = [op for op in m.ops if op.outputs[0] in dev and dev[op.outputs[0]].ndim == 4 and min(dev[op.outputs[0]].shape[1:3]) >= 4]
    stem = spatial[0].outputs[0]
    dw2 = next(op.outputs[0] for op in spatial if op.name == "DEPTHWISE_CONV_2D" and op.opts["stride_h"] == 2)
    big = max((op.outputs[0] for op in spatial[len(spatial) // 2:-1]), key=lambda t: dev[t].size)
    out = m.outputs[0]
    for t in (stem, dw2, big, out):
        for what in EDGE_FAULTS:
            b = _edge_fault(dev[t], what)
            change = float(np.abs(b.astype(np.float64) - dev[t]).max())
            if t not in (stem, dw2) and not change > rows0[t]["bar"] + rows0[t]["local"]:
                print("%-18s t%-3d %-18s %-13s: moves the tensor by %.3g, below its bar" % (model, t, "x".join(map(str, dev[t].shape)), what, change))
                continue
            mut = dict(dev)
            mut[t] = b
            fails = G.failing(G.audit(path, x, mut, ot, exact, m))
            print("%-18s t%-3d %-18s %-13s: failed at %s" % (model, t, "x".join(map(str, dev[t].shape)), what, fails))
            assert t in fails, "%s of t%d replaced by its neighbour passes" % (what, t)
            checked.setdefault(what, []).append(t)
    for what in EDGE_FAULTS:
        assert {stem, dw2} <= set(checked.get(what, [])), "%s: asserted on %s only" % (what, checked.get(what, []))
    if model != "lite-16x16":
        return
    # The 16x16 graph shrinks to 1x1 in its middle: every tensor that still has two rows and two columns takes the five faults.  One that moves the tensor by more
    # than its bar plus its own local error must fail there (the triangle inequality); a tensor counts as caught when all five did.
    caught, small = [], []
    for op in m.ops:
        t = op.outputs[0]
        if t not in dev or dev[t].ndim != 4:
            continue
        if min(dev[t].shape[1:3]) < 2:
            small.append(t)
            continue
        n = 0
        for what in EDGE_FAULTS:
            b = _edge_fault(dev[t], what)
            if not float(np.abs(b.astype(np.float64) - dev[t]).max()) > rows0[t]["bar"] + rows0[t]["local"]:
                continue
            mut = dict(dev)
            mut[t] = b
            assert t in G.failing(G.audit(path, x, mut, ot, exact, m)), "%s of t%d (%s) replaced by its neighbour passes" % (what, t, "x".join(map(str, dev[t].shape)))
            n += 1
        if n == len(EDGE_FAULTS):
            caught.append(t)
    print("%s: all five faults caught in %d tensors %s; %d tensors of fewer than two rows or columns skipped" % (model, len(caught), caught, len(small)))
    assert len(caught) >= 10 and small


# ------------------------------------------------------------------------------------------------------------------------------
# The bars of the reduced-precision audit (f64_graph: audit_reduced), proven the same way
# ------------------------------------------------------------------------------------------------------------------------------
# Stand-in devices, all from f64_graph's operators on PyTorch's f32 CPU kernels:
#   half storage   the cut tensors other than the network output are rounded to half; downstream operators consume the rounded values
#   f16 operands   the operators operand_rounding_rule names run on x.half().float() and w.half().float()
#   both
RULE_STREAMS = 9          # the batch at which every 1x1 convolution of DeepLab's 33x33 levels has its 8192 rows: the widest rule


def _cuts(m, dev):
    every = sorted(dev)
    return (("every tensor", every), ("every 12th + output", sorted(set(every[::12] + [m.outputs[0]]))))


@functools.lru_cache(maxsize=None)
def _rule(model):
    import backscrub_amd
    from backscrub_amd import tflite_io
    return G.operand_rounding_rule(backscrub_amd.model_describe(_path(model)), tflite_io.load(_path(model)), "fast", RULE_STREAMS)


def _stand_in(m, x, cut, half_storage, rounding, fault=None):
    """tensor index → f32 array over `cut` of the stand-in device.  fault: (tensor, callable f32 tensor → stored f32 tensor) replaces the storing of one cut tensor;
    (tensor, "slab") drops input channels 32..63 from that convolution."""
    val = G._constants(m, torch.float32)
    val[m.inputs[0]] = torch.from_numpy(np.asarray(x, dtype=np.float32))
    cut, dev, out = set(cut), {}, m.outputs[0]
    for op in m.ops:
        o = op.outputs[0]
        r = (rounding or {}).get(o)
        if fault and fault[0] == o and fault[1] == "slab":
            assert op.name == "CONV_2D" and r
            v2 = dict(val)
            xz = val[op.inputs[0]].clone()
            xz[..., 32:64] = 0
            v2[op.inputs[0]] = xz
            v = G._eval(op, v2, torch.float32, w16=r, x16=True)
        else:
            v = G._eval(op, val, torch.float32, w16=r, x16=bool(r))
        if o in cut and op.name != "DEQUANTIZE":
            if fault and fault[0] == o and callable(fault[1]):
                v = fault[1](v)
            elif half_storage and o != out:
                v = v.half().float()
            dev[o] = v.numpy().copy()
        val[o] = v
    return dev


STAND_INS = [(model, "half storage") for model in SHIPPED] +[("deeplab-synthetic", "f16 operands"), ("deeplab-synthetic", "both")]


@pytest.mark.parametrize("model,kind", STAND_INS, ids=["%s-%s" % (a, b.replace(" ", "_")) for a, b in STAND_INS])
def test_the_reduced_precision_stand_ins_pass_at_half_the_bar(model, kind):
    """Fairness of (a) and (b): with B32 HALVED (the "<= 4 of 8" of the f32 proof) no element of any stand-in is outside its interval, on the five inputs and both
    cut sets; nothing overflows a half."""
    if not os.path.exists(_path(model)):
        pytest.fail("model fixture %s is missing" % _path(model))
    half_storage, rounding = kind != "f16 operands", (_rule(model) if kind != "half storage" else {})
    if kind != "half storage":
        assert len(rounding) >= 30 and any(isinstance(s, tuple) for s in rounding.values()), "the rule names %d operators" % len(rounding)
    for inp in INPUTS:
        path, x, ot, exact, m, dev0 = _case(model, inp)
        for cutname, cut in _cuts(m, dev0):
            dev = _stand_in(m, x, cut, half_storage, rounding)
            half = set(cut) - {m.outputs[0]} if half_storage else set()
            rows = G.audit_reduced(path, x, dev, ot, half, rounding, exact, m, bar_scale=0.5)
            outside = sum(r["outside"] for r in rows)
            print("%-18s %-13s %-9s %-20s %3d tensors (%3d as halves), %d elements outside, largest allowance %.3g, largest magnitude %.4g" % (
                model, kind, inp, cutname, len(rows), len(half), outside, max(r["allow"] for r in rows), max(r["scale"] for r in rows)))
            assert len(rows) == len(cut) and all(r["finite"] for r in rows)
            assert not G.failing_reduced(rows), "%s / %s / %s / %s\n%s" % (model, kind, inp, cutname, G.format_table_reduced(rows))


def _trunc16(v):
    h = v.half()
    bits = torch.where(h.float().abs() > v.abs(), h.view(torch.int16) - 1, h.view(torch.int16))      # one half ulp toward zero where nearest-even went away from it
    return bits.view(torch.float16).float()


def _largest_channel(v):
    return int(v.abs().reshape(-1, v.shape[-1]).max(0).values.argmax())


def _scaled(v):
    b = v.clone()
    b[..., _largest_channel(v)] *= 1 + 2.0 ** -9
    return b.half().float()


def _swapped(v):
    b = v.half().float().clone()
    px = b[:, -1, -1]
    c = int((px[0, 1:] - px[0, :-1]).abs().argmax())             # the adjacent pair of the last pixel that differs most
    b[:, -1, -1, [c, c + 1]] = b[:, -1, -1, [c + 1, c]]
    return b


def _last_column(v):
    b = v.half().float().clone()
    b[:, :, -1] = b[:, :, -2]
    return b


FAULTS = {"truncation toward zero": _trunc16, "one channel scaled by 1 + 2^-9": _scaled, "two adjacent channels swapped at the last pixel": _swapped,
          "last column from its inward neighbour": _last_column}


@pytest.mark.parametrize("fault", list(FAULTS), ids=[re_id.replace(" ", "_").replace("^", "") for re_id in FAULTS])
def test_a_storage_fault_in_one_cut_tensor_fails_there_and_nowhere_else(fault):
    """Sharpness of (a), at the FULL bar: each storage fault, injected into one tensor of the sparse cut of lite on the noise network input, puts elements of that
    tensor outside their interval and of no other tensor."""
    path, x, ot, exact, m, dev0 = _case("lite", "noise tensor")
    cut = _cuts(m, dev0)[1][1]
    half = set(cut) - {m.outputs[0]}
    clean = G.audit_reduced(path, x, _stand_in(m, x, cut, True, {}), ot, half, {}, exact, m)
    assert not G.failing_reduced(clean)
    spatial = [t for t in cut if t in half and dev0[t].ndim == 4 and min(dev0[t].shape[1:3]) >= 4][:4]
    assert len(spatial) == 4
    for t in spatial:
        rows = G.audit_reduced(path, x, _stand_in(m, x, cut, True, {}, fault=(t, FAULTS[fault])), ot, half, {}, exact, m)
        got = {r["t"]: r["outside"] for r in rows if r["outside"]}
        print("lite t%-3d %-20s %-48s elements outside: %s" % (t, "x".join(map(str, dev0[t].shape)), fault, got))
        assert set(got) == {t}, "%s in t%d: tensors with elements outside their interval: %s" % (fault, t, got)


def test_a_dropped_k_slab_of_one_1x1_convolution_fails_there_and_nowhere_else():
    """Sharpness of (b): the f16-operand stand-in of DeepLab with input channels 32..63 missing from ONE 1x1 convolution (one K slab of the GEMM) fails at that
    convolution's output and at no other tensor — the allowance, 2^-11 of the absolute products, is far below one slab's contribution."""
    model = "deeplab-synthetic"
    path, x, ot, exact, m, dev0 = _case(model, "noise")
    rounding = _rule(model)
    cut = _cuts(m, dev0)[0][1]
    prod = G.producers(m)
    t = next(o for o in sorted(rounding) if rounding[o] is True and prod[o].opts["act"] == 0 and int(m.tensors[prod[o].inputs[1]].shape[3]) >= 96)
    clean = G.audit_reduced(path, x, _stand_in(m, x, cut, False, rounding), ot, set(), rounding, exact, m)
    assert not G.failing_reduced(clean)
    rows = G.audit_reduced(path, x, _stand_in(m, x, cut, False, rounding, fault=(t, "slab")), ot, set(), rounding, exact, m)
    got = {r["t"]: r["outside"] for r in rows if r["outside"]}
    print("%s t%d (%s): elements outside: %s" % (model, t, "x".join(map(str, dev0[t].shape)), got))
    assert set(got) == {t}
