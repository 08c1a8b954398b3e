"""k2's staged weights on the GPU: every staged form against form 0 (BSX_K2_GLOBAL_W=1, debug library), bit for bit.

The staged forms move where seg_k2_k reads its 1x1 / depthwise weights from (LDS instead of global memory), not what enters its instructions, so everything k2 writes —
B, c0 and the pooled partial sums of B, read back through the entry the layer audit uses — and everything downstream of it (the filtered network output `ofinal`, the
masks, the composites) must be the same bytes, over three steps from a random state of the temporal filter."""
import re

import numpy as np
import pytest

from conftest import model_path

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

VGA, HD = (640, 480), (1280, 720)
STEPS = 3
FORM1_CAP = "25000"          # BSX_K2_LDS_CAP: an LDS budget that holds one workgroup with form 1's block and none with form 2's, so the planner takes form 1

# (model, frame size, streams, environment of both contexts, environment of the staged one, the form it must report)
CASES = [
    ("lite", VGA, 1, {}, {}, 2),                       # C = 72: the last channel group is ragged
    ("lite", VGA, 9, {}, {}, 2),                       # n % 8 != 0: the order xcd_frame_tile gives the workgroups
    ("full", HD, 2, {}, {}, 2),
    ("mlkit", HD, 2, {}, {}, 2),
    ("lite", VGA, 2, {"BSX_ACT16": "1"}, {}, 2),       # 16-bit storage of B and c0
    ("lite", VGA, 9, {}, {"BSX_K2_LDS_CAP": FORM1_CAP}, 1),      # the 1x1 tiles alone
    ("lite", VGA, 2, {"BSX_NO_RTC": "1"}, {}, 2),      # the ahead-of-time instance: it leaves the planned block unused (global weights whatever the form) and must not mind it
]


def _id(c):
    key, res, n, both, staged, form = c
    return "%s-%dx%d-n%d-form%d%s" % (key, res[0], res[1], n, form, "".join("-" + k[4:].lower() for k in both))


def _run(bs, monkeypatch, key, res, n, env):
    from backscrub_amd import synth
    W, H = res
    for k in ("BSX_K2_GLOBAL_W", "BSX_K2_LDS_CAP", "BSX_ACT16", "BSX_NO_RTC"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    mg = bs.MaskGen(model_path(key), W, H, n_streams=n)
    try:
        plan = mg.plan()
        k2 = re.search(r"^segment k2 .*\(weights staged: form (\d), (\d+) B\), stores t(\d+)(?::f16)? t(\d+)(?::f16)?$", plan, re.M)
        pB = re.search(r"^segment partial sums .* B t(\d+),", plan, re.M)
        assert k2 and pB, plan
        form, tB, tc0, tpB = int(k2.group(1)), int(k2.group(3)), int(k2.group(4)), int(pB.group(1))
        i = mg.info
        mg.ofinal().copy_(torch.from_numpy(synth.random_u8((n, i["out_h"], i["out_w"]), 41)).cuda())      # a random state of the temporal filter
        bg = torch.from_numpy(synth.background(W, H)).cuda()
        out = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
        got = []
        for t in range(STEPS):
            frames = torch.from_numpy(np.stack([synth.frame(W, H, s, t) for s in range(n)])).cuda()
            mg.step(frames, bg, out)
            torch.cuda.synchronize()
            rec = {"composite": out.cpu().numpy().copy(), "masks": mg.masks().cpu().numpy().copy(), "ofinal": mg.ofinal().cpu().numpy().copy()}
            for name, tid in (("B", tB), ("c0", tc0), ("partial sums of B", tpB)):
                rec[name] = np.stack([mg.graph_tensor(tid, s) for s in range(n)])
            got.append(rec)
        return form, got
    finally:
        mg.close()


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_staged_weights_are_bit_identical_to_global_weights(case, monkeypatch, debug_switches):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    bs = debug_switches
    key, res, n, both, staged, want_form = case
    form0, ref = _run(bs, monkeypatch, key, res, n, dict(both, BSX_K2_GLOBAL_W="1"))
    form, got = _run(bs, monkeypatch, key, res, n, dict(both, **staged))
    assert form0 == 0 and form == want_form, (form0, form)
    for t in range(STEPS):
        for name in ref[t]:
            a, b = ref[t][name], got[t][name]
            assert a.shape == b.shape and a.dtype == b.dtype
            assert np.isfinite(a.astype(np.float64)).all(), "step %d: %s of the reference run is not finite" % (t, name)
            same = a.view(np.uint8).reshape(-1) == b.view(np.uint8).reshape(-1)
            assert same.all(), "step %d: %s differs from form 0 in %d of %d bytes" % (t, name, int((~same).sum()), same.size)
    # the comparison is not vacuous: k2's outputs are not constant and the filter state moved
    assert np.ptp(ref[-1]["B"]) > 0 and np.ptp(ref[-1]["c0"]) > 0 and not np.array_equal(ref[0]["ofinal"], ref[-1]["ofinal"])
