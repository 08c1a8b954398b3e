"""k3's per-frame form on the GPU: against the tile form and the gate launch (BSX_K3_TILES=1, debug library), bit for bit.

bsx_seg_k3f does seg_k3_k's and seg_gate_k's arithmetic with the same operands in the same order — one 1024-lane workgroup per frame instead of six tiles and a launch —
so everything the two launches write (lo, the pooled partial sums of lo, the tail's gate vector, read back through the entry the layer audit uses) and everything
downstream (the filtered network output `ofinal`, the masks, the composites) must be the same bytes, over three steps from a random state of the temporal filter."""
import re

import numpy as np
import pytest

from conftest import model_path

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

VGA, HD = (640, 480), (1280, 720)
STEPS = 3

# (model, frame size, streams, environment of both contexts, the form the unforced context must report)
CASES = [
    ("lite", VGA, 1, {}, "frame"),                          # a single workgroup
    ("lite", VGA, 3, {}, "frame"),                          # frames at different blockIdx
    ("lite", VGA, 2, {"BSX_ACT16": "1"}, "frame"),          # the H16 loads and as_stored's rounding
    ("lite", VGA, 2, {"BSX_NO_RTC": "1"}, "tiles"),         # the ahead-of-time path: the form is part of the specialised module only, and the plan says so
    ("full", HD, 2, {}, "tiles"),                           # a frame that does not fit: the planner's rule did not leak
]


def _id(c):
    key, res, n, both, form = c
    return "%s-%dx%d-n%d-%s%s" % (key, res[0], res[1], n, form, "".join("-" + k[4:].lower() for k in both))


def _run(bs, monkeypatch, key, res, n, env):
    from backscrub_amd import synth
    W, H = res
    for k in ("BSX_K3_TILES", "BSX_ACT16", "BSX_NO_RTC"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    mg = bs.MaskGen(model_path(key), W, H, n_streams=n)
    try:
        plan = mg.plan()
        k3 = re.search(r"^segment k3 .*tiles per frame.* stores t(\d+)(?::f16)?$", plan, re.M)
        plo = re.search(r"^segment partial sums .* lo t(\d+)$", plan, re.M)
        frame = re.search(r"^segment k3 form: per-frame, .*finishes gate\(tail\) t(\d+)$", plan, re.M)
        tiles = re.search(r"^segment k3 form: tiles, then a launch for gate\(tail\) t(\d+) ", plan, re.M)
        assert k3 and plo and (frame or tiles) and not (frame and tiles), plan
        form = "frame" if frame and "segment k3 execution: tiles and the gate launch" not in plan else "tiles"
        tlo, tplo, tgate = int(k3.group(1)), int(plo.group(1)), int((frame or tiles).group(1))
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
            for name, tid in (("lo", tlo), ("partial sums of lo", tplo), ("gate(tail)", tgate)):
                rec[name] = np.stack([mg.graph_tensor(tid, s) for s in range(n)])
            got.append(rec)
        return form, got
    finally:
        mg.close()


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_the_per_frame_form_is_bit_identical_to_the_tiles_and_the_gate_launch(case, monkeypatch, debug_switches):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    bs = debug_switches
    key, res, n, both, want = case
    form0, ref = _run(bs, monkeypatch, key, res, n, dict(both, BSX_K3_TILES="1"))
    form, got = _run(bs, monkeypatch, key, res, n, dict(both))
    assert form0 == "tiles" and form == want, (form0, form)
    for t in range(STEPS):
        for name in ref[t]:
            a, b = ref[t][name], got[t][name]
            assert a.shape == b.shape and a.dtype == b.dtype
            assert np.isfinite(a.astype(np.float64)).all(), "step %d: %s of the reference run is not finite" % (t, name)
            same = a.view(np.uint8).reshape(-1) == b.view(np.uint8).reshape(-1)
            assert same.all(), "step %d: %s differs from the tile form in %d of %d bytes" % (t, name, int((~same).sum()), same.size)
    # the comparison is not vacuous: k3's outputs are not constant and the filter state moved
    assert np.ptp(ref[-1]["lo"]) > 0 and np.ptp(ref[-1]["gate(tail)"]) > 0 and not np.array_equal(ref[0]["ofinal"], ref[-1]["ofinal"])
