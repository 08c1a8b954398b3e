"""The Meet-family and MLKit network kernels at other model input sizes than the three shipped ones (tests/model_size_cases.py; docs/design/02a-layer-audit.md,
"Other model sizes").

(a) every tensor every execution path stores, against the float64 evaluation of its own operator group — the audit of tests/test_gpu_layers.py, unchanged, on twelve
    graphs whose geometry the shipped shapes never produce: 1x1 tile grids and tiles smaller than their targets, partial last tiles, an asymmetric stem pad, odd extents
    through the middle program, a 5x5 depthwise larger than its input, k3's tile form on a lite graph, Meet-family graphs that are not segmented, and the SAME-cropped
    transpose convolution;
(b) the four stages and one step per case at two frame sizes, against the oracle: here a 16x16 or 8x8 network output meets the mask up-scaler (40:1, 80:1; the
    shipped models stay below 7:1) and a 97x161 output its linear tables;
(c) the graph-specialised segment kernels against the ahead-of-time ones, bit for bit, at two of the new geometries;
(d) the DeepLab graph — the per-launch path of kernels_nn.hip — at twelve other input sizes and once at twice the channel width (tests/deeplab_size_cases.py; "Other model
    sizes: DeepLab"): (a) on every row of its paths, after the plan of the context has stated the facts of the case's row, and (b), where a 1/8 map that is no 2^k + 1
    meets the fused align-corners resize + argmax at a scale that is no power of two."""
import re

import numpy as np
import pytest

import deeplab_size_cases as D
from geometry_cases import mask_of_state
from model_size_cases import BY_NAME, CASES, FORCED, FORCED_KNOBS, model_file
from test_gpu_layers import KNOBS, NO_FUSION, _paths, audit_every_stored_tensor
from test_gpu_parity import _dev, bs  # noqa: F401 (bs: the library fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("sized_models")
    return {**{c.name: model_file(c, d) for c in CASES}, **{c.name: D.model_file(c, d) for c in D.CASES}}


def _slug(s):
    return re.sub(r"[^a-z0-9]+", "_", s.lower()).strip("_")[:40]


W_AUDIT, H_AUDIT = 640, 480


def _refused(bs, path, case, W, H, n):
    from backscrub_amd import api
    with pytest.raises(api.BsxError) as e:
        bs.MaskGen(path, W, H, n_streams=n).close()
    assert case.refused in str(e.value), str(e.value)


# ---- (a) ------------------------------------------------------------------------------------------------------------------------
AUDIT = [(c.name, pname, env) for c in CASES for pname, env in _paths(c.family)] + \
        [(name, "segments + specialised middle kernel (hipRTC), " + what, dict(env)) for name, what, env in FORCED]


@pytest.mark.parametrize("name,pname,env", AUDIT, ids=["%s-%s" % (n, _slug(p)) for n, p, _ in AUDIT])
def test_every_stored_tensor_against_float64(name, pname, env, models, oracle, monkeypatch, debug_switches):
    case = BY_NAME[name]
    if case.refused:                                           # no context of this model exists at any frame size: the refusal is the result (and a context is a finding)
        _refused(debug_switches, models[name], case, W_AUDIT, H_AUDIT, 8)
        return

    def about_plan(plan):
        segmented = re.search(r"^segment ", plan, re.M) is not None
        wants = case.segmented and "BSX_NO_SEGMENTS" not in env and "BSX_NO_FRAME_PROGRAM" not in env
        # a case the planner does not segment runs whatever it gives on the "segments" rows — but never a half-segmented plan
        assert segmented == wants, "%s on %r: %s\n%s" % (name, pname, "no segment line" if wants else "segment lines in a plan that should have none", plan)
        if "BSX_K3_TILES" in env:
            assert "segment k3 form: tiles, then a launch for gate(tail)" in plan and "switched off" in plan, plan
        if "BSX_SEG_TILES" in env:
            assert "segment head  tile 2x4, 4x3 tiles per frame" in plan and "segment tail  tile 4x5, 4x5 tiles per frame" in plan, plan

    audit_every_stored_tensor(debug_switches, oracle, monkeypatch, models[name], case.family, pname, env, model=name, knobs=KNOBS + FORCED_KNOBS, about_plan=about_plan)


# ---- (b) ------------------------------------------------------------------------------------------------------------------------
SIZES = [(640, 480), (322, 242)]


@pytest.mark.parametrize("res", SIZES, ids=["%dx%d" % r for r in SIZES])
@pytest.mark.parametrize("name", [c.name for c in CASES] + [c.name for c in D.CASES])
def test_stages_and_one_step_match_the_oracle(bs, oracle, models, name, res):
    """test_stages_match_oracle's body (prep byte-equal, logits within 1e-4 relative, decode + IIR from a random state byte-equal on the oracle's logits, mask
    byte-equal), then one step from that state whose mask and composite are the oracle's up-scale, blur and blend of the temporal state the device itself holds
    (the method of docs/design/02b-geometry-audit.md)."""
    from backscrub_amd import synth
    path = models[name]
    W, H = res
    n = 3
    if name in BY_NAME and BY_NAME[name].refused:
        _refused(bs, path, BY_NAME[name], W, H, n)
        return
    mg = bs.MaskGen(path, W, H, n_streams=n)
    oc = [oracle.Ctx(path, W, H) for _ in range(n)]
    try:
        info = mg.info
        assert tuple(info["roi"]) == oc[0].roidim and tuple(info["in_roi"]) == oc[0].in_roidim
        frames = np.stack([synth.frame(W, H, s) for s in range(n)])
        frames[2] = synth.random_u8((H, W, 3), 7)
        d_frames = _dev(frames)
        mg.run_stage(0, d_frames)
        got_in = mg.input_tensor().cpu().numpy()
        for i in range(n):
            want = oc[i].prep(frames[i])
            assert np.array_equal(got_in[i], want), "prep mismatch stream %d: %d px differ, max %g" % (i, (got_in[i] != want).sum(), np.abs(got_in[i] - want).max())
        mg.run_stage(1, n=n)
        got_out = mg.output_tensor().cpu().numpy()
        for i in range(n):
            want = oc[i].infer()
            assert got_out[i].size == want.size
            err = float(np.abs(got_out[i].reshape(want.shape) - want).max()) / max(1.0, float(np.abs(want).max()))
            print("%s %dx%d stream %d: logits rel err %.3g" % (name, W, H, i, err))
            assert err < 1e-4, "logits rel err %g (stream %d)" % (err, i)
        prev = synth.random_u8((n, info["out_h"], info["out_w"]), 11)
        mg.output_tensor().copy_(_dev(np.stack([c.output() for c in oc]).reshape(got_out.shape)))
        mg.ofinal().copy_(_dev(prev))
        mg.run_stage(2, n=n)
        got_of = mg.ofinal().cpu().numpy()
        for i in range(n):
            oc[i].set_ofinal(prev[i])
            oc[i].post()
            assert np.array_equal(got_of[i], oc[i].ofinal()), "decode mismatch stream %d" % i
        mg.run_stage(3, n=n)
        got_m = mg.masks().cpu().numpy()
        for i in range(n):
            assert np.array_equal(got_m[i], oc[i].mask()), "mask mismatch stream %d: %d px" % (i, (got_m[i] != oc[i].mask()).sum())
        # one step: the temporal state it leaves is the device's own; the mask and the composite must be what that state implies
        bg = synth.background(W, H)
        out = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
        frames2 = np.stack([synth.frame(W, H, s, 1) for s in range(n)])
        frames2[2] = synth.random_u8((H, W, 3), 8)
        mg.step(_dev(frames2), _dev(bg), out)
        torch.cuda.synchronize()
        state, masks, comp = mg.ofinal().cpu().numpy(), mg.masks().cpu().numpy(), out.cpu().numpy()
        assert not np.array_equal(state, got_of), "the step left the temporal state where it was"
        for i in range(n):
            want_m = mask_of_state(oracle, state[i], info, W, H)
            assert np.array_equal(masks[i], want_m), "step: mask of stream %d differs from its own state's in %d px" % (i, (masks[i] != want_m).sum())
            assert np.array_equal(comp[i], oracle.alpha_blend(bg, frames2[i], want_m)), "step: composite of stream %d" % i
    finally:
        for c in oc:
            c.close()
        mg.close()


# ---- (d) ------------------------------------------------------------------------------------------------------------------------
def _deeplab_rows(c):
    """The rows of _paths("deeplab") the case runs.  Without the rewrites every DeepLab step list has a micro-op form, and bsx_new runs it as a frame program where most
    of its tensors fit the LDS (the 9x9, 17x17, 33x33 and 65x97 graphs): "no graph rewrites" audits whichever of the two bsx_new chooses, and "nothing fused" switches
    the program off, as it does on the Meet graphs.  9x9 has a micro-op form WITH the rewrites too and runs it on every row: one more row runs the per-launch
    kernels on its rewritten step list."""
    rows = [(pname, dict(env, BSX_NO_FRAME_PROGRAM="1") if pname == NO_FUSION else env) for i, (pname, env) in enumerate(_paths(D.FAMILY)) if c.rows is None or i in c.rows]
    return rows + ([("one launch per step", {"BSX_NO_FRAME_PROGRAM": "1"})] if c.micro_ops else [])


DEEPLAB_AUDIT = [(c.name, pname, env) for c in D.CASES for pname, env in _deeplab_rows(c)]


@pytest.mark.parametrize("name,pname,env", DEEPLAB_AUDIT, ids=["%s-%s" % (n, _slug(p)) for n, p, _ in DEEPLAB_AUDIT])
def test_every_stored_tensor_of_a_sized_deeplab_against_float64(name, pname, env, models, oracle, monkeypatch, debug_switches):
    case = D.BY_NAME[name]

    def about_plan(plan):
        """the context's own plan still has the geometry the case is in the table for — on the rows that leave the fusions on"""
        got = D.plan_facts(plan)
        fp = re.search(r"^frame program: (ON|off), (\d+) micro-ops, .* (\d+) tensors in LDS, (\d+) in HBM$", plan, re.M)
        assert fp, "no 'frame program:' line of the expected form in the plan\n" + plan
        program, micro_ops = fp.group(1) == "ON", int(fp.group(2))
        # bsx_new's rule: a plan that has a program runs it when at least as many of its tensors are in LDS as in HBM
        assert program == (micro_ops > 0 and int(fp.group(3)) >= int(fp.group(4)) and "BSX_NO_FRAME_PROGRAM" not in env), fp.group(0)
        if "BSX_NO_REWRITES" not in env:
            assert micro_ops == case.micro_ops, "%s on %r: %s\n%s" % (name, pname, fp.group(0), plan)
        if micro_ops:                                                                 # (a plan that has a program, used or not, fuses nothing: plan.cpp)
            assert not got["head_fused"] and not got["pairs"] and not got["chain"], plan
            return
        assert got["chain"] == case.chain, plan
        if "BSX_NO_IR_FUSE" not in env:                                               # (it switches the fused head off as well)
            assert got["pairs"] == D.pairs_of(case) and got["unfused"] == case.unfused, (got, plan)
            if "BSX_NO_HEAD0" not in env:
                assert got["head_fused"] == case.head_fused, plan

    audit_every_stored_tensor(debug_switches, oracle, monkeypatch, models[name], D.FAMILY, pname, env, model=name, about_plan=about_plan,
                              n_streams=case.streams, n_stepped=case.stepped)


# ---- (c) ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lite-32x48", "lite-104x168"])
def test_specialised_segment_kernels_equal_the_ahead_of_time_ones(bs, models, name, monkeypatch, debug_switches):
    """All four segment kernels (and k3's per-frame form at 32x48, its tile form at 104x168) as hipRTC compiled them for the graph, against the ahead-of-time kernels
    with the descriptor as an argument (BSX_NO_SEG_RTC=1, debug library): the body of tests/test_gpu_parity.py's test of that name — temporal state, masks and
    composites identical bit for bit over three steps.  Then nothing specialised at all (BSX_NO_RTC=1: the interpreted middle program too): the logits are those of
    the same frames within the 1e-4 of every execution path."""
    from backscrub_amd import synth
    W, H, n = 640, 480, 3
    path = models[name]
    bg = _dev(synth.background(W, H))
    got, logits = [], []
    for env in ({}, {"BSX_NO_SEG_RTC": "1"}, {"BSX_NO_RTC": "1"}):
        for k in ("BSX_NO_SEG_RTC", "BSX_NO_RTC"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        mg = debug_switches.MaskGen(path, W, H, n_streams=n)
        try:
            plan = mg.plan()
            assert ("segment execution: specialised kernels (hipRTC" in plan) == (not env), plan[-400:]
            frames = np.stack([synth.frame(W, H, i, 3) for i in range(n)])
            mg.run_stage(0, _dev(frames))
            mg.run_stage(1, n=n)
            logits.append(mg.output_tensor().cpu().numpy().copy())
            out = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
            snaps = []
            for t in range(3):
                frames = np.stack([synth.frame(W, H, i, t) for i in range(n)])
                frames[n - 1] = synth.random_u8((H, W, 3), 50 + t)
                mg.step(_dev(frames), bg, out)
                snaps.append((mg.ofinal().clone(), mg.masks().clone(), out.clone()))
            got.append(snaps)
        finally:
            mg.close()
    for k in ("BSX_NO_SEG_RTC", "BSX_NO_RTC"):
        monkeypatch.delenv(k, raising=False)
    for t in range(3):
        for a, b in zip(got[0][t], got[1][t]):
            assert torch.equal(a, b), "step %d" % t
    assert not torch.equal(got[0][0][0], got[0][2][0])                                  # the state moved: the comparison is not of three equal frames
    assert np.isfinite(logits[0]).all() and np.ptp(logits[0]) > 0 and np.array_equal(logits[0], logits[1])
    err = float(np.abs(logits[2] - logits[0]).max()) / max(1.0, float(np.abs(logits[0]).max()))
    assert err < 1e-4, "nothing specialised: logits rel err %g against the specialised kernels" % err
