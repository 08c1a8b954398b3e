"""The three reduced-precision network modes, tensor by tensor: every tensor they store, against a float64 evaluation of its own operator group.

tests/test_gpu_layers.py audits the f32 network; the modes below were checked at the last tensor only, through gates (logits within 1e-2 .. 2e-2, decisions
agreeing to 99.5 %) that a packed-half quad at the wrong index of one tile column, two channels swapped inside a quad, truncation instead of round-to-nearest-even or
a producer and a consumer that disagree on which layers are stored as halves all pass.

  BSX_ACT16=1            16-bit STORAGE of the segmented networks (segment kernels' ldg4 / stg4<H16>, the generated middle kernel's SP_GLB16 forms), f32 arithmetic
  BSX_F16_GEMM=fast      f16 MFMA OPERANDS (pw_gemm_f16s_k<1, N>, ir_expand_dw_k<1, ..>), f32 accumulation and storage
  BSX_F16_GEMM=fast16    both: the fused expand + depthwise kernels store halves (OUT16) that the project GEMM reads (IN16), from 8192 rows

Same harness as the f32 audit (libbsx_dbg.so, BSX_ARENA_NO_REUSE=1, BSX_ARENA_POISON=1 — NaN bytes are NaN as halves too —, 640x480 frames, per-stream read-back) and
the same assertions, with the bars of tests/f64_graph.py (audit_reduced) that tests/test_f64_forced_host.py proves fair and sharp; nothing in them is measured on the
kernels.  Besides: the set of half-stored tensors is what the plan text marks f16, and every tensor it marks f32 holds a value no half can represent.

The segmented paths also store two tensors the file does not have — the 1x1 convolutions that a rewrite moved below their resize — and BSX_ACT16 rounds them to half:
they are read back and audited as well (f64_graph.moved_convs), against the convolution of the resize's input; without them their rounding shows up as an error of the
gate and of the network output that nothing explains.

The f16-operand modes also run on three DeepLab graphs of other sizes (tests/deeplab_size_cases.py): 129x129 at 8 streams (8712 rows at its 1/4 level, 2312 at
its 1/8 level: operand_rounding_rule has to name the fused expands and the GEMMs of one level only), 353x481 at 4 (every level of 8192 rows and more, the stem
unfused: its K = 16 GEMM too) and the wide graph at 10 (the expands from Cin = 160 run as plain GEMMs, the chain does not exist).

The accumulated error at the network output is printed and recorded, not asserted: these modes are not parity-grade; their gates (tests/test_gpu_parity.py) stay in force."""
import json
import os
import re
import time

import numpy as np
import pytest

import deeplab_size_cases as D
from conftest import reference_model_path, synthetic_model_path
from test_gpu_layers import H, KNOBS, W, half_by_plan, stored_by_plan

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import f64_graph as G  # noqa: E402

SEGMENTED = [("lite", True), ("full", True), ("mlkit", True), ("lite", False), ("full", False), ("mlkit", False)]
# (architecture, real weights, environment, streams of the context, streams stepped)
CASES = ([(a, r, {"BSX_ACT16": "1"}, 8, 5) for a, r in SEGMENTED] + [(a, r, {"BSX_ACT16": "1", "BSX_F32_INPUT": "1"}, 8, 5) for a, r in SEGMENTED] +
         [("deeplab", False, {"BSX_F16_GEMM": mode}, ns, n) for mode in ("fast", "fast16") for ns, n in ((8, 5), (9, 9))] +
         [(name, False, {"BSX_F16_GEMM": mode}, ns, n) for name, ns, n in (("deeplab-129x129", 8, 8), ("deeplab-353x481", 8, 4), ("deeplab-wide-193x257", 10, 10))
          for mode in ("fast", "fast16")])


def _mode_id(c):
    _, _, env, ns, n = c
    return "%s-%dof%d" % ("-".join(re.sub(r"^bsx_", "", k.lower()) + ("" if v == "1" else "_" + v) for k, v in sorted(env.items())), n, ns)


def _case_id(c):
    return "%s-%s-%s" % (c[0], "real" if c[1] else "synthetic", _mode_id(c))


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_every_stored_tensor_of_a_reduced_precision_mode_against_float64(case, oracle, monkeypatch, debug_switches, tmp_path):
    from backscrub_amd import tflite_io
    bs = debug_switches
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    t_start = time.time()
    arch, real, env, n_streams, n_stepped = case
    if arch in D.BY_NAME:
        path = D.model_file(D.BY_NAME[arch], tmp_path)
    else:
        path = reference_model_path(arch) if real else synthetic_model_path(arch)
    if real and not os.path.exists(path):
        pytest.fail("model fixture %s is missing" % path)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("BSX_ARENA_NO_REUSE", "1")
    monkeypatch.setenv("BSX_ARENA_POISON", "1")
    mode = env.get("BSX_F16_GEMM", "act16")
    f32_input = "BSX_F32_INPUT" in env
    m = tflite_io.load(path)
    nt, t_in, t_out = len(m.tensors), m.inputs[0], m.outputs[0]
    mg = bs.MaskGen(path, W, H, n_streams=n_streams)
    oc = None
    try:
        plan = mg.plan()
        assert "slot of its own" in plan and "NaN bytes" in plan, "the loaded library ignores BSX_ARENA_NO_REUSE / BSX_ARENA_POISON"
        expected, _, program_on = stored_by_plan(plan, nt, n_stepped, True, chained=False)      # (pw_chain3_k is a kernel of the split-f16 mode)
        expected_half = half_by_plan(plan, nt, n_stepped)
        # what the rewrites store where the file has no tensor (the 1x1 convolution moved below its resize): read, and audited against the convolution of the resize's input
        moved = G.moved_convs(plan, m)
        synthetic = {t for t in stored_by_plan(plan, 1 << 30, n_stepped, True, chained=False)[0] if t >= nt}
        synthetic_half = {t for t in half_by_plan(plan, 1 << 30, n_stepped) if t >= nt}
        # (other synthetic tensors — DeepLab's folded pool branch, a per-frame f32 bias — are f32 operands of a launch whose output IS audited; a HALF-stored one that
        #  the audit does not know would be a rounding it cannot see)
        assert synthetic_half <= set(moved) & synthetic, "the plan stores tensors %s as halves that are neither the file's nor a moved convolution's\n%s" % (
            sorted(synthetic_half - set(moved)), plan)
        synthetic &= set(moved)
        rounding = G.operand_rounding_rule(plan, m, mode, n_stepped)
        if mode == "act16":
            assert program_on and "segment head" in plan and "16-bit activation storage" in plan, "BSX_ACT16 needs the segmented path with the specialised middle kernel\n" + plan
            assert len(expected_half) >= 5 and not rounding and synthetic_half == synthetic
        else:
            assert not program_on and len(rounding) >= 16
            assert bool(expected_half) == (mode == "fast16"), "tensors the plan stores as halves under %s at %d streams: %s" % (mode, n_stepped, sorted(expected_half))
        assert expected_half <= expected
        frames = G.audit_frames(W, H)
        oc = oracle.Ctx(path, W, H)
        om = oc.model()
        if f32_input:
            rng = np.random.default_rng(77)
            shp = tuple(m.tensors[t_in].shape)[1:]
            inputs = [rng.uniform(0.0, 1.0, shp).astype(np.float32) for _ in range(3)] + [np.zeros(shp, np.float32), np.ones(shp, np.float32)]
            names = ["uniform0", "uniform1", "uniform2", "all 0", "all 1"]
        else:
            inputs = [oc.prep(f) for _, f in frames]
            names = [nm for nm, _ in frames]
        which = [i % len(inputs) for i in range(n_stepped)]             # stream i runs input i mod 5
        if f32_input:
            mg.input_tensor()[:n_stepped].copy_(torch.from_numpy(np.stack([inputs[k] for k in which])).cuda())
        else:
            mg.run_stage(0, torch.from_numpy(np.stack([frames[k][1] for k in which])).cuda())
        mg.run_stage(1, n=n_stepped)
        torch.cuda.synchronize()
        per_input = {}                                                  # input → (oracle tensors, unforced float64 run): computed once, shared by the streams on it
        problems, record, f32_seen = [], [], {}
        for i in range(n_stepped):
            k = which[i]
            dev = G.read_stored(mg, nt, i)
            got_in = dev.pop(t_in, None)
            assert got_in is not None and np.array_equal(got_in.reshape(inputs[k].shape), inputs[k]), "stream %d: the network input read back differs from what was given" % i
            nonfinite = [t for t in dev if not np.isfinite(dev[t]).all()]
            assert not nonfinite, "stream %d (%s): tensors %s come back non-finite: served, but not (completely) written, or past the range of a half\n%s" % (i, names[k], nonfinite, plan)
            assert set(dev) == expected, "stream %d: the entry serves %s beyond the plan's stored set and refuses %s of it\n%s" % (
                i, sorted(set(dev) - expected), sorted(expected - set(dev)), plan)
            for t in sorted(synthetic):
                dev[t] = mg.graph_tensor(t, i)
                assert np.isfinite(dev[t]).all(), "stream %d: the moved convolution's tensor %d comes back non-finite" % (i, t)
            for t in dev:
                if t not in expected_half | synthetic_half:
                    f32_seen[t] = f32_seen.get(t, 0) + G.not_half_representable(dev[t])
            if k not in per_input:
                om.invoke(inputs[k])
                per_input[k] = (G.oracle_tensors(om, sorted(t for t in dev if t < nt)), G.run(path, inputs[k][None], model=m)[0])      # (the oracle has the file's tensors only)
            ot, exact = per_input[k]
            rows = G.audit_reduced(path, inputs[k][None], dev, ot, expected_half | synthetic_half, rounding, exact, m, moved=moved)
            assert len(rows) == len(expected) + len(synthetic), "stream %d: %d of %d stored tensors audited" % (i, len(rows), len(expected) + len(synthetic))
            outside = sum(r["outside"] for r in rows)
            wf = max((r for r in rows if not r["half"]), key=lambda r: r["worst"])
            out = next(r for r in rows if r["t"] == t_out)
            print("%-7s %-9s %-28s stream %d %-9s: %3d tensors audited, %2d stored as halves, %d elements outside, worst |d - v| / (B32 + allowance) of an f32 tensor %5.2f at t%-3d, "
                  "accumulated error at the output %.3g (scale %.3g)" % (arch, "real" if real else "synthetic", _mode_id(case), i, names[k], len(rows),
                                                                        sum(r["half"] for r in rows), outside, wf["worst"], wf["t"], out["acc"], out["scale"]))
            record.append({"stream": i, "input": names[k], "audited": len(rows), "half": sum(r["half"] for r in rows), "outside": outside, "worst_f32": wf["worst"],
                           "worst_f32_tensor": wf["t"], "worst": max(r["worst"] for r in rows), "out_acc": out["acc"], "out_scale": out["scale"]})
            bad = G.failing_reduced(rows)
            if bad:
                problems.append("stream %d (%s): tensors %s have elements outside their interval; the first is the one to look at\n%s" % (i, names[k], bad, G.format_table_reduced(rows)))
        # ---- a tensor the plan marks f32 really is one: over the streams it holds at least one value that no half represents
        looks_half = sorted(t for t, cnt in f32_seen.items() if cnt == 0)
        print("f32-stored tensors: %d; values no half represents, fewest in one tensor: %s" % (len(f32_seen), min(f32_seen.values()) if f32_seen else None))
        seconds = time.time() - t_start
        out_path = os.environ.get("BSX_LAYER_AUDIT_OUT")
        if out_path:
            with open(out_path, "a") as f:
                f.write(json.dumps({"model": arch, "weights": "real" if real else "synthetic", "path": _mode_id(case), "stored": len(expected) + len(synthetic),
                                    "half": len(expected_half | synthetic_half), "rounding_ops": sorted(rounding), "seconds": round(seconds, 1), "streams": record}) + "\n")
        assert not looks_half, "tensors %s are marked f32 by the plan and hold nothing but half-representable values\n%s" % (looks_half, plan)
        assert not problems, "\n".join(problems)
    finally:
        if oc is not None:
            oc.close()
        mg.close()
        for k in KNOBS + ("BSX_ARENA_NO_REUSE", "BSX_ARENA_POISON"):
            monkeypatch.delenv(k, raising=False)
