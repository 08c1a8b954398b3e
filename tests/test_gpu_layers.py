"""Every tensor the GPU network stores, on every execution path, against a float64 evaluation of its own operator group.

The other GPU tests see a network at its last tensor only (logits within 1e-4 of the oracle's f32 logits).  Here every tensor that a path writes to HBM is read back
per stream (libbsx_dbg.so, BSX_ARENA_NO_REUSE=1: no slot is written twice) and audited by tests/f64_graph.py: the float64 evaluation is FORCED through the device's
own values, so each tensor is compared with a float64 evaluation of exactly the operators between it and the nearest stored tensors upstream — one kernel's or one
fused launch's rounding, measured against the oracle's rounding on the same operators and input.  tests/test_f64_forced_host.py proves that bar fair (an independent
f32 evaluation passes at less than half of it) and sharp (a 2^-16 change of one channel, one border row, one corner pixel fail at the tensor they are in).

BSX_ARENA_POISON=1 fills the arena with NaN bytes in front of the network stage: a tensor that the read-back entry serves although the path keeps it in LDS or in
registers comes back non-finite.  The set the entry serves must be exactly what the plan text says the path stores.

The accumulated error of interior tensors (device against the UNFORCED float64 run) is printed and recorded (docs/design/02a-layer-audit.md), not asserted: on the
black and white inputs the networks amplify rounding a hundredfold, and the ratio of two amplified errors is noise.  At the network output it is asserted."""
import json
import os
import re

import numpy as np
import pytest

from conftest import reference_model_path, synthetic_model_path
from test_gpu_parity import NETWORK_PATHS

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import f64_graph as G  # noqa: E402

W, H = 640, 480
N_STREAMS, N_STEPPED = 8, 5
KNOBS = ("BSX_F32_INPUT", "BSX_ACT16", "BSX_NO_RTC", "BSX_NO_SEGMENTS", "BSX_NO_FRAME_PROGRAM", "BSX_F16_GEMM", "BSX_NO_REWRITES", "BSX_FORCE_FRAME_PROGRAM", "BSX_NO_IR_FUSE",
         "BSX_NO_HEAD0", "BSX_NO_CHAIN3")
F32_INPUT = "arbitrary f32 network inputs (BSX_F32_INPUT), stage 1 only"
NO_FUSION = "one launch per step, no rewrites, no fused kernels"


def _paths(arch):
    """the rows of NETWORK_PATHS (`full` takes lite's), the per-launch path with every rewrite and fusion off, and the default path fed with arbitrary f32 inputs"""
    rows = [(name, dict(env)) for name, env, _ in NETWORK_PATHS["lite" if arch == "full" else arch]]
    off = {"BSX_NO_REWRITES": "1", "BSX_NO_IR_FUSE": "1", "BSX_NO_HEAD0": "1"}
    if arch != "deeplab":
        off["BSX_NO_FRAME_PROGRAM"] = "1"
    return rows + [(NO_FUSION, off), (F32_INPUT, {"BSX_F32_INPUT": "1"})]


# real weights where they are fixtures; the synthetic model of every architecture (random weights: gates and pools far from their trained, nearly constant values)
MODELS = [("lite", True), ("full", True), ("mlkit", True), ("lite", False), ("full", False), ("mlkit", False), ("deeplab", False)]
CASES = [(arch, real, i) for arch, real in MODELS for i in range(len(_paths(arch)))]

# Stored tensors that hold something else than the file's tensor of that index BY DESIGN of a graph rewrite: (architecture, path name) → {tensor: what it holds}.
# They must still be finite.  At most four per path; none on a path without rewrites and fusions.
HOLDS_SOMETHING_ELSE = {}


def _case_id(c):
    arch, real, i = c
    return "%s-%s-%s" % (arch, "real" if real else "synthetic", re.sub(r"[^a-z0-9]+", "_", _paths(arch)[i][0].lower()).strip("_")[:40])


SEGMENT_STORES = r"^segment .* stores((?: t\d+(?::f16)?)+)$"


def segment_stores(plan, width=None):
    """the tensors the segment lines say their kernels store (width "f16": only those marked as packed halves, "t33:f16")"""
    named = [t for mm in re.finditer(SEGMENT_STORES, plan, re.M) for t in mm.group(1).split()]
    return {int(t[1:].split(":")[0]) for t in named if width is None or t.endswith(":" + width)}


def half_by_plan(plan, n_file_tensors, n):
    """The stored tensors the plan text marks as 16-bit storage for a batch of n: "hbm f16" on a P line of the frame program, "t33:f16" on a segment line, and — per-launch
    path — the "f16 storage:" line of a fused expand + depthwise pair, which names the pixel count from which its output is stored as halves."""
    half = {int(m.group(1)) for m in re.finditer(r"^P\d+ .* -> t(\d+) hbm f16$", plan, re.M)} | segment_stores(plan, "f16")
    for m in re.finditer(r"^f16 storage: .* store t(\d+) \((\d+)x(\d+)x\d+ per frame\) as f16 at (\d+) pixels and more", plan, re.M):
        if n * int(m.group(2)) * int(m.group(3)) >= int(m.group(4)):
            half.add(int(m.group(1)))
    return {t for t in half if t < n_file_tensors}


def stored_by_plan(plan, n_file_tensors, n, f16_gemm, chained=None):
    """The file tensors the plan text says this path writes to HBM, the network output included, the network input not.
    per-launch path: every step's output, minus the interiors of the fused launches the text announces (fused head; expand + depthwise where the f16 GEMM
    kernels run; the chain of three 1x1 convolutions from 8192 pixels up — chained: the split-f16 mode only, i.e. not under BSX_F16_GEMM=fast / fast16; default: as
    f16_gemm).  frame program: the outputs its P lines mark "hbm" (or "output"), plus — segmented — what
    the segment lines store."""
    steps = [(int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4))) for m in            # (index, OH, OW, output tensor)
             re.finditer(r"^\s*(\d+) \w+\s+\S.*?\s+in \d+x\d+x\d+ -> out (\d+)x(\d+)x\d+ .* t-?\d+->t(\d+)$", plan, re.M)]
    assert steps, "no step lines in the plan text"
    program_on = re.search(r"^frame program: ON", plan, re.M) is not None
    chained = f16_gemm if chained is None else chained
    stored = set()
    if program_on:
        for m in re.finditer(r"^P\d+ .* -> t(\d+) (lds|hbm|elided|output)(?: f16)?$", plan, re.M):
            if m.group(2) in ("hbm", "output"):
                stored.add(int(m.group(1)))
        stored |= segment_stores(plan)
        stored.add(steps[-1][3])
    else:
        out_of = {i: out for i, _, _, out in steps}
        dims = {i: (oh, ow) for i, oh, ow, _ in steps}
        stored = set(out_of.values())
        lines = plan.split("\n")
        for k, line in enumerate(lines):
            owner = re.match(r"^\s*(\d+) \w+", lines[k - 1]) if k else None
            if "^ fused with steps 1 and 2" in line:
                stored -= {out_of[0], out_of[1]}
            m = re.search(r"\^ fused with step (\d+) \(expand", line)
            if m and f16_gemm:
                stored.discard(out_of[int(m.group(1)) - 1])
            m = re.search(r"\^ chained with steps (\d+) and (\d+) at 8192 pixels and more", line)
            if m and chained and owner:
                mid = int(owner.group(1))
                if n * dims[mid][0] * dims[mid][1] >= 8192:
                    stored -= {out_of[int(m.group(1))], out_of[mid]}
    return {t for t in stored if t < n_file_tensors}, [out for _, _, _, out in steps], program_on


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_every_stored_tensor_against_float64(case, oracle, monkeypatch, debug_switches):
    arch, real, pi = case
    pname, env = _paths(arch)[pi]
    path = reference_model_path(arch) if real else synthetic_model_path(arch)
    if real and not os.path.exists(path):
        pytest.fail("model fixture %s is missing" % path)
    audit_every_stored_tensor(debug_switches, oracle, monkeypatch, path, arch, pname, env, weights="real" if real else "synthetic")


def audit_every_stored_tensor(bs, oracle, monkeypatch, path, arch, pname, env, weights="synthetic", model=None, knobs=KNOBS, about_plan=None,
                              n_streams=N_STREAMS, n_stepped=N_STEPPED):
    """The audit of one model file on one execution path (bs: the debug library's binding; arch: the architecture whose paths and input range apply; env: the path's
    switches; model: the name on the printed and recorded lines, default arch; knobs: every switch to clear first; about_plan: called with the context's plan text
    for what a caller has to assert of it; n_streams, n_stepped: streams of the context and how many of them the network stage runs — stream i runs input i mod 5,
    and streams on the same input share the oracle's and the unforced float64 run).  tests/test_gpu_model_sizes.py runs it on the graphs of other input sizes."""
    from backscrub_amd import tflite_io
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    model = model or arch
    real = weights == "real"
    for k in knobs:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("BSX_ARENA_NO_REUSE", "1")
    monkeypatch.setenv("BSX_ARENA_POISON", "1")
    m = tflite_io.load(path)
    nt, t_in, t_out = len(m.tensors), m.inputs[0], m.outputs[0]
    mg = bs.MaskGen(path, W, H, n_streams=n_streams)
    oc = None
    try:
        plan = mg.plan()
        assert "slot of its own" in plan and "NaN bytes" in plan, "the loaded library ignores BSX_ARENA_NO_REUSE / BSX_ARENA_POISON"
        if about_plan:
            about_plan(plan)
        expected, step_outs, program_on = stored_by_plan(plan, nt, n_stepped, env.get("BSX_F16_GEMM") != "off")
        frames = G.audit_frames(W, H)
        oc = oracle.Ctx(path, W, H)
        om = oc.model()
        if pname == F32_INPUT:
            lo, hi = (-1.0, 1.0) if arch == "deeplab" else (0.0, 1.0)
            rng = np.random.default_rng(77)
            shp = tuple(m.tensors[t_in].shape)[1:]
            xs = [rng.uniform(lo, hi, shp).astype(np.float32) for _ in range(3)] + [np.full(shp, lo, np.float32), np.full(shp, hi, np.float32)]
            names = ["uniform%d" % i for i in range(3)] + ["all %g" % lo, "all %g" % hi]
        else:
            names = [nm for nm, _ in frames]
            xs = [oc.prep(f) for _, f in frames]          # (prep itself is asserted bit-exact by test_stages_match_oracle; checked again below through the read-back entry)
        which = [i % len(xs) for i in range(n_stepped)]    # stream i runs input i mod 5
        xs, names = [xs[k] for k in which], [names[k] for k in which]
        if pname == F32_INPUT:
            mg.input_tensor()[:n_stepped].copy_(torch.from_numpy(np.stack(xs)).cuda())
        else:
            mg.run_stage(0, torch.from_numpy(np.stack([frames[k][1] for k in which])).cuda())
        mg.run_stage(1, n=n_stepped)
        torch.cuda.synchronize()
        excluded = HOLDS_SOMETHING_ELSE.get((arch, pname), {})
        assert len(excluded) <= 4 and not (excluded and pname == NO_FUSION)
        problems, record, per_input = [], [], {}
        for i in range(n_stepped):
            dev = G.read_stored(mg, nt, i)
            got_in = dev.pop(t_in, None)
            assert got_in is not None and np.array_equal(got_in.reshape(xs[i].shape), xs[i]), "stream %d: the network input read back differs from what was given" % i
            # ---- every readable tensor is finite: the arena was NaN in front of the stage, so a tensor that is served although the path never wrote it is caught
            #      here, before and independently of the comparison with the plan text
            nonfinite = [t for t in dev if not np.isfinite(dev[t]).all()]
            assert not nonfinite, "stream %d (%s): tensors %s come back non-finite: served, but not (completely) written\n%s" % (i, names[i], nonfinite, plan)
            # ---- the readable set is what the plan says the path stores
            assert set(dev) == expected, "stream %d: the entry serves %s beyond the plan's stored set and refuses %s of it\n%s" % (
                i, sorted(set(dev) - expected), sorted(expected - set(dev)), plan)
            if which[i] not in per_input:
                if pname == F32_INPUT:
                    om.invoke(xs[i])
                else:
                    oc.prep(frames[which[i]][1])
                    oc.infer()
                per_input[which[i]] = (G.oracle_tensors(om, sorted(dev)), G.run(path, xs[i][None], model=m)[0])
            ot, exact = per_input[which[i]]
            rows = G.audit(path, xs[i][None], {t: dev[t] for t in dev if t not in excluded}, ot, exact, m)
            assert len(rows) == len(expected) - len(set(excluded) & expected), "stream %d: %d of %d stored tensors audited" % (i, len(rows), len(expected))
            n, ratio, at, acc, acc_at = G.summary(rows)
            print("%-7s %-9s %-60s stream %d %-9s: %3d tensors audited, worst local ratio %5.2f at t%-3d, worst accumulated error %7.1f ulps at t%d" % (
                model, "real" if real else "synthetic", pname, i, names[i], n, ratio, at, acc, acc_at))
            record.append({"stream": i, "input": names[i], "audited": n, "worst_ratio": ratio, "worst_ratio_tensor": at, "worst_acc_ulps": acc, "worst_acc_tensor": acc_at})
            bad = G.failing(rows)
            if bad:
                problems.append("stream %d (%s): tensors %s are over the bar; the first is the one to look at\n%s" % (i, names[i], bad, G.format_table(rows)))
            # ---- the network output: accumulated error against the unforced float64 run, by the oracle's own accumulated error
            out = next(r for r in rows if r["t"] == t_out)
            out_bar = G.BAR_FACTOR * max(out["acc_oracle"], G.BAR_FLOOR_ULPS * G.ULP * float(exact[t_out].abs().max()))
            if not out["acc"] <= out_bar:
                problems.append("stream %d (%s): network output off by %.3g from float64, the oracle by %.3g: bar %.3g" % (i, names[i], out["acc"], out["acc_oracle"], out_bar))
        # ---- what the stored set must contain
        if program_on and "segment head" in plan:
            named = segment_stores(plan)
            assert {t for t in named if t < nt} | {t_out} <= expected and len(named) >= 5
        if pname == NO_FUSION:
            assert not program_on
            assert {t for t in step_outs if t < nt} == expected, "a path of one launch per step stores every step's output"
        out_path = os.environ.get("BSX_LAYER_AUDIT_OUT")
        if out_path:
            with open(out_path, "a") as f:
                f.write(json.dumps({"model": model, "weights": "real" if real else "synthetic", "path": pname, "stored": len(expected), "streams": record}) + "\n")
        assert not problems, "\n".join(problems)
    finally:
        if oc is not None:
            oc.close()
        mg.close()
        for k in tuple(knobs) + ("BSX_ARENA_NO_REUSE", "BSX_ARENA_POISON"):
            monkeypatch.delenv(k, raising=False)
