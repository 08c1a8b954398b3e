"""Layer-by-layer audit of the GPU network against float64 (run on a GPU box; needs libbsx_dbg.so, the build with the debug switches).

Usage: python tools/debug_layers.py <model.tflite|key> [W H]     (execution-path switches such as BSX_NO_RTC=1 or BSX_F16_GEMM=off are taken from the environment)
       python tools/debug_layers.py --model-size family:HxW [W H]    a Meet-family ("lite") or MLKit ("mlkit") graph of that network input size, e.g. lite:104x168:
                                                                     the model of tests/model_size_cases.py where that is one of its cases (same seed), written to a temporary directory

The same helper and the same table as tests/test_gpu_layers.py (tests/f64_graph.py: audit): per tensor the path stores, its distance from a float64 evaluation of the
operators since the nearest stored tensors upstream (local), the oracle's distance on the same operators (loc.oracle), their ratio (a tensor passes up to 8) and the
accumulated error against the unforced float64 run.  The arena is planned without reuse and filled with NaNs in front of the network stage, so a tensor that is
listed was written by this run.

In the reduced-precision modes (BSX_ACT16=1 on a segmented network, BSX_F16_GEMM=fast / fast16) the table is the one of tests/test_gpu_layers_reduced.py
(tests/f64_graph.py: audit_reduced): per tensor its storage width as the plan text marks it, B32, the largest operand allowance, the count and the first index of
the elements outside their interval (must be 0) and the worst |d - v| / (B32 + allowance)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("BSX_ARENA_NO_REUSE", "1")
os.environ.setdefault("BSX_ARENA_POISON", "1")
from backscrub_amd import build  # noqa: E402

os.environ.setdefault("BSX_LIBRARY", build.LIB_DBG)
import torch  # noqa: E402

import backscrub_amd  # noqa: E402
import f64_graph as G  # noqa: E402
from backscrub_amd import tflite_io  # noqa: E402
from conftest import MODEL_KEYS, model_path  # noqa: E402
from oracle import oracle_py as O  # noqa: E402

argv = sys.argv[1:]
if argv and argv[0] == "--model-size":
    import re
    import tempfile
    from model_size_cases import CASES, Case, model_file  # noqa: E402
    spec = re.fullmatch(r"(lite|mlkit):(\d+)x(\d+)", argv[1] if len(argv) > 1 else "")
    if not spec:
        sys.exit("--model-size takes family:HxW with family lite or mlkit, e.g. lite:104x168")
    fam, mh, mw = spec.group(1), int(spec.group(2)), int(spec.group(3))
    case = next((c for c in CASES if (c.family, c.H, c.W) == (fam, mh, mw)), None) or Case("%s-%dx%d" % (fam, mh, mw), fam, mh, mw, 4999, *([None] * 7))
    path = model_file(case, tempfile.mkdtemp(prefix="bsx_model_size_"))
    argv = argv[2:]
else:
    arg = argv[0] if argv else "lite"
    path = model_path(arg) if arg in MODEL_KEYS else arg
    argv = argv[1:]
W, H = (int(argv[0]), int(argv[1])) if len(argv) > 1 else (640, 480)
m = tflite_io.load(path)
frames = G.audit_frames(W, H)
mg = backscrub_amd.MaskGen(path, W, H, n_streams=len(frames))
plan = mg.plan()
print(plan)
if "slot of its own" not in plan or "NaN bytes" not in plan:      # the release library ignores both switches: its table would list slots that were reused or never written
    sys.exit("the loaded library (%s) does not honour BSX_ARENA_NO_REUSE / BSX_ARENA_POISON: build libbsx_dbg.so (python -m backscrub_amd.build) and load that" %
             os.environ["BSX_LIBRARY"])
mode = os.environ.get("BSX_F16_GEMM") if os.environ.get("BSX_F16_GEMM") in G.OPERAND_MODES else ("act16" if "16-bit activation storage" in plan else None)
if mode:
    from test_gpu_layers import half_by_plan  # noqa: E402
    from test_gpu_layers import stored_by_plan  # noqa: E402
    moved = G.moved_convs(plan, m)                  # the 1x1 convolutions a rewrite moved below their resize: stored where the file has no tensor
    synthetic = sorted(t for t in stored_by_plan(plan, 1 << 30, len(frames), True, chained=False)[0] if t in moved)
    half = half_by_plan(plan, 1 << 30, len(frames))
    rounding = G.operand_rounding_rule(plan, m, mode, len(frames))
    print("reduced-precision mode %s: %d tensors stored as halves %s, %d operators with f16 operands %s" % (mode, len(half), sorted(half), len(rounding), sorted(rounding)))
oc = O.Ctx(path, W, H)
mg.run_stage(0, torch.from_numpy(np.stack([f for _, f in frames])).cuda())
mg.run_stage(1, n=len(frames))
torch.cuda.synchronize()
bad = 0
for i, (name, f) in enumerate(frames):
    x = oc.prep(f)
    oc.infer()
    dev = G.read_stored(mg, len(m.tensors), i)
    dev.pop(m.inputs[0], None)
    if mode:
        ot = G.oracle_tensors(oc.model(), sorted(dev))
        dev.update({t: mg.graph_tensor(t, i) for t in synthetic})
        rows = G.audit_reduced(path, x[None], dev, ot, half, rounding, model=m, moved=moved)
        print("---- stream %d: %s — %d stored tensors, %d as halves, %d elements outside their interval" % (i, name, len(rows), sum(r["half"] for r in rows), sum(r["outside"] for r in rows)))
        print(G.format_table_reduced(rows))
        bad += len(G.failing_reduced(rows))
        continue
    rows = G.audit(path, x[None], dev, G.oracle_tensors(oc.model(), sorted(dev)), model=m)
    n, ratio, at, acc, acc_at = G.summary(rows)
    print("---- stream %d: %s — %d stored tensors, worst local ratio %.2f at t%d, worst accumulated error %.1f ulps at t%d" % (i, name, n, ratio, at, acc, acc_at))
    print(G.format_table(rows))
    bad += len(G.failing(rows)) + sum(not r["finite"] for r in rows)
print("tensors over the bar, with elements outside their interval or non-finite:", bad)
mg.close()
sys.exit(1 if bad else 0)
