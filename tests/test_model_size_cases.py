"""The cases of the model-size audit (tests/model_size_cases.py), as far as they can be checked without a GPU: every case plans, its plan text states the facts its row
of the table names (so a later change of the planner's tile targets says which case lost its purpose), the head's pad constants are what the derivation in
docs/design/02a-layer-audit.md says, the specialised segment source of every segmented case compiles for gfx950 without scratch, and the model generator writes the
transpose convolution's own output shape."""
import hashlib
import os
import re
import subprocess

import pytest

import deeplab_size_cases as D
from conftest import ROOT
from model_size_cases import CASES, FORCED, FORCED_KNOBS, SEGMENTED, STEM_PAD, BY_NAME, model_file
from test_k3_frame_codegen import FRAME_LINE, HIPCC, LDS_CU, TILES_LINE

TILE_LINE = r"^segment (\w+)\s+tile (\d+)x(\d+), (\d+)x(\d+) tiles per frame, LDS ([\d.]+) KiB"


@pytest.fixture(scope="module")
def api():
    from backscrub_amd import api as a
    a.lib()
    return a


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("sized_models")
    return {**{c.name: model_file(c, d) for c in CASES}, **{c.name: D.model_file(c, d) for c in D.CASES}}


def plan_facts(d):
    """what a test reads from a plan text: the four tile lines, the k3 form, the step and micro-op counts, the reason there is no specialised middle kernel"""
    tiles = {m.group(1): tuple(int(m.group(i)) for i in (2, 3, 4, 5)) for m in re.finditer(TILE_LINE, d, re.M)}
    f, t = re.search(FRAME_LINE, d, re.M), re.search(TILES_LINE, d, re.M)
    k3 = ("frame", int(f.group(1))) if f else (("tiles", t.group(2), int(t.group(3))) if t else None)
    steps = int(re.search(r"^ops=\d+ nodes=\d+ steps=(\d+) ", d, re.M).group(1))
    prog = re.search(r"^program micro-ops=(\d+) .* hbm_tensors=(\d+) ", d, re.M)
    none = re.search(r"^specialised middle kernel: none \((.*)\)$", d, re.M)
    return {"tiles": tiles or None, "k3": k3, "steps": steps, "micro_ops": int(prog.group(1)), "hbm_tensors": int(prog.group(2)), "middle": none.group(1) if none else None,
            "segmented": any(l.startswith("segment ") for l in d.splitlines())}


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_every_case_plans_and_its_plan_states_the_facts_of_its_row(api, models, case):
    d = api.model_describe(models[case.name])
    got = plan_facts(d)
    assert got["segmented"] == case.segmented, d
    assert got["tiles"] == case.tiles and got["k3"] == case.k3, (got, d)
    assert (got["steps"], got["micro_ops"], got["middle"]) == (case.steps, case.micro_ops, case.middle), (got, d)
    # the <= 4 pixel form of a 1x1 convolution (mo_gemv) has no add operand: an x * s + a convolution of a 2x2 or 1x1 decoder level must not take it
    assert not re.search(r"^P\d+ \S*\+muladd .* gemv ", d, re.M), d
    if case.segmented:
        assert len(re.findall(r"^segment ", d, re.M)) == 6                          # four tile lines, the partial sums, the k3 form
        assert case.k3[-1] <= LDS_CU or (case.k3[0] == "tiles" and "does not fit" in case.k3[1])
    else:
        assert "segment" not in d and re.search(r"^P0 ", d, re.M), d                  # a whole-network program, not a half-segmented plan and not per launch
        assert "specialised middle kernel: none" in d


def test_the_table_reaches_what_it_claims():
    """the properties the cases were chosen for, from the table itself (a case edited later must not lose them)"""
    t = {c.name: c for c in CASES}
    assert all(v == (v[0], v[1], 1, 1) for v in t["lite-16x16"].tiles.values())
    assert t["lite-32x48"].tiles["head"][2:] == (2, 1) and t["lite-32x48"].tiles["tail"][2:] == (1, 2)
    assert t["lite-104x168"].k3[0] == "tiles" and t["lite-104x168"].family == "lite" and t["lite-104x168"].k3[2] <= LDS_CU
    assert t["mlkit-128x128"].k3[0] == "tiles" and t["mlkit-128x128"].k3[2] <= LDS_CU and t["mlkit-264x248"].k3[2] > LDS_CU
    assert t["mlkit-264x248"].tiles["tail"][0] == 17 and all(n % 2 for n in t["mlkit-264x248"].tiles["k3"][2:])
    assert t["lite-160x96"].tiles["head"][2] > t["lite-160x96"].tiles["head"][3]
    # a partial last tile: the extent is no multiple of the tile (104x168: head H2 = 26 in 7 tiles of 4, k2 H3 = 13 in 4 of 4, k3 26 in 2 of 13 is exact, 21 columns in 3 of 7)
    assert 7 * 4 > 26 and 4 * 4 > 13 and 3 * 18 > 52
    assert len(CASES) == 13 and len({c.name for c in CASES}) == 13 and len({c.seed for c in CASES}) == 13
    assert [c.name for c in CASES if c.refused] == ["mlkit-250x246"] and -(-250 // 2) * 2 - 1 < 250 and t["mlkit-249x245"].refused is None
    assert sum(c.segmented for c in CASES) == 7
    for name, _, env in FORCED:
        assert t[name].segmented and set(env) <= set(FORCED_KNOBS)


@pytest.mark.parametrize("case", SEGMENTED, ids=[c.name for c in SEGMENTED])
def test_the_pads_of_a_segmented_plan_and_its_specialised_source(api, models, case, tmp_path):
    """Uniform 2x resize weights lo2 -> B and lo -> A force H(b0) = 2 H(c0) and H(A) = 2 H(b0): b0 and A are even, both stride-2 depthwise convolutions have no top / left
    pad, and only the stem's pad is free (H0 = 2 H(A) - 1 gives 1).  The specialised source carries the constants, compiles for gfx950 and spills nothing."""
    src = api.model_seg_source(models[case.name])
    head = src[src.index("constexpr SegHead kSegHEAD = [] {"):]
    head = head[:head.index("return t; }();")]
    k = {a: int(v) for a, v in re.findall(r"t\.(\w+) = (-?\d+);", head)}
    pad = STEM_PAD.get(case.name, 0)
    assert (k["stem_pt"], k["stem_pl"], k["dw_pt"], k["dw_pl"]) == (pad, pad, 0, 0), k
    assert (k["H0"], k["W0"]) == (case.H, case.W) and (k["H1"], k["W1"]) == (-(-case.H // 2), -(-case.W // 2)) and (k["H1"], k["W1"]) == (2 * k["H2"], 2 * k["W2"])
    assert (k["TR"], k["TC"], k["tiles_y"], k["tiles_x"]) == case.tiles["head"]
    k2 = src[src.index("constexpr SegK2 kSegK2 = [] {"):]
    assert re.search(r"t\.dw_pt = 0; t\.dw_pl = 0;", k2[:k2.index("return t; }();")])
    assert ("#define BSXS_SEG_K3F %d\n" % (case.k3[0] == "frame")) in src
    p = tmp_path / "seg.hip"
    p.write_text(src)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S", "-o", str(p) + ".s", str(p)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = (tmp_path / "seg.hip.s").read_text()
    kernels = ["bsx_seg_head", "bsx_seg_k2", "bsx_seg_k3", "bsx_seg_tail"] + (["bsx_seg_k3f"] if case.k3[0] == "frame" else [])
    for name in kernels:                                                              # the shipped shapes show no scratch in any of them (tests/test_mid_codegen.py)
        blk = asm[asm.index(".amdhsa_kernel %s\n" % name):]
        blk = blk[:blk.index(".end_amdhsa_kernel")]
        sc = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", blk).group(1))
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", blk).group(1))
        assert sc == 0 and lds <= LDS_CU, "%s of %s: %d B of scratch, %d B of LDS" % (name, case.name, sc, lds)
    assert (".amdhsa_kernel bsx_seg_k3f\n" in asm) == (case.k3[0] == "frame")


@pytest.mark.parametrize("name,what,env", FORCED, ids=[re.sub(r"\W+", "_", "%s-%s" % (n, w)) for n, w, _ in FORCED])
def test_the_forced_tile_variants_plan_in_the_debug_library_only(api, models, name, what, env, monkeypatch, debug_switches):
    from backscrub_amd import build
    path, case = models[name], BY_NAME[name]
    for k in FORCED_KNOBS:
        monkeypatch.delenv(k, raising=False)
    plain = plan_facts(debug_switches.model_describe(path))
    assert plain["tiles"] == case.tiles and plain["k3"] == case.k3
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got = plan_facts(debug_switches.model_describe(path))
    if "BSX_SEG_TILES" in env:
        # 32x48: head 8x12 at targets 2,5 -> 2x4 in 4x3; k2 4x6 at 2,3 -> 2x3 in 2x2; k3 8x12 at 3,5 -> 3x4 in 3x3 (last row tile: 2 rows); tail 16x24 at 5,5 -> 4x5 in 4x5 (last column tile: 4)
        assert got["tiles"] == {"head": (2, 4, 4, 3), "k2": (2, 3, 2, 2), "k3": (3, 4, 3, 3), "tail": (4, 5, 4, 5)}, got
        assert got["k3"][0] == "frame"
    else:
        assert got["tiles"] == case.tiles and got["k3"][0] == "tiles" and got["k3"][1] == "switched off" and got["k3"][2] == case.k3[1], got
    for k in env:
        assert k.encode() not in open(build.LIB, "rb").read() and k.encode() in open(build.LIB_DBG, "rb").read()


# ---- the DeepLab graph at other sizes and widths (tests/deeplab_size_cases.py) ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.CASES, ids=[c.name for c in D.CASES])
def test_every_deeplab_case_plans_and_its_plan_states_the_facts_of_its_row(api, models, case):
    from backscrub_amd import tflite_io as T
    from tools import make_synthetic_model as S
    d = api.model_describe(models[case.name])
    got = D.plan_facts(d)
    assert (got["steps"], got["micro_ops"]) == (case.steps, case.micro_ops), (got, d)
    assert got["head_fused"] == case.head_fused and got["chain"] == case.chain, (got, d)
    assert got["pairs"] == D.pairs_of(case), (got["pairs"], d)
    assert got["unfused"] == case.unfused and set(got["pairs"]) | set(got["unfused"]) == set(D.EXPANDS), (got, d)
    assert "segment" not in d and ("specialised middle kernel: none" in d) == (case.micro_ops > 0), d
    # the graph is the shipped one in everything but its extents and widths: the same 70 operators, every extent by the operators' own rules
    m, ref = T.load(models[case.name]), T.load(S.ensure("deeplab"))
    assert [op.name for op in m.ops] == [op.name for op in ref.ops] and len(m.tensors) == len(ref.tensors)
    assert m.tensors[m.inputs[0]].shape == [1, case.H, case.W, 3] and m.tensors[m.outputs[0]].shape == [1, case.H, case.W, 21]
    fh, fw = case.H, case.W
    for _ in range(3):                                                               # three stride-2 SAME levels: the 1/8 map
        fh, fw = -(-fh // 2), -(-fw // 2)
    resizes = [op for op in m.ops if op.name == "RESIZE_BILINEAR"]
    assert [m.tensors[op.outputs[0]].shape[1:3] for op in resizes] == [[fh, fw], [fh, fw], [case.H, case.W]]
    assert all(op.opts["align_corners"] == 1 and op.opts["half_pixel_centers"] == 0 for op in resizes)
    stem = m.tensors[m.ops[0].outputs[0]].shape
    assert stem[3] == 16 * case.width and m.tensors[next(op for op in m.ops if op.name == "CONCATENATION").outputs[0]].shape == [1, fh, fw, 512]


def test_the_deeplab_table_reaches_what_it_claims():
    """the arithmetic behind the rows (a case edited later must not lose it); the kernels' own thresholds are quoted where they are used"""
    t = D.BY_NAME
    names = [c.name for c in D.CASES]
    assert len(names) == 13 == len(set(names)) == len({c.seed for c in D.CASES}) and all("deeplab" in n for n in names)
    assert not {c.seed for c in D.CASES} & {c.seed for c in CASES}

    def level(c, k):                                                                  # extents of the 1/2^k map
        h, w = c.H, c.W
        for _ in range(k):
            h, w = -(-h // 2), -(-w // 2)
        return h, w

    def partial(rows, bh, nb):                                                        # nb bands of bh rows cover `rows` with a shorter last band
        return (nb - 1) * bh < rows < nb * bh

    # 256x256: even extents at every level (pad_t = pad_l = 0 under SAME, stride 2), a scale that is no power of two, the 64 output rows of the first stride-2 depthwise in 16 bands of 4 exactly
    assert all(x % 2 == 0 for k in range(3) for x in level(t["deeplab-256x256"], k)) and level(t["deeplab-256x256"], 3) == (32, 32) and 16 * 4 == 64
    # 129x129: 33 depthwise rows in 4 bands of 9; the M of its 1/8 and 1/4 levels at the five stepped streams against launch_step's 4096 and 8192
    c = t["deeplab-129x129"]
    assert D.pairs_of(c)[3] == (16, 9, 4) and partial(33, 9, 4) and level(c, 2) == (33, 33) and level(c, 3) == (17, 17)
    assert c.stepped * 17 * 17 == 1445 <= 4096 < c.stepped * 33 * 33 == 5445 < 8192
    assert D.pairs_of(t["deeplab-65x97"])[3][0] == 24 and D.pairs_of(t["deeplab-65x97"])[3][2] == 1 and t["deeplab-65x97"].H != t["deeplab-65x97"].W
    c = t["deeplab-200x312"]
    assert [level(c, k) for k in range(4)] == [(200, 312), (100, 156), (50, 78), (25, 39)]       # even, even, even, then odd in both axes
    # 385x289: the 16-channel chunk in one band on every layer from step 12 on, the dilated ones included; 49 rows in 10 bands of 5; 97 in 11 of 9
    c = t["deeplab-385x289"]
    assert all(D.pairs_of(c)[s] == (16, 49, 1) for s in range(12, 49, 3)) and level(c, 3) == (49, 37) and partial(49, 5, 10) and partial(97, 9, 11)
    # 353x481: the stem is 241 wide behind a 481-wide input: > 339, the widest input whose band fits the LDS of dl_head0_k; banded DILATED pairs with a partial
    # last band (45 rows in 3 of 15 is exact, in 4 of 12 it is not); the 1/8 level has 8192 rows at the streams it steps
    c = t["deeplab-353x481"]
    assert c.W > 339 and not c.head_fused and level(c, 3) == (45, 61)
    assert all(D.pairs_of(c)[s] == (16, 15, 3) for s in range(21, 40, 3)) and all(D.pairs_of(c)[s] == (16, 12, 4) for s in (42, 45, 48)) and partial(45, 12, 4) and 3 * 15 == 45
    assert c.stepped * 45 * 61 >= 8192 and D.pairs_of(c)[9][1] == 2 and D.pairs_of(c)[3][1] == 2
    c = t["deeplab-65x513"]
    assert c.W > 339 and not c.head_fused and c.unfused == (3,) and level(c, 1) == (33, 257)
    assert t["deeplab-65x337"].head_fused and 337 <= t["deeplab-65x337"].W <= 339 and not t["deeplab-65x329"].head_fused and t["deeplab-65x329"].W < 340
    # 33x33 and 17x17: from the level with fewer than 64 pixels on nothing is fused; the dilation reaches (d = 4 on 5x5: 4 * d > H) and passes (3x3) the map's size
    assert level(t["deeplab-33x33"], 3) == (5, 5) and 5 * 5 < 64 and t["deeplab-33x33"].unfused == tuple(range(12, 49, 3)) and 5 < 4 * 2
    assert level(t["deeplab-17x17"], 3) == (3, 3) and level(t["deeplab-17x17"], 2) == (5, 5) and t["deeplab-17x17"].unfused == tuple(range(6, 49, 3))
    c = t["deeplab-9x9"]
    assert level(c, 3) == (2, 2) and c.micro_ops == 58 and c.steps == 59 and not c.pairs and c.unfused == D.EXPANDS
    assert [x.name for x in D.CASES if x.micro_ops] == ["deeplab-9x9"]
    # the wide case: 8192 rows at its 1/8 level need ten streams (nine have 7425); the expands from Cin = 160 (K padded to 160 > 96) are not fused
    c = t["deeplab-wide-193x257"]
    assert c.width == 2 and level(c, 3) == (25, 33) and c.stepped * 25 * 33 >= 8192 > (c.stepped - 1) * 25 * 33 and c.streams >= c.stepped
    assert c.unfused == (42, 45, 48) and not c.chain and not c.head_fused
    assert [x.name for x in D.CASES if x.rows is not None] == ["deeplab-wide-193x257"] and D.ROWS_DIFFERENT == (0, 1, 4)      # the one case that cannot lose streams
    assert set(D.HOST_PROOF) <= set(names) and all(t[n].H * t[n].W <= 65 * 97 for n in D.HOST_PROOF)


@pytest.mark.parametrize("env,keeps", [({"BSX_NO_HEAD0": "1"}, ("pairs", "chain")), ({"BSX_NO_IR_FUSE": "1"}, ("chain",)), ({"BSX_NO_REWRITES": "1"}, ())],
                         ids=["no_head0", "no_ir_fuse", "no_rewrites"])
def test_a_switch_of_the_debug_library_removes_its_own_fusions_from_a_deeplab_plan_only(models, env, keeps, monkeypatch, debug_switches):
    """what tests/test_gpu_model_sizes.py asserts of a context's plan on the rows that switch one fusion off: the other facts of the case's row stay"""
    for k in ("BSX_NO_HEAD0", "BSX_NO_IR_FUSE", "BSX_NO_REWRITES"):
        monkeypatch.delenv(k, raising=False)
    for name in ("deeplab-129x129", "deeplab-353x481", "deeplab-wide-193x257"):
        case = D.BY_NAME[name]
        want = {"head_fused": case.head_fused, "pairs": D.pairs_of(case), "chain": case.chain}
        assert {k: v for k, v in D.plan_facts(debug_switches.model_describe(models[name])).items() if k in want} == want
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        got = D.plan_facts(debug_switches.model_describe(models[name]))
        for k in env:
            monkeypatch.delenv(k)
        assert {k: got[k] for k in keeps} == {k: want[k] for k in keeps}, (name, env, got)
        # (BSX_NO_IR_FUSE switches the fused head off as well; without the rewrites the step list has a micro-op form, and a plan with a program fuses nothing: plan.cpp)
        for gone in {"head_fused", "pairs", "chain"} - set(keeps):
            assert not got[gone], (name, env, gone, got[gone])


# sha256 of the four synthetic models of the shipped sizes, as the generator wrote them before it learnt the transpose convolution's cropped output shape
SHIPPED = {
    "lite": "232407a407d39cf124836038ddb6f46d69d374cb156ca7ce4c7c12664135d95c",
    "full": "f4c0054c5cab2903438e0b6254e274b3b505cbe323e78982eb328569771649ef",
    "mlkit": "f7dfe10d650fadcfdf2d91e726832eff2d36a55df4d4a6f80f927e0b8212c690",
    "deeplab": "9eee438e63f34c0382ed8b03bb79f23f4dc92fb50eb78259343cd7546844fa70",
}


@pytest.mark.parametrize("key", list(SHIPPED))
def test_the_shipped_synthetic_models_regenerate_byte_for_byte(key):
    from backscrub_amd import tflite_io as T
    from tools import make_synthetic_model as S
    data = T.dumps(S.build(key))
    assert hashlib.sha256(data).hexdigest() == SHIPPED[key]
    with open(S.ensure(key), "rb") as f:                                             # the file under tests/golden/models (generated by build(), not committed)
        assert f.read() == data
    assert os.path.dirname(S.ensure(key)) == os.path.join(ROOT, "tests", "golden", "models")


@pytest.mark.parametrize("name", ["lite-97x161", "mlkit-250x246", "mlkit-249x245"])
def test_a_model_with_an_odd_A_has_the_cropped_output_shape_and_loads(api, oracle, models, name):
    """Convolution2DTransposeBias under SAME: stride * (in - 1) + k - pad with pad = 1 for an odd input — 2h - 1, not 2h.  The planner refuses a file that says 2h
    ("tconv output shape mismatch"); the operator of the reference (the oracle's object code) resizes its output to 2h - 1 whatever the file says."""
    import numpy as np
    from backscrub_amd import tflite_io as T
    case = BY_NAME[name]
    m = T.load(models[name])
    tc = m.ops[-2] if case.family == "mlkit" else m.ops[-1]
    assert tc.code == 32
    ah, aw = -(-case.H // 2), -(-case.W // 2)
    assert ah % 2 == 1 and aw % 2 == 1
    assert m.tensors[tc.inputs[0]].shape[1:3] == [ah, aw] and m.tensors[tc.outputs[0]].shape[1:3] == [2 * ah - 1, 2 * aw - 1]
    assert m.tensors[m.outputs[0]].shape[1:3] == [2 * ah - 1, 2 * aw - 1]
    d = api.model_describe(models[name])
    assert re.search(r"-> out %dx%dx%d " % (2 * ah - 1, 2 * aw - 1, 1 if case.family == "mlkit" else 2), d), d
    # The fused tail micro-op (kernels_frame.hip: tail_body) stores the whole 2x2 block of every input pixel: at a cropped output the second row of the last input
    # row lies behind the tensor (the next frame's first row; behind the buffer for the last frame) and the second column of the last input column is the next row's
    # first pixel.  The planner keeps the three micro-ops apart there (the stand-alone one walks the OH x OW outputs), and fuses as before where nothing is cropped.
    assert "tail[pw+dw+tconv]" not in d and re.search(r"^P\d+ tconv#\d+ +%dx%dx16->%dx%dx\d in:hbm out:hbm" % (ah, aw, 2 * ah - 1, 2 * aw - 1), d, re.M), d
    assert "tail[pw+dw+tconv]" in api.model_describe(models["lite-100x164"])
    om = oracle.Model(models[name])
    try:
        x = np.random.default_rng(3).uniform(0, 1, om.shape(om.input)).astype(np.float32)
        y = om.invoke(x)
        assert y.size == (2 * ah - 1) * (2 * aw - 1) * (1 if case.family == "mlkit" else 2) and np.isfinite(y).all() and y.std() > 1e-4
    finally:
        om.close()
