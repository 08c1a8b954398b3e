"""The DeepLab graph at other network input sizes and channel widths than the shipped 257x257: the case table of the model-size audit of the per-launch path
(kernels_nn.hip) and the model builder — the sibling of tests/model_size_cases.py, whose `Case` states tile grids and k3 forms that a DeepLab plan does not have.

At 257x257 every extent is 2^k + 1: every stride-2 SAME convolution has pad_t = pad_l = 1, every align-corners resize a dyadic scale (33 -> 257 is exactly 1/8), the
stem band is 3 rows, the three banded expand + depthwise launches are the undilated ones, every dilated depthwise runs whole-frame at 32 channels per workgroup, the
head and the first expand are always fused and the ASPP head is always the 160 -> 256 -> 256 -> 21 chain.  The cases below are the smallest models that leave each of
those habits (docs/design/02a-layer-audit.md, "Other model sizes: DeepLab").  Per case the table states what the planner's text (bsx_model_describe) must say for the
case to keep its purpose: tests/test_model_size_cases.py asserts it without a GPU, tests/test_gpu_model_sizes.py runs the audit.

No GPU and no library at import time; models are written on demand into a directory the caller supplies (nothing is committed)."""
import collections
import os
import re

DCase = collections.namedtuple("DCase", "name H W width seed streams stepped rows head_fused pairs unfused chain steps micro_ops reaches")
# streams, stepped: streams of the audit's context and how many of them the network stage runs
# rows:      None = every row of test_gpu_layers._paths("deeplab"); else the indices of the rows the audit runs (ROWS_DIFFERENT, the wide case: the reason is at the constant)
# head_fused: the plan says "^ fused with steps 1 and 2" (dl_head0_k)
# pairs:     {expand step: (channels per workgroup, depthwise output rows per band, bands)} of every "^ fused with step" line (ir_expand_dw_k), written as runs:
#            ((first step, last step, (CH, BH, bands)), ...) over the expand steps 3, 6, 9, ... 48
# unfused:   the expand steps (a 1x1 convolution whose output a depthwise convolution reads) that have no such line
# chain:     the plan has the "^ chained with steps 53 and 56" line (pw_chain3_k, from 8192 pixels)
FAMILY = "deeplab"
EXPANDS = tuple(range(3, 49, 3))        # the sixteen expand steps of the 58-step list: 3 and 6 (1/2 and 1/4 level, stride 2 behind 3 and 9), 12..18 d = 1, 21..39 d = 2, 42..48 d = 4
# The forced float64 walk of the host takes about a second per stream at 1.67 GMAC per frame, and the wide case needs ten streams for its 8192 rows: its rows take
# 10.5 .. 11.2 s each, more than twice the 4.8 s of the slowest case before it, and it cannot lose streams.  It runs the three rows whose launches differ from each
# other at its size — the default path, the f32 MFMA GEMMs, nothing fused — and not "no graph rewrites" (a plan with an unused program: the launches of "nothing
# fused"), "one launch per layer" (no fusion with the rewrites) and the f32 input (the default's launches on uniform inputs, which no other row of it supplies).
# 353x481 (1.65 GMAC) steps 4 streams — 10980 rows at its 1/8 level (45x61 = 2745 pixels per frame), clear of the 8192 from which the GEMM, chain and f16-storage
# forms run — and at 7 .. 8 s per row keeps all six rows.
ROWS_DIFFERENT = (0, 1, 4)


def _runs(*runs):
    return tuple(runs)


CASES = [
    DCase("deeplab-256x256", 256, 256, 1, 4100, 8, 5, None, True, _runs((3, 3, (16, 4, 16)), (6, 6, (24, 11, 6)), (9, 9, (24, 6, 6)), (12, 48, (32, 32, 1))), (), True, 58, 0,
          "even extents: no top / left pad in the stem (inside dl_head0_k) and in both stride-2 depthwise; align-corners scale 31/255 in resize_k / resize_argmax_iir_k; "
          "bands that divide exactly (64 depthwise rows in 16 bands of 4)"),
    DCase("deeplab-129x129", 129, 129, 1, 4101, 8, 5, None, True, _runs((3, 3, (16, 9, 4)), (6, 6, (24, 33, 1)), (9, 9, (24, 17, 1)), (12, 48, (32, 17, 1))), (), True, 58, 0,
          "partial last band (33 rows in 4 bands of 9); stride-2 depthwise whole-frame; 24-channel chunk in one band; at 5 streams the 1/8 level has M = 1445 "
          "(pw_small_k) and the 1/4 level M = 5445 (pw_conv_k, between 4096 and 8192)"),
    DCase("deeplab-65x97", 65, 97, 1, 4102, 8, 5, None, True, _runs((3, 6, (24, 17, 1)), (9, 9, (24, 9, 1)), (12, 48, (32, 9, 1))), (), True, 58, 0,
          "non-square; first expand whole-frame at 24 channels; stem band of 8 rows (W <= 134)"),
    DCase("deeplab-200x312", 200, 312, 1, 4103, 8, 5, None, True, _runs((3, 3, (16, 3, 17)), (6, 6, (24, 8, 7)), (9, 9, (24, 4, 7)), (12, 48, (32, 25, 1))), (), True, 58, 0,
          "even and non-square: pad 0 in one axis's chain and odd extents later (25x39)"),
    DCase("deeplab-385x289", 385, 289, 1, 4104, 8, 5, None, True, _runs((3, 3, (16, 3, 33)), (6, 6, (24, 9, 11)), (9, 9, (24, 5, 10)), (12, 48, (16, 49, 1))), (), True, 58, 0,
          "the 16-channel chunk on the dilated layers (Cexp 192 / 288 / 480, d = 2 and 4); 49 rows in 10 bands of 5 (partial); stem band of 2 rows"),
    DCase("deeplab-353x481", 353, 481, 1, 4105, 8, 4, None, False,
          _runs((3, 3, (16, 2, 45)), (6, 6, (24, 4, 23)), (9, 9, (24, 2, 23)), (12, 39, (16, 15, 3)), (42, 48, (16, 12, 4))), (), True, 58, 0,
          "head not fused (W > 339): unfused stem conv_k + dw_col_k + K = 16 GEMM; banded dilated depthwise: halo rows 2d of a band, clamped at the frame's bottom; "
          "bands of 2 rows; with 4 streams the 1/8 level (45x61) has 10980 rows: GEMM, chain and f16-storage forms"),
    DCase("deeplab-65x513", 65, 513, 1, 4106, 8, 5, None, False, _runs((6, 6, (24, 4, 5)), (9, 9, (24, 2, 5)), (12, 48, (32, 9, 1))), (3,), True, 58, 0,
          "head not fused, first expand not fused (no band of >= 2 rows fits 80 KB at W = 257): a 48-channel expand as a plain GEMM + dw_conv_k stride 2 at 33x257; "
          "a wide, short frame"),
    DCase("deeplab-65x337", 65, 337, 1, 4107, 8, 5, None, True, _runs((3, 3, (16, 3, 6)), (6, 6, (24, 17, 1)), (9, 9, (24, 9, 1)), (12, 48, (32, 9, 1))), (), True, 58, 0,
          "head0_band_rows takes its second loop (W = 337 .. 339 only): one workgroup per CU, <= 156 KB, 5 rows"),
    DCase("deeplab-65x329", 65, 329, 1, 4108, 8, 5, None, False, _runs((3, 3, (16, 3, 6)), (6, 6, (24, 17, 1)), (9, 9, (24, 9, 1)), (12, 48, (32, 9, 1))), (), True, 58, 0,
          "head NOT fused although W < 340: the band's input rows exceed 8 quads per lane"),
    DCase("deeplab-33x33", 33, 33, 1, 4109, 8, 5, None, True, _runs((3, 6, (24, 9, 1)), (9, 9, (24, 5, 1))), tuple(range(12, 49, 3)), True, 58, 0,
          "from the 5x5 level on OH * OW < 64: unfused expand / depthwise; dilation 2 and 4 on a 5x5 map (d = 4: every tap outside except the centre row / column); "
          "dw_col_k's H >= 4 * dh switch to dw_conv_k; GAP over 25 pixels"),
    DCase("deeplab-17x17", 17, 17, 1, 4110, 8, 5, None, True, _runs((3, 3, (24, 5, 1))), tuple(range(6, 49, 3)), True, 58, 0,
          "3x3 maps: dilation larger than the input"),
    DCase("deeplab-9x9", 9, 9, 1, 4111, 8, 5, None, False, (), EXPANDS, False, 59, 58,
          "a DeepLab-family graph as a whole-network frame program (kernels_frame.hip): concat, global pool, align-corners resize 1x1 -> 2x2 and dilated depthwise "
          "on 2x2 as micro-ops; concat and pool branch not folded"),
    DCase("deeplab-wide-193x257", 193, 257, 2, 4112, 10, 10, ROWS_DIFFERENT, False,
          _runs((3, 3, (16, 4, 13)), (6, 6, (16, 17, 3)), (9, 9, (16, 9, 3)), (12, 39, (32, 25, 1))), (42, 45, 48), False, 58, 0,
          "every channel count x 2 (MobileNetV2's own): conv_k with two channel tiles, K tail Cin = 24, exact 2- and 3-slab K; plain GEMMs with K up to 960 and "
          "N = 960, 320, 160; the 256 -> 256 GEMM that carries the folded pool branch as out_bias, outside the chain; 256 -> 21 through a GEMM's half-empty column "
          "tile; dw_col_k / dw_conv_k at d = 4 on 960 channels; M >= 8192 at the 1/8 level (25x33 = 825 pixels per frame) at 10 of 10 streams"),
]
BY_NAME = {c.name: c for c in CASES}
HOST_PROOF = ["deeplab-33x33", "deeplab-65x97", "deeplab-9x9"]          # the three smallest graphs: the host proof of the bar (tests/test_f64_forced_host.py)


def pairs_of(case):
    """{expand step: (CH, BH, bands)} of a case's runs"""
    out = {}
    for first, last, g in case.pairs:
        for s in EXPANDS:
            if first <= s <= last:
                out[s] = g
    return out


_STEP = r"^\s*(\d+) (\w+)\s+\S.*?\s+in (\d+)x(\d+)x(\d+) -> out (\d+)x(\d+)x(\d+) "
_FUSED = r"\^ fused with step (\d+) \(expand \+ depthwise in one kernel: (\d+) channels x (\d+) rows per workgroup, (\d+) band"


def plan_facts(d):
    """what a test reads from a DeepLab plan text (bsx_model_describe or a context's plan)"""
    kinds, pairs, last = {}, {}, None
    for line in d.split("\n"):
        m = re.match(_STEP, line)
        if m:
            last = int(m.group(1))
            kinds[last] = m.group(2)
        m = re.search(_FUSED, line)
        if m:
            assert int(m.group(1)) == last + 1, line
            pairs[last] = (int(m.group(2)), int(m.group(3)), int(m.group(4)))
    head = "^ fused with steps 1 and 2" in d
    unfused = tuple(i for i in sorted(kinds) if kinds[i] == "pwconv" and kinds.get(i + 1) == "dwconv" and i not in pairs)
    steps, prog = re.search(r"^ops=\d+ nodes=\d+ steps=(\d+) ", d, re.M), re.search(r"^program micro-ops=(\d+) ", d, re.M)      # (bsx_model_describe's lines only)
    return {"steps": int(steps.group(1)) if steps else None, "micro_ops": int(prog.group(1)) if prog else None, "head_fused": head,
            "pairs": pairs, "unfused": unfused, "chain": re.search(r"\^ chained with steps \d+ and \d+ at 8192 pixels and more", d) is not None}


def model_file(case, directory):
    """path of the case's model inside `directory`, written on first use (seeded: the same bytes every time)"""
    from backscrub_amd import tflite_io
    from tools import make_synthetic_model as S
    path = os.path.join(str(directory), S.sized_file_name(FAMILY, case.H, case.W, case.width))
    if not os.path.exists(path):
        tflite_io.save(S.build_sized(FAMILY, case.H, case.W, case.seed, case.width), path)
    return path
