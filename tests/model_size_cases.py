"""Meet-family and MLKit graphs at other network input sizes than the three shipped ones: the case table of the model-size audit and the model builder.

Every shipped shape (96x160, 144x256, 256x256) is a multiple of 32 in both axes, so every stride-2 SAME convolution has no top / left pad, every tensor of the middle
program has even extents, every tile grid has several tiles of full size, "lite" means k3's per-frame form and "full / MLKit" its tile form, and every plan is segmented.
The cases below are the smallest models that leave each of those habits (docs/design/02a-layer-audit.md, "Other model sizes").  Per case the table states what the
planner's text (bsx_model_describe) must say for the case to keep its purpose: tests/test_model_size_cases.py asserts it without a GPU, tests/test_gpu_model_sizes.py
runs the audit.

No GPU and no library at import time; models are written on demand into a directory the caller supplies (nothing is committed)."""
import collections
import os

Case = collections.namedtuple("Case", "name family H W seed segmented tiles k3 steps micro_ops middle reaches refused", defaults=(None,))
# tiles: {"head" | "k2" | "k3" | "tail": (TR, TC, tiles_y, tiles_x)} of the four `segment … tile` lines
# k3:    ("frame", LDS bytes) — the per-frame form — or ("tiles", reason, the LDS bytes the per-frame form would take)
# middle: None = a specialised middle kernel exists; else the reason the plan text gives for "specialised middle kernel: none"
# refused: None, or the text with which bsx_new refuses a context of the model at every frame size (the model still loads, plans and runs in the oracle)
OUTSIDE = "the shape is outside the per-frame kernel's limits"
NO_FIT = "a frame does not fit the LDS"
IN_IO = "operand in the network input / output buffer"
NO_ROI = "frame/model geometry yields an empty or out-of-range ROI"


def _t(head, k2, k3, tail):
    return {"head": head, "k2": k2, "k3": k3, "tail": tail}


CASES = [
    Case("lite-16x16", "lite", 16, 16, 4000, True, _t((4, 4, 1, 1), (2, 2, 1, 1), (4, 4, 1, 1), (8, 8, 1, 1)), ("frame", 23872), 74, 39,
         "micro-op kind 1 has no specialised body",
         "1x1 tile grids, every tile smaller than its target; c0 2x2, middle tensors 1x1: 5x5 depthwise larger than its input"),
    Case("lite-32x48", "lite", 32, 48, 4001, True, _t((4, 12, 2, 1), (4, 6, 1, 1), (8, 12, 1, 1), (16, 12, 1, 2)), ("frame", 29248), 68, 33, None,
         "grids one tile wide and one tile high"),
    Case("lite-95x159", "lite", 95, 159, 4002, True, _t((4, 14, 6, 3), (4, 7, 3, 3), (12, 14, 2, 3), (16, 14, 3, 6)), ("frame", 118144), 68, 33, None,
         "stem_pt = stem_pl = 1: the only asymmetric pad a segmented plan can have; network output 96x160 is not the input's size"),
    Case("lite-104x168", "lite", 104, 168, 4003, True, _t((4, 14, 7, 3), (4, 7, 4, 3), (13, 14, 2, 3), (18, 14, 3, 6)), ("tiles", OUTSIDE, 126400), 68, 33, None,
         "c0 13x21: odd extents through the middle program (5x5 stride-2 depthwise with pad_t = 2); partial last tiles in all four kernels; tile form on a lite graph"),
    Case("lite-160x96", "lite", 160, 96, 4004, True, _t((4, 12, 10, 2), (4, 6, 5, 2), (14, 12, 3, 2), (16, 12, 5, 4)), ("tiles", OUTSIDE, 124288), 68, 33, None,
         "portrait: more row tiles than column tiles, k3 TR = 14"),
    Case("mlkit-128x128", "mlkit", 128, 128, 4005, True, _t((4, 11, 8, 3), (4, 6, 4, 3), (16, 11, 2, 3), (16, 13, 4, 5)), ("tiles", OUTSIDE, 143744), 68, 33, None,
         "the per-frame form refused with LDS to spare"),
    Case("mlkit-264x248", "mlkit", 264, 248, 4006, True, _t((4, 13, 17, 5), (4, 7, 9, 5), (14, 13, 5, 5), (17, 14, 8, 9)), ("tiles", NO_FIT, 457216), 68, 33, None,
         "odd tile counts, tail TR = 17, c0 33x31"),
    Case("lite-100x164", "lite", 100, 164, 4007, False, None, None, 68, 47, IN_IO,
         "not segmented (lo2 13x21 -> B 25x41: non-uniform resize weights): whole-network program; pad = 1 in the head's and k2's depthwise as micro-ops; 25x41, 13x21, 7x11"),
    Case("lite-36x52", "lite", 36, 52, 4008, False, None, None, 68, 49, IN_IO,
         "not segmented, small: 9x13, 5x7, 3x4"),
    Case("lite-8x8", "lite", 8, 8, 4009, False, None, None, 75, 56, IN_IO,
         "not segmented; another step list: rewrites that do not apply at 1x1 extents"),
    Case("lite-97x161", "lite", 97, 161, 4010, False, None, None, 68, 49, IN_IO,
         "SAME-cropped transpose convolution (A 49x81 -> 97x161) as a micro-op of its own: no fused tail; every stride-2 pad asymmetric"),
    Case("mlkit-250x246", "mlkit", 250, 246, 4011, False, None, None, 68, 49, IN_IO,
         "SAME-cropped transpose convolution (A 125x123 -> 249x245); network output SMALLER than the input: the part of the input a frame maps to spans one whole axis "
         "of the input (250 rows or 246 columns) and does not exist in the 249x245 output, at any frame size — as in the reference, whose ofinal(in_roidim) is out of "
         "range — so bsx_new refuses the context", NO_ROI),
    # not in the issue's table: the MLKit graph whose cropped output IS its input's size, so that the cropped transpose convolution with one sigmoid channel runs
    Case("mlkit-249x245", "mlkit", 249, 245, 4012, False, None, None, 68, 49, IN_IO,
         "SAME-cropped transpose convolution of the MLKit form (A 125x123 -> 249x245, one channel, logistic) as a micro-op of its own"),
]
BY_NAME = {c.name: c for c in CASES}
SEGMENTED = [c for c in CASES if c.segmented]
STEM_PAD = {"lite-95x159": 1}          # SegHead.stem_pt = stem_pl of the segmented cases (default 0); dw_pt = dw_pl = 0 in all of them

# Forced tile geometries on the smallest segmented shapes: extra environments of the DEBUG library (the release library does not read them)
FORCED = [
    ("lite-32x48", "many small tiles", {"BSX_SEG_TILES": "2,5,2,3,3,5,5,5"}),
    ("lite-32x48", "k3 in tiles", {"BSX_K3_TILES": "1"}),
]
FORCED_KNOBS = ("BSX_SEG_TILES", "BSX_K3_TILES")


def model_file(case, directory):
    """path of the case's model inside `directory`, written on first use (seeded: the same bytes every time)"""
    from backscrub_amd import tflite_io
    from tools import make_synthetic_model as S
    path = os.path.join(str(directory), S.sized_file_name(case.family, case.H, case.W))
    if not os.path.exists(path):
        tflite_io.save(S.build_sized(case.family, case.H, case.W, case.seed), path)
    return path
