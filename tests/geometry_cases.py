"""The frame-geometry matrix of the image kernels (docs/design/02b-geometry-audit.md): plain data and a few helpers, shared by tests/test_geometry_host.py (which
proves from launch traces that every row takes the route written next to it) and tests/test_gpu_geometry.py (which compares every row's bytes with the oracle).

The frame size and the model's input shape pick, per context: the ROI branch (pillarboxed frame / pillarboxed model canvas), the table mode of the two resizes
(0 linear, 1 copy, 2 exact 2x2 area mean), the LDS tile kernel or the generic per-pixel mask kernel, whether mask and blend fuse, the whole-row instantiation of the
tile kernel, the tile classifier or its memset, and how YUYV input reaches prep.  A row's `route` is what the library was OBSERVED to do under the HIP interposer
(tools/step_trace.py); the host test fails when the library stops doing it, so a row cannot silently stop covering what it is there for.

route fields:
  prep      "linear"  prep_fused_k<.., LINEAR = true>: the table-driven 8-byte tap window
            "general" prep_fused_k<.., LINEAR = false>: sample_linear per pixel (copy, 2x2 area mean, or a row narrower than the 8-byte window)
  mask      "tile" mask_tile_k | "generic" mask_upscale_blur_k
  fused     the plain step composites inside the mask kernel (no separate blend launch)
  rows      launches of the mask kernel in the plain step: "one" | "whole" (the WH instantiation alone) | "whole+partial" (WH plus the edge-testing one for the last tile row)
  cls       "kernel" tile_class_k | "memset" (out of the classifier's range) | "none" (the generic kernel has no classes)
  outside   the ROI is not the whole frame: the fused routes launch an outside_roi_* kernel (copy / flip / yuyv / mixed, by the call's flags)
  yuyv_in   the step with YUYV frames: "prep" the prep kernel reads them | "convert" yuyv_to_bgr_k first (prep cannot, or the separate blend needs BGR) | "refused" (odd width)
  stage4    prep_yuyv_fusable: the stage entry runs prep on YUYV frames (true on every "prep" row, and on unfused rows whose step converts for the blend's sake)
  mixed     bsx_step_batch_mixed accepts the geometry (the fused routes only)
"""
import re

LAUNCH = ("hipLaunchKernel", "hipModuleLaunchKernel")


def R(prep, mask, fused, rows, cls, outside, yuyv_in, stage4=None):
    return dict(prep=prep, mask=mask, fused=fused, rows=rows, cls=cls, outside=outside, yuyv_in=yuyv_in, mixed=fused, stage4=(yuyv_in == "prep") if stage4 is None else stage4)


# (model, W, H, streams, what the row is there for, the observed route)
ROWS = [
    ("lite", 80, 48, 3, "prep up-samples 2x; mask table mode 2 (exact 2x2 area mean); fusable widths: the generic kernel with the blend fused",
     R("linear", "generic", True, "one", "none", False, "prep")),
    ("full", 128, 72, 3, "the same on segm_full; roi.w == 128: one whole tile column, in the generic kernel",
     R("linear", "generic", True, "one", "none", False, "prep")),
    ("mlkit", 128, 128, 3, "mask mode 2 on a square model (ROI branch B with the whole canvas)",
     R("linear", "generic", True, "one", "none", False, "prep")),
    ("lite", 320, 192, 3, "prep mode 2 (exact 2x2 area mean); YUYV input must take the convert-first route",
     R("general", "tile", True, "one", "kernel", False, "convert")),
    ("full", 512, 288, 3, "prep mode 2; fused, whole tile rows only (288 = 9 x 32, 512 = 4 x 128)",
     R("general", "tile", True, "whole", "kernel", False, "convert")),
    ("mlkit", 512, 512, 3, "prep mode 2; mask exactly 2x linear",
     R("general", "tile", True, "whole", "kernel", False, "convert")),
    ("deeplab", 514, 514, 3, "prep mode 2 with W % 4 == 2: unfused",
     R("general", "tile", False, "one", "kernel", False, "convert")),
    ("mlkit", 256, 256, 3, "copy both ways (table mode 1) on a square model",
     R("general", "generic", True, "one", "none", False, "convert")),
    ("deeplab", 257, 257, 3, "copy both ways, odd width: unfused",
     R("general", "generic", False, "one", "none", False, "refused")),
    ("lite", 132, 100, 3, "the tile fits with 36 source rows x 125 columns (4500 of 4752 bytes)",
     R("linear", "tile", True, "one", "kernel", False, "prep")),
    ("mlkit", 512, 288, 3, "roi = (112,0,288,288); the tile fits with 34 x 119",
     R("linear", "tile", True, "one", "kernel", True, "prep")),
    ("deeplab", 322, 242, 3, "40 source rows (equal to the limit) x 139 columns: fails the area limit only",
     R("linear", "generic", False, "one", "none", True, "convert", True)),
    ("lite", 108, 88, 3, "the tile fits with exactly 40 source rows (the row limit itself) x 117 columns (4680 of 4752 bytes)",
     R("linear", "tile", True, "one", "kernel", False, "prep")),
    ("full", 128, 128, 3, "42 source rows: fails the row limit; widths fusable",
     R("linear", "generic", True, "one", "none", False, "prep")),
    ("mlkit", 160, 96, 3, "the mask 'up-scale' is a 2.67x down-scale: the generic kernel's per-pixel linear body",
     R("linear", "generic", True, "one", "none", True, "prep")),
    ("lite", 48, 64, 3, "portrait; generic",
     R("linear", "generic", True, "one", "none", False, "prep")),
    ("lite", 360, 640, 3, "portrait; in_roi = (53,0,54,96); tile kernel",
     R("linear", "tile", True, "one", "kernel", False, "prep")),
    ("full", 96, 160, 3, "portrait; in_roi = (84,0,86,144); the tile fits with 34 rows",
     R("linear", "tile", True, "one", "kernel", False, "prep")),
    ("mlkit", 240, 320, 3, "ROI branch B on a square model; in_roi = (32,0,192,256)",
     R("linear", "tile", True, "one", "kernel", False, "prep")),
    ("deeplab", 96, 160, 3, "branch B; in_roi = (51,0,154,257); generic",
     R("linear", "generic", True, "one", "none", False, "prep")),
    ("lite", 512, 288, 3, "roi = (16,0,479,288): odd roi.w, unfused, ROI branch A",
     R("linear", "tile", False, "one", "kernel", True, "convert", True)),
    ("lite", 1920, 1080, 2, "roi = (60,0,1799,1080): the most common camera, off the fused route (float truncation)",
     R("linear", "tile", False, "one", "kernel", True, "convert", True)),
    ("lite", 16, 8, 3, "roi = (1,0,13,8): odd roi.x with W % 4 == 0; YUYV input not fusable",
     R("linear", "generic", False, "one", "none", True, "convert")),
    ("mlkit", 16, 12, 3, "roi = (2,0,12,12): YUYV prep fusable, blend not",
     R("linear", "generic", False, "one", "none", True, "convert", True)),
    ("full", 2048, 1152, 2, "ntx = 16: the classifier's last size in range; the WH instantiation (16 tile columns, 36 whole tile rows)",
     R("linear", "tile", True, "whole", "kernel", False, "prep")),
    ("full", 2056, 1160, 2, "ntx = 17: the classifier replaced by the memset; in_roi.w = 255 (float truncation)",
     R("linear", "tile", True, "one", "memset", False, "prep")),
    # the degenerate rows stay last: frames narrower than the 4-pixel groups every fused route works in
    ("lite", 2, 2, 3, "prep's narrow-row body ((W - roi.x) * 3 < 8); YUYV in / out legal (W even) but no fused route applies",
     R("general", "generic", False, "one", "none", False, "convert")),
    ("lite", 3, 5, 3, "odd width below 4: the YUYV forms must be refused",
     R("linear", "generic", False, "one", "none", False, "refused")),
]
# the row above was listed for "WH plus a partial last row", but 1152 = 36 x 32 has no partial row: this one has (1160 = 36.25 x 32), at the same 16 tile columns
ROWS.insert(-3, ("full", 2048, 1160, 2, "ntx = 16 and the WH instantiation plus a second launch for the partial last tile row; in_roi.w = 254",
                 R("linear", "tile", True, "whole+partial", "kernel", False, "prep")))

# every route class the audit claims: (name, predicate on a row's route) — the host test requires at least one row per class
ROUTE_CLASSES = [
    ("tile kernel", lambda r: r["mask"] == "tile"),
    ("generic kernel", lambda r: r["mask"] == "generic"),
    ("generic kernel, fused", lambda r: r["mask"] == "generic" and r["fused"]),
    ("generic kernel, unfused", lambda r: r["mask"] == "generic" and not r["fused"]),
    ("tile kernel, fused", lambda r: r["mask"] == "tile" and r["fused"]),
    ("tile kernel, unfused", lambda r: r["mask"] == "tile" and not r["fused"]),
    ("whole tile rows only", lambda r: r["rows"] == "whole"),
    ("whole tile rows plus a partial row", lambda r: r["rows"] == "whole+partial"),
    ("classifier kernel", lambda r: r["cls"] == "kernel"),
    ("classifier memset", lambda r: r["cls"] == "memset"),
    ("outside-ROI kernel, fused", lambda r: r["outside"] and r["fused"]),
    ("pillarboxed frame, unfused", lambda r: r["outside"] and not r["fused"]),
    ("prep linear", lambda r: r["prep"] == "linear"),
    ("prep general", lambda r: r["prep"] == "general"),
    ("YUYV read by prep", lambda r: r["yuyv_in"] == "prep"),
    ("YUYV converted first", lambda r: r["yuyv_in"] == "convert"),
    ("YUYV refused", lambda r: r["yuyv_in"] == "refused"),
]


def row_id(row):
    return "%s-%dx%d" % row[:3]


def kernels(trace):
    """trace entries of one call → [(kernel name, [template arguments], (gx, gy, gz))] for the launches, ("memset", [], bytes) for a hipMemsetAsync"""
    out = []
    for l in trace:
        f = l.split()
        if f[1] == "hipMemsetAsync":
            out.append(("memset", [], int(f[2][2:])))
        elif f[1] in LAUNCH:
            m = re.match(r"_ZN3bsx(?:12_GLOBAL__N_1)?(\d+)", f[2])
            if m:
                k = int(m.group(1))
                name, rest = f[2][m.end():m.end() + k], f[2][m.end() + k:]
                targs = [int(v) for v in re.findall(r"L[bi](\d+)E", rest[:rest.index("EE") + 1])] if rest.startswith("I") else []
            else:
                name, targs = f[2], []
            out.append((name, targs, tuple(int(v) for v in f[3][2:].split(","))))
    return out


IMAGE_KERNELS = ("prep_fused_k", "mask_tile_k", "mask_upscale_blur_k", "tile_class_k", "blend4x4_k", "blend1_k", "outside_roi_copy_k", "outside_roi_flip_k",
                 "outside_roi_yuyv_k", "outside_roi_mixed_k", "yuyv_to_bgr_k", "yuyv_k", "flip_bgr_k", "memset")


def observed_route(calls, W, H):
    """the route of one context from the brief drive of tools/step_trace.py (step, flip_h, yuyv, yuyv_in, mixed, stage_3)"""
    step = [k for k in kernels(calls["step"]["trace"]) if k[0] in IMAGE_KERNELS]
    names = [k[0] for k in step]
    prep = [k for k in step if k[0] == "prep_fused_k"]
    assert len(prep) == 1, names
    masks = [k for k in step if k[0] in ("mask_tile_k", "mask_upscale_blur_k")]
    assert masks and len({k[0] for k in masks}) == 1, names
    tile = masks[0][0] == "mask_tile_k"
    blend = [k for k in step if k[0] in ("blend4x4_k", "blend1_k")]
    fused = all(k[1][0] == 1 for k in masks)                     # BLEND
    assert fused != bool(blend), names                           # a composite is made exactly once
    wh = [k[1][3] for k in masks] if tile else [0]
    rows = {(0,): "one", (1,): "whole", (1, 0): "whole+partial"}[tuple(wh)]
    cls = "kernel" if "tile_class_k" in names else ("memset" if "memset" in names else "none")
    outside = [k[0] for k in step if k[0].startswith("outside_roi")]
    stage3 = [k[0] for k in kernels(calls["stage_3"]["trace"])]
    assert [k for k in stage3 if k.startswith("mask_")] == [masks[0][0]], stage3      # stage 3 runs the same mask kernel, stand-alone
    assert (("tile_class_k" in stage3) and "kernel" or ("memset" in stage3) and "memset" or "none") == cls
    yin = calls["ex_yuyv_in"]
    if yin["rc"] != 0:
        yuyv_in = "refused"
    else:
        ky = kernels(yin["trace"])
        conv = any(k[0] == "yuyv_to_bgr_k" for k in ky)
        pk = [k for k in ky if k[0] == "prep_fused_k"][0]
        assert conv != (pk[1][2] == 1), ky                        # YIN instantiation of prep, or the conversion in front of the BGR one
        yuyv_in = "convert" if conv else "prep"
    pillar = calls["_info"]["roi"] != [0, 0, W, H]
    assert bool(outside) == (pillar and fused), names                # unfused: the blend covers the whole frame, the mask is 255 outside the ROI
    return dict(prep="linear" if prep[0][1][1] else "general", mask="tile" if tile else "generic", fused=fused, rows=rows, cls=cls,
                outside=pillar, yuyv_in=yuyv_in, mixed=calls["mixed"]["rc"] == 0, stage4=calls["stage_4"]["rc"] == 0)


def mask_of_state(oracle, state, info, W, H):
    """the full-resolution mask a model-resolution temporal state implies: cv::resize + cv::blur(5x5) of its in_roi into the ROI of a 255-filled frame
    (lib/libbackscrub.cc:367-371) — by the oracle's own resize and blur; `info`: a context's info (roi, in_roi)"""
    import numpy as np
    rx, ry, rw, rh = info["roi"]
    qx, qy, qw, qh = info["in_roi"]
    want = np.full((H, W), 255, np.uint8)
    want[ry:ry + rh, rx:rx + rw] = oracle.blur5(oracle.resize_linear(np.ascontiguousarray(state[qy:qy + qh, qx:qx + qw]), rw, rh))
    return want
