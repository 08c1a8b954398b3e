"""The frame-geometry audit on a box without a GPU (docs/design/02b-geometry-audit.md): tools/step_trace.py drives libbsx.so's real host code under
tests/hip_stub/libhipstub.so for every row of tests/geometry_cases.py.  Asserted:
  * every row takes the route written next to it — tile or generic mask kernel, one launch / the whole-row instantiation / that plus a partial-row launch, the
    tile classifier or its memset, fused or separate blend, which outside_roi_* kernel each flag route runs, and how YUYV frames reach prep — read from the
    kernel names, template arguments and grids of the launch trace;
  * every route class of the audit is taken by at least one row (the coverage claim, checked);
  * the library's ROI rectangles equal the oracle's (the reference's float truncation) over a sweep of capture sizes for all four models, and the library
    refuses no size the oracle accepts."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import geometry_cases as gc

sys.path.insert(0, ROOT)
KTW, KTH, MAX_SRC_ROWS, SRC_BLOCK_BYTES = 128, 32, 40, 36 * 132


@pytest.fixture(scope="module")
def traces():
    from backscrub_amd import build
    build.build()
    from tools import step_trace
    d = step_trace.trace_all(False, 3, sizes=[r[:4] for r in gc.ROWS], brief=True)
    assert len(d) == len(gc.ROWS)
    return {gc.row_id(r): d["%s %dx%d -" % r[:3]] for r in gc.ROWS}


def _mode(sw, sh, dw, dh):
    """make_resize_tab's table mode: 1 copy, 2 exact 2x2 area mean, 0 linear"""
    return 1 if (sw, sh) == (dw, dh) else (2 if (sw, sh) == (2 * dw, 2 * dh) else 0)


def _ofs(s, d):
    """source offsets of cv::resize(INTER_LINEAR), as make_resize_tab: floor of the float32 source coordinate"""
    f = ((np.arange(d) + 0.5) * (1.0 / (d / s)) - 0.5).astype(np.float32)
    return np.floor(f).astype(np.int64)


def _tile_source_block(sw, sh, dw, dh):
    """(rows, columns) of the largest source block a 128 x 32 mask tile with its blur apron reads: mask_tile_fits restated"""
    xo, yo = np.clip(_ofs(sw, dw), 0, sw - 1), _ofs(sh, dh)
    rows = max(int(np.clip(yo[min(t + KTH + 1, dh - 1)] + 1, 0, sh - 1) - np.clip(yo[max(t - 2, 0)], 0, sh - 1) + 1) for t in range(0, dh, KTH))
    cols = max(int(min(xo[min(t + KTW + 1, dw - 1)] + 1, sw - 1) - xo[max(t - 2, 0)] + 1) for t in range(0, dw, KTW))
    return rows, cols


def _bodies(row, info):
    """what the trace cannot show, restated from the context's own rectangles: the table modes and the sampling body of the generic mask kernel"""
    (rx, _, rw, rh), (_, _, qw, qh) = info["roi"], info["in_roi"]
    down, up = _mode(rw, rh, qw, qh), _mode(qw, qh, rw, rh)
    narrow = (row[1] - rx) * 3 < 8
    body = {1: "copy", 2: "area"}.get(up)
    if body is None:
        rows, cols = _tile_source_block(qw, qh, rw, rh)
        fits = rows <= MAX_SRC_ROWS and rows * cols <= SRC_BLOCK_BYTES
        body = "tile" if fits else ("lds rows" if rows <= MAX_SRC_ROWS else "per pixel")
    return dict(down=down, up=up, narrow=narrow, body=body)


@pytest.mark.parametrize("row", gc.ROWS, ids=gc.row_id)
def test_row_takes_its_route(traces, row):
    calls = traces[gc.row_id(row)]
    W, H, n = row[1], row[2], row[3]
    route = row[5]
    assert gc.observed_route(calls, W, H) == route
    b = _bodies(row, calls["_info"])
    assert (route["prep"] == "general") == (b["down"] != 0 or b["narrow"]), b
    assert (route["mask"] == "tile") == (b["body"] == "tile"), b                 # the restated fit rule agrees with the launch the library made
    assert route["stage4"] == (b["down"] == 0 and W % 2 == 0 and calls["_info"]["roi"][0] % 2 == 0 and (W - calls["_info"]["roi"][0]) * 2 >= 8)
    rx, ry, rw, rh = calls["_info"]["roi"]
    ntx, nty = (rw + KTW - 1) // KTW, (rh + KTH - 1) // KTH
    step = gc.kernels(calls["step"]["trace"])
    masks = [k for k in step if k[0] in ("mask_tile_k", "mask_upscale_blur_k")]
    # grids: one workgroup per tile and stream; the whole rows and the partial row split them
    if route["rows"] == "whole+partial":
        assert [k[2] for k in masks] == [(ntx * (rh // KTH) * n, 1, 1), (ntx * n, 1, 1)] and rh % KTH
    else:
        assert [k[2] for k in masks] == [(ntx * nty * n, 1, 1)]
        assert route["rows"] != "whole" or (rh % KTH == 0 and rw % KTW == 0)
    cls = [k for k in step if k[0] in ("tile_class_k", "memset")]
    if route["cls"] == "kernel":
        assert [k[2] for k in cls] == [(n, 1, 1)] and ntx <= 16
    elif route["cls"] == "memset":
        assert [k[2] for k in cls] == [ntx * nty * n] and ntx > 16
    else:
        assert cls == []
    # the outside-ROI kernel of every flag route (fused routes only: the separate blend covers the whole frame)
    for call, kernel in (("step", "outside_roi_copy_k"), ("ex_in_place", "outside_roi_copy_k"), ("ex_flip_h", "outside_roi_flip_k"), ("ex_yuyv", "outside_roi_yuyv_k"),
                         ("ex_yuyv_flip", "outside_roi_flip_k"), ("ex_no_mask_flip_v", "outside_roi_flip_k"), ("mixed", "outside_roi_mixed_k")):
        c = calls[call]
        if c["rc"] != 0:
            assert (call == "mixed" and not route["fused"]) or (W % 2 and "yuyv" in call), (call, c["error"])
            assert c["trace"] == []
            continue
        got = [k[0] for k in gc.kernels(c["trace"]) if k[0].startswith("outside_roi")]
        assert got == ([kernel] if route["outside"] and route["fused"] else []), (call, got)
    assert route["mixed"] == route["fused"]
    if W % 2:                                                                    # odd width: every YUYV form is refused with its reason, nothing enqueued
        for call in ("ex_yuyv", "ex_yuyv_flip", "ex_yuyv_in"):
            assert calls[call]["rc"] == -1 and "even" in calls[call]["error"] and calls[call]["trace"] == []
        assert calls["stage_4"]["rc"] == -1 and calls["stage_4"]["trace"] == []
    for call in ("step", "ex_flip_h", "ex_no_mask_flip_v", "ex_in_place", "stage_0", "stage_3"):
        assert calls[call]["rc"] == 0, (call, calls[call]["error"])


def test_every_route_class_is_taken(traces):
    routes = {gc.row_id(r): gc.observed_route(traces[gc.row_id(r)], r[1], r[2]) for r in gc.ROWS}
    for name, pred in gc.ROUTE_CLASSES:
        assert any(pred(r) for r in routes.values()), "no row takes: %s" % name
    bodies = {gc.row_id(r): _bodies(r, traces[gc.row_id(r)]["_info"]) for r in gc.ROWS}
    for want in ("tile", "lds rows", "per pixel", "copy", "area"):                 # the tile kernel and the generic kernel's sampling bodies
        assert any(b["body"] == want for b in bodies.values()), "no row samples by: %s" % want
    for down in (0, 1, 2):
        assert any(b["down"] == down for b in bodies.values()), "no row preps with table mode %d" % down
    assert any(b["narrow"] for b in bodies.values())
    # prep up-samples; ROI branch B with a narrow in_roi on a square model; a portrait frame; odd roi.w on a pillarboxed frame; a frame narrower than 4
    infos = {gc.row_id(r): (r, traces[gc.row_id(r)]["_info"]) for r in gc.ROWS}
    assert any(i["roi"][2] < i["in_roi"][2] and b["down"] == 0 for (_, i), b in zip(infos.values(), bodies.values()))
    assert any(r[0] in ("mlkit", "deeplab") and i["in_roi"][0] > 0 for r, i in infos.values())
    assert any(r[2] > r[1] for r, _ in infos.values())
    assert any(i["roi"][0] > 0 and i["roi"][2] % 2 for _, i in infos.values())
    assert any(r[1] < 4 for r, _ in infos.values())
    assert infos["lite-1920x1080"][1]["roi"] == [60, 0, 1799, 1080] and infos["full-2056x1160"][1]["in_roi"] == [0, 0, 255, 144]


def sweep_sizes():
    """every 7th width of 2..2600 plus every multiple of 64 and its two neighbours, each at 16:9, 4:3, 1:1, 3:4 and 9:16; and the matrix rows"""
    ws = set(range(2, 2601, 7))
    for m in range(64, 2601, 64):
        ws.update(w for w in (m - 1, m, m + 1) if 2 <= w <= 2600)
    sizes = set()
    for w in sorted(ws):
        for h in (round(w * 9 / 16), round(w * 3 / 4), w, round(w * 4 / 3), round(w * 16 / 9)):
            sizes.add((w, max(int(h), 1)))
    sizes.update((r[1], r[2]) for r in gc.ROWS)
    return sorted(sizes)


@pytest.mark.parametrize("key", ["lite", "full", "mlkit", "deeplab"])
def test_roi_rectangles_equal_the_oracles_over_a_sweep(oracle, key, tmp_path):
    from backscrub_amd import build
    build.build()
    from tools import step_trace
    sizes = sweep_sizes()
    path = step_trace.model_file(key)
    # the library's side in four child processes under the interposer (a context costs 10-30 ms of host work); the oracle's side meanwhile, here
    procs = []
    for k in range(4):
        (tmp_path / ("sizes%d.json" % k)).write_text(json.dumps(sizes[k::4]))
        env = dict(os.environ, LD_PRELOAD=step_trace.build_stub(), BSX_STUB_LOG=str(tmp_path / ("hip%d.log" % k)), BSX_STUB_NDEV="1", BSX_LIBRARY=build.LIB)
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tools", "step_trace.py"), "--roi-sweep", path, str(tmp_path / ("sizes%d.json" % k))], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    want = {}
    for W, H in sizes:
        try:
            oc = oracle.Ctx(path, W, H)
        except RuntimeError:
            continue                                                            # the oracle refuses the size: the library may refuse it too, or not
        want[(W, H)] = (list(oc.roidim), list(oc.in_roidim))
        oc.close()
    got = []
    for p in procs:
        out, err = p.communicate(timeout=1800)
        assert p.returncode == 0, err[-3000:]
        got += json.loads([l for l in out.splitlines() if l.startswith("[")][-1])
    assert len(got) == len(sizes) > 2000
    accepted = 0
    for W, H, roi, in_roi in got:
        if (W, H) not in want:
            continue
        assert roi is not None, "%s %dx%d: the oracle accepts the size (%s), the library refuses it" % (key, W, H, want[(W, H)])
        assert (roi, in_roi) == want[(W, H)], "%s %dx%d" % (key, W, H)
        accepted += 1
    assert accepted > 0.95 * len(sizes), (accepted, len(sizes))                  # the sweep is not vacuous: the oracle accepts nearly every size
