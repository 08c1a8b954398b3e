"""The fleets of tests/geoms_route_cases.py, without the library: every matrix-derived class is one bsx_new_geoms takes, the rectangles written next to each class
are what the reference's float arithmetic gives, and each fleet holds the classes its purpose names (tests/test_gpu_geoms_routes.py steps them on the GPU)."""
import re

import numpy as np
import pytest

import geometry_cases as gc
import geoms_route_cases as rc

ALL = [(name, i) for name in rc.FLEETS for i in range(len(rc.FLEETS[name]["classes"]))]


def _id(p):
    c = rc.FLEETS[p[0]]["classes"][p[1]]
    return "%s-%dx%d" % ((p[0],) + c["size"])


def capture_rois(inW, inH, W, H):
    """capture_rois of bsx_api.hip (lib/libbackscrub.cc:230-246) in float32, every intermediate rounded as the C expression rounds it, truncated to int"""
    f = np.float32
    ratio, frameratio = f(inH) / f(inW), f(H) / f(W)
    if frameratio < ratio:
        return (int((f(W) - f(H) / ratio) / f(2)), 0, int(f(H) / ratio), H), (0, 0, inW, inH)
    return (0, 0, W, H), (int((f(inW) - f(inH) / frameratio) / f(2)), 0, int(f(inH) / frameratio), inH)


@pytest.mark.parametrize("p", ALL, ids=_id)
def test_matrix_classes_are_fused_tile_rows(p):
    """bsx_new_geoms takes a class only on the fused tile route: the row a class names must have been observed there"""
    fleet, c = rc.FLEETS[p[0]], rc.FLEETS[p[0]]["classes"][p[1]]
    row = rc.matrix_row(c)
    if row is None:
        return
    key, W, H, _n, _text, route = row
    assert key == fleet["model"] and (W, H) == c["size"]
    assert route["mask"] == "tile" and route["fused"], "%s is not a fused tile row: %s" % (c["row"], route)
    assert (route["prep"] == "general") == (c["down"] == 2)
    assert route["outside"] == (c["roi"] != (0, 0, W, H))
    assert (route["cls"] == "memset") == (c["tiles"][0] > rc.CLS_MAX_TX)
    assert (route["yuyv_in"] == "prep") == rc.yuyv_in_admitted(c)


@pytest.mark.parametrize("p", ALL, ids=_id)
def test_rois_are_what_the_float_arithmetic_gives(p):
    fleet, c = rc.FLEETS[p[0]], rc.FLEETS[p[0]]["classes"][p[1]]
    inW, inH = rc.MODEL_INPUT[fleet["model"]]
    W, H = c["size"]
    roi, in_roi = capture_rois(inW, inH, W, H)
    assert roi == c["roi"] and in_roi == c["in_roi"], "%dx%d: computed %s %s, written %s %s" % (W, H, roi, in_roi, c["roi"], c["in_roi"])
    # the fused route's alignment, the table mode of the down-scale (exactly 2x both ways: the area mean) and the tile grid
    assert W % 4 == 0 and roi[0] % 4 == 0 and roi[2] % 4 == 0
    assert c["down"] == (2 if (roi[2], roi[3]) == (2 * in_roi[2], 2 * in_roi[3]) else 0) and (roi[2], roi[3]) != (in_roi[2], in_roi[3])
    assert c["tiles"] == (-(-roi[2] // rc.TILE_W), -(-roi[3] // rc.TILE_H))
    row = rc.matrix_row(c)
    if row is not None:                                  # what the row's own text states about its rectangles
        text = row[4]
        for name, rect in (("roi", roi), ("in_roi", in_roi)):
            m = re.search(r"(?<![\w.])%s = \((\d+),(\d+),(\d+),(\d+)\)" % name, text)
            if m:
                assert tuple(int(v) for v in m.groups()) == rect, "%s: the row states %s = %s" % (c["row"], name, m.group(0))
            m = re.search(r"(?<![\w.])%s\.w = (\d+)" % name, text)
            if m:
                assert int(m.group(1)) == rect[2], "%s: the row states %s" % (c["row"], m.group(0))
        m = re.search(r"ntx = (\d+)", text)
        if m:
            assert int(m.group(1)) == c["tiles"][0]


def test_the_table_of_the_issue():
    """the values the audit was written around, one by one"""
    by = {(rc.FLEETS[n]["model"],) + c["size"]: c for n in rc.STEP_FLEETS for c in rc.FLEETS[n]["classes"]}
    t = lambda c: c["tiles"][0] * c["tiles"][1]
    assert by["lite", 320, 192]["down"] == 2 and by["lite", 320, 192]["in_roi"] == (0, 0, 160, 96)
    assert by["lite", 132, 100]["in_roi"] == (16, 0, 126, 96) and t(by["lite", 132, 100]) == 8
    assert by["lite", 108, 88]["in_roi"] == (21, 0, 117, 96) and t(by["lite", 108, 88]) == 3
    assert by["lite", 360, 640]["in_roi"] == (53, 0, 54, 96) and t(by["lite", 360, 640]) == 60
    assert by["lite", 640, 480]["in_roi"] == (16, 0, 128, 96) == by["lite", 800, 600]["in_roi"]
    assert by["lite", 1280, 720]["roi"] == (40, 0, 1200, 720) and by["lite", 640, 360]["roi"] == (20, 0, 600, 360)
    assert by["full", 512, 288]["down"] == 2 and t(by["full", 512, 288]) == 36
    assert by["full", 96, 160]["in_roi"] == (84, 0, 86, 144) and t(by["full", 96, 160]) == 5
    assert by["full", 2048, 1152]["tiles"] == (16, 36)
    assert by["full", 2048, 1160]["in_roi"][2] == 254 and by["full", 2048, 1160]["tiles"] == (16, 37)
    assert by["full", 2056, 1160]["in_roi"][2] == 255 and by["full", 2056, 1160]["tiles"] == (17, 37)
    assert by["full", 640, 480]["in_roi"] == (32, 0, 192, 144)
    assert by["mlkit", 512, 512]["down"] == 2
    assert by["mlkit", 512, 288]["roi"] == (112, 0, 288, 288) and t(by["mlkit", 512, 288]) == 27
    assert by["mlkit", 240, 320]["in_roi"] == (32, 0, 192, 256)
    assert by["mlkit", 640, 480]["roi"] == (80, 0, 480, 480)


def test_each_fleet_covers_what_it_is_there_for():
    F = {n: f["classes"] for n, f in rc.FLEETS.items()}
    ntx = lambda c: c["tiles"][0]
    tiles = lambda c: c["tiles"][0] * c["tiles"][1]
    pillar = lambda c: c["roi"] != (0, 0) + c["size"]
    portrait = lambda c: c["size"][1] > c["size"][0]
    for name, cl in F.items():
        sizes = [c["size"] for c in cl]
        assert len(set(sizes)) == len(sizes) <= 8 and all(c["n"] >= 1 for c in cl), name
    # across the fleets: the general prep body, the zero-fill of the classifier, and its last size in range
    every = [c for n in rc.STEP_FLEETS for c in F[n]]
    assert any(c["down"] == 2 for c in every) and any(ntx(c) > rc.CLS_MAX_TX for c in every) and any(ntx(c) == rc.CLS_MAX_TX for c in every)
    for name in rc.STEP_FLEETS:
        assert any(c["down"] == 2 for c in F[name]), "%s has no class with the 2x2 area down-scale" % name
        assert all(c["n"] == 2 for c in F[name])
        assert 0 < len([c for c in F[name] if rc.yuyv_in_admitted(c)]) < len(F[name])           # call 8 has admitted classes and a refused one
    # lite8: kMaxGeoms classes; the two fit-boundary rows; a portrait; pillarboxed beside whole-frame classes
    assert len(F["lite8"]) == 8
    assert {(132, 100), (108, 88)} <= {c["size"] for c in F["lite8"]} and any(portrait(c) for c in F["lite8"])
    assert sorted(c["roi"][0] for c in F["lite8"] if pillar(c)) == [20, 40] and sum(not pillar(c) for c in F["lite8"]) == 6
    assert min(tiles(c) for c in F["lite8"]) == 3 and max(tiles(c) for c in F["lite8"]) == 230
    # full6: the classifier's three cases in one launch; a 5-tile class beside 576 / 592 / 629
    assert sorted(tiles(c) for c in F["full6"]) == [5, 36, 75, 576, 592, 629]
    assert [ntx(c) for c in F["full6"] if ntx(c) >= 16] == [16, 16, 17]
    assert [c["size"][1] % rc.TILE_H for c in F["full6"] if ntx(c) == 16] == [0, 8]              # whole tile rows only / a partial last row
    assert any(portrait(c) and tiles(c) == 5 for c in F["full6"])
    # mlkit4: two outside-ROI classes, the branch-B portrait (whole frame on a pillarboxed canvas)
    assert sorted(c["roi"][0] for c in F["mlkit4"] if pillar(c)) == [80, 112]
    assert any(portrait(c) and c["in_roi"][0] > 0 for c in F["mlkit4"])
    # the middle class a call leaves out, and the first and last class, exist in every fleet
    assert all(len(F[n]) >= 3 for n in rc.STEP_FLEETS)
    # xcd_*: the second class takes the one-XCD-per-frame order, with whole groups of 8 positions and a remainder
    for name in rc.XCD_FLEETS:
        a, b = F[name]
        assert rc.shares_lines(b) and b["n"] >= 8 and b["n"] % 8 != 0, name
        assert (b["n"] - 2) >= 8 and (b["n"] - 2) % 8 != 0                                       # the call with 9 of the 11
        assert tiles(a) * a["n"] % 8 != 0                                                        # the segment does not start on a multiple of 8 workgroups
    assert tiles(F["xcd_lite"][0]) * F["xcd_lite"][0]["n"] == 3 and tiles(F["xcd_lite"][1]) == 8
    assert tiles(F["xcd_mlkit"][1]) == 27 and pillar(F["xcd_mlkit"][1])


def test_helpers_agree_with_the_matrix():
    assert rc.geoms("xcd_lite") == [(108, 88, 1), (132, 100, 11)] and rc.first_streams("lite8") == list(range(0, 16, 2))
    assert rc.matrix_row("full-2056x1160")[5]["cls"] == "memset" and rc.matrix_row(None) is None
    with pytest.raises(AssertionError):
        rc.matrix_row("lite-1x1")
    assert {gc.row_id(r) for r in gc.ROWS} >= {c["row"] for f in rc.FLEETS.values() for c in f["classes"] if c["row"]}
