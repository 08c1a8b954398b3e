"""BSX_STREAM_YUYV_IN on a box without a GPU: the library's real host code under tests/hip_stub/libhipstub.so (every kernel launch logged with its name and grid),
driven by tests/geoms_yuyv_in_drive.py.  Asserted:
  * a call of BGR items launches exactly the kernels it launched before the bit existed (prep_geoms_k, tile_class_geoms_k, mask_tile_geoms_k, outside_roi_geoms_k;
    mask_geoms_k and vg_geoms_k for the vcam step), before and after a call with YUYV items;
  * ONE YUYV item switches the call's frame-reading launches to the per-format kernels — the same number of launches, the same grids, the same network launches —
    and the launches that read no frame (tile_class_geoms_k, mask_geoms_k) stay;
  * the refusals return BSX_EINVAL with their texts and make no HIP call: the batch flag on both entry points, an output over the last bytes of a YUYV frame (and a
    BGR frame keeps its W * H * 3 extent), a YUYV item of a class whose down-scale is the 2x2 area mean, bit 64 in the mixed steps' settings;
  * an output directly behind the W * H * 2 bytes of a YUYV frame is accepted."""
import json
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT, model_path

STUB_DIR = os.path.join(ROOT, "tests", "hip_stub")
STUB = os.path.join(STUB_DIR, "libhipstub.so")
BSX_EINVAL = -1
FMT = {"prep_geoms_k": "prep_geoms_fmt_k", "mask_tile_geoms_k": "mask_tile_geoms_fmt_k", "outside_roi_geoms_k": "outside_roi_geoms_fmt_k", "vg_geoms_k": "vg_geoms_fmt_k"}


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from backscrub_amd import build
    build.build()
    src = os.path.join(STUB_DIR, "hip_stub.cpp")
    if not os.path.exists(STUB) or os.path.getmtime(STUB) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", STUB, src])
    log = str(tmp_path_factory.mktemp("geoms_yuyv_in") / "hip.log")
    env = dict(os.environ, LD_PRELOAD=STUB, BSX_STUB_LOG=log, BSX_STUB_NDEV="2")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "geoms_yuyv_in_drive.py"), model_path("lite"), "1"], env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert "error" not in d, d
    return d, [l.split() for l in open(log).read().splitlines() if l.strip()]


def _span(d, lines, key):
    a, b = d["calls"][key]["log"]
    return lines[a:b]


def _kernels(d, lines, key):
    """(kernel family, mangled name, grid x) of every launch of the call, in order; family: the name up to its template arguments, digits of the mangling dropped"""
    out = []
    for l in _span(d, lines, key):
        if l[0] == "affine" and l[1] in ("hipLaunchKernel", "hipModuleLaunchKernel"):
            m = re.search(r"([a-z][a-z0-9_]*_k)(?:I|E|$)", l[3])
            out.append((m.group(1) if m else l[3], l[3], int(l[4][2:].split(",")[0])))
    return out


def _families(t):
    return [f for f, _, _ in t]


def test_a_call_of_bgr_items_launches_the_kernels_it_always_did(run):
    d, lines = run
    for key in ("bgr", "bgr_again", "v_bgr"):
        assert d["calls"][key]["rc"] == 0, d["calls"][key]
        assert not [f for f in _families(_kernels(d, lines, key)) if "_fmt_k" in f], key
    t = _families(_kernels(d, lines, "bgr"))
    for name in ("prep_geoms_k", "tile_class_geoms_k", "mask_tile_geoms_k", "outside_roi_geoms_k"):
        assert t.count(name) == 1, (name, t)
    assert _kernels(d, lines, "bgr") == _kernels(d, lines, "bgr_again")
    v = _families(_kernels(d, lines, "v_bgr"))
    for name in ("prep_geoms_k", "tile_class_geoms_k", "mask_geoms_k", "vg_geoms_k"):
        assert v.count(name) == 1, (name, v)


@pytest.mark.parametrize("key,base", [("one_yuyv", "bgr"), ("all_yuyv", "bgr"), ("all_yuyv_yuyv_out", "bgr"), ("v_mixed", "v_bgr"), ("v_mixed_yuyv_out", "v_bgr")])
def test_one_yuyv_item_switches_the_frame_reading_launches_and_nothing_else(run, key, base):
    d, lines = run
    assert d["calls"][key]["rc"] == 0, d["calls"][key]
    got, want = _kernels(d, lines, key), _kernels(d, lines, base)
    assert len(got) == len(want)
    for (gf, gname, ggrid), (wf, wname, wgrid) in zip(got, want):
        assert ggrid == wgrid, (gf, wf)
        if wf in FMT:
            assert gf == FMT[wf], "%s: %s where the call has a YUYV item" % (key, gname)
        else:
            assert gname == wname, "%s: a launch that reads no frame changed: %s -> %s" % (key, wname, gname)
    apis = [l[1] for l in _span(d, lines, key) if l[0] == "affine"]
    assert apis.count("hipMemcpyAsync") == 2 and "hipStreamSynchronize" not in apis and "hipDeviceSynchronize" not in apis


@pytest.mark.parametrize("key,words", [
    ("r_batch_flag", ["flags 0x10", "YUYV input", "items[i].setting.flags"]),
    ("r_v_batch_flag", ["flags 0x10", "YUYV input"]),
    ("r_overlap", ["items[0]", "d_out", "overlaps a frame or background of items[0]"]),
    ("r_v_overlap", ["items[0]", "d_out", "overlaps a frame or background of items[0]"]),
    ("r_bgr_extent", ["items[0]", "overlaps a frame or background of items[0]"]),
    ("r_area", ["items[1]", "stream 1", "256 x 192", "no fused YUYV prep", "2x2 area mean", "bsx_yuyv_to_bgr"]),
    ("r_v_area", ["items[1]", "stream 1", "256 x 192", "2x2 area mean", "bsx_yuyv_to_bgr"]),
    ("r_mixed", ["settings[0]", "flags 0x40", "flip / blur / filter-off"]),
    ("r_vcam_mixed", ["settings[0]", "flags 0x40", "flip / blur / filter-off"]),
])
def test_refusals_name_the_position_and_enqueue_nothing(run, key, words):
    d, lines = run
    c = d["calls"][key]
    assert c["rc"] == BSX_EINVAL, c
    for w in words:
        assert w in c["error"], (key, c["error"])
    assert "BSX_" not in c["error"], c["error"]
    assert _span(d, lines, key) == [], "%s: a refused call made HIP calls" % key


def test_what_is_accepted(run):
    d, lines = run
    ca = d["infos"]["ca"]
    assert ca[1]["roi"] == [0, 0, 256, 192] and ca[1]["in_roi"][2:] == [128, 96]          # exactly twice the model ROI: the area table
    for key in ("behind", "v_behind", "area_as_bgr"):
        assert d["calls"][key]["rc"] == 0, (key, d["calls"][key])
    # the area class's stream as BGR next to a YUYV VGA stream: the per-format prep, whose BGR position takes the non-linear body
    assert "prep_geoms_fmt_k" in _families(_kernels(d, lines, "area_as_bgr"))
