"""bsx_new_geoms / bsx_step_batch_geoms on a box without a GPU: the library's real host code runs against tests/hip_stub/libhipstub.so (two pretend devices, every
HIP call logged with the calling thread's current device and every kernel launch with its name and grid), driven by tests/hip_stub/drive_geoms.py for contexts on
device 1 with the caller on device 0.  Asserted:
  * a step of a three-class context returns 0, makes HIP calls on device 1 only, restores the caller's device, stages ids and descriptors with hipMemcpyAsync
    behind a ring event, never synchronises the host and allocates its ring once;
  * the launch trace: one step of the same number of positions on contexts of 1, 2 and 3 classes is the SAME list of kernel names — exactly one prep, one
    tile-class, one tile and at most one outside-ROI launch — the tile grid is the sum of the positions' tile counts, and the network's launches are those of
    bsx_step_batch_mixed on a one-geometry context;
  * every other stepping entry point on a three-class context returns BSX_EINVAL, names the geometry count and makes no HIP call; reset, reset_streams, info,
    resize and the background grab run;
  * each refusal of the step and of bsx_new_geoms: BSX_EINVAL / NULL, a text with position or class and value, no HIP call; n == 0 is a no-op;
  * MaskGen.step_geoms validates its arguments against the class of each id before the library is reached;
  * the new kernels' resources (tools/kernel_regs.sh): no scratch, the prep form within 64 architectural VGPRs, the tile form's LDS not above mask_tile_k's."""
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
TILE_W, TILE_H = 128, 32


@pytest.fixture(scope="module")
def stub():
    from backscrub_amd import build
    build.build()
    src = os.path.join(STUB_DIR, "hip_stub.cpp")
    if not os.path.exists(STUB) or os.path.getmtime(STUB) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", STUB, src])
    return STUB


@pytest.fixture(scope="module")
def run(stub, tmp_path_factory):
    log = str(tmp_path_factory.mktemp("geoms") / "hip.log")
    env = dict(os.environ, LD_PRELOAD=stub, BSX_STUB_LOG=log, BSX_STUB_NDEV="2")
    r = subprocess.run([sys.executable, os.path.join(STUB_DIR, "drive_geoms.py"), model_path("lite"), "1"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert "error" not in d, d
    lines = [l.split() for l in open(log).read().splitlines() if l.strip()]
    return d, lines


def _span(d, lines, key):
    a, b = d["calls"][key]["log"]
    return lines[a:b]


def _kernels(d, lines, key):
    """(kernel name, grid x) of every launch of the call, in order"""
    out = []
    for l in _span(d, lines, key):
        if l[0] == "affine" and l[1] in ("hipLaunchKernel", "hipModuleLaunchKernel"):
            out.append((l[3], int(l[4][2:].split(",")[0])))
    return out


def _tiles(roi):
    return ((roi[2] + TILE_W - 1) // TILE_W) * ((roi[3] + TILE_H - 1) // TILE_H)


OK_CALLS = ["trace_1", "trace_2", "trace_3", "trace_3_again", "yuyv", "no_mask", "subset", "on_bsx_new", "after_reset", "bg_null_filter_off"] + \
    ["ring_%d" % i for i in range(6)]


def test_header_library_and_binding_agree_on_the_new_symbols(stub):
    import ctypes
    from backscrub_amd import api, build
    names = {s[0] for s in api.SYMBOLS}
    hdr = open(os.path.join(ROOT, "include", "bsx.h")).read()
    for sym in ("bsx_new_geoms", "bsx_geom_count", "bsx_get_geom_info", "bsx_step_batch_geoms"):
        assert sym in names and re.search(r"^BSX_API [^;(]*\b%s\(" % sym, hdr, re.M), sym
        for lib in (build.LIB, build.LIB_DBG):
            assert hasattr(ctypes.CDLL(lib), sym), (lib, sym)
    assert "#define BSX_MAX_GEOMS 8" in hdr
    assert ctypes.sizeof(api._Geometry) == 12 and ctypes.sizeof(api._GeomItem) == 32 and ctypes.sizeof(api._GeomInfo) == 56


def test_geometry_info_of_the_classes(run):
    d, _ = run
    g = d["infos"]["c3"]
    assert [(q["width"], q["height"], q["n_streams"], q["first_stream"]) for q in g] == [(640, 480, 2, 0), (1280, 720, 2, 2), (640, 360, 2, 4)]
    assert g[0]["in_roi"] == [16, 0, 128, 96] and g[0]["roi"] == [0, 0, 640, 480]
    assert g[1]["roi"] == [40, 0, 1200, 720] and g[2]["roi"] == [20, 0, 600, 360]
    assert [q["mask_offset"] for q in g] == [0, 2 * 640 * 480, 2 * 640 * 480 + 2 * 1280 * 720]
    assert d["mask_bytes"] == 2 * (640 * 480 + 1280 * 720 + 640 * 360) and d["masks_dev"]
    assert d["info"] == {"width": 640, "height": 480, "n_streams": 6}          # class 0's geometry, the total stream count
    assert len(d["infos"]["c1"]) == 1 and d["one_ok"] == [True, True]


def test_steps_run_on_the_contexts_device_only_and_never_synchronise(run):
    d, lines = run
    for key in OK_CALLS:
        c = d["calls"][key]
        assert c["rc"] == 0, (key, c)
        assert c["caller_device"] == 0, "%s: the caller's device was not restored" % key
        span = _span(d, lines, key)
        affine = [l for l in span if l[0] == "affine"]
        assert affine, "%s enqueued nothing" % key
        off = [l for l in affine if int(l[2]) != 1]
        assert not off, "%s: HIP calls made while device 0 was current: %s" % (key, sorted({l[1] for l in off}))
        assert not [l for l in span if l[0] == "MISMATCH"], key
        apis = [l[1] for l in affine]
        assert apis.count("hipMemcpyAsync") == 2, "%s: ids and descriptors go to the device in one copy each: %s" % (key, apis)
        assert "hipEventRecord" in apis, "%s: the ring entry is not guarded by an event" % key
        assert "hipStreamSynchronize" not in apis and "hipDeviceSynchronize" not in apis and "hipEventSynchronize" not in apis, "%s synchronised the host" % key
    assert d["pipelined"] == [0, 0]


def test_the_rings_are_allocated_once(run):
    d, lines = run
    first = [l[1] for l in _span(d, lines, "trace_3") if l[0] == "affine"]
    assert first.count("hipHostMalloc") == 1          # the id ring (the descriptor ring of a multi-class context exists since bsx_new_geoms)
    lazy = [l[1] for l in _span(d, lines, "trace_1") if l[0] == "affine"]
    assert lazy.count("hipHostMalloc") == 2           # a one-class context: descriptor ring and id ring on the first geoms step
    for key in ["trace_3_again", "yuyv", "no_mask", "subset", "after_reset"] + ["ring_%d" % i for i in range(6)]:
        apis = [l[1] for l in _span(d, lines, key) if l[0] == "affine"]
        assert "hipHostMalloc" not in apis and "hipMalloc" not in apis, key
    reused = [l[1] for k in ("ring_%d" % i for i in range(6)) for l in _span(d, lines, k) if l[0] == "affine"]
    assert "hipEventQuery" in reused


def test_the_launch_trace_does_not_depend_on_the_number_of_classes(run):
    d, lines = run
    traces = {k: _kernels(d, lines, k) for k in ("trace_1", "trace_2", "trace_3", "mixed_1")}

    def names(t, drop_outside=True):
        return [re.sub(r"\d+", "#", n) for n, _ in t if not (drop_outside and "outside_roi" in n)]
    # the same list of kernel names whatever the number of classes (the outside-ROI launch exists only where some class has a ROI smaller than its frame)
    assert names(traces["trace_1"]) == names(traces["trace_2"]) == names(traces["trace_3"])
    for key, classes in (("trace_1", "c1"), ("trace_2", "c2"), ("trace_3", "c3")):
        t = traces[key]
        prep = [x for x in t if "prep_geoms_k" in x[0]]
        cls = [x for x in t if "tile_class_geoms_k" in x[0]]
        tile = [x for x in t if "mask_tile_geoms_k" in x[0]]
        outside = [x for x in t if "outside_roi_geoms_k" in x[0]]
        assert len(prep) == 1 and len(cls) == 1 and len(tile) == 1 and len(outside) <= 1, (key, [x[0] for x in t])
        assert not [x for x in t if "prep_fused_k" in x[0] or "mask_tile_k" in x[0] or "12tile_class_k" in x[0] or "outside_roi_mixed_k" in x[0]], key
        info = d["infos"][classes]
        ids = [4, 0, 2, 5, 1, 3]
        of = [[q for q in info if q["first_stream"] <= s < q["first_stream"] + q["n_streams"]][0] for s in ids]
        assert tile[0][1] == sum(_tiles(q["roi"]) for q in of), (key, tile)
        assert cls[0][1] == len(ids)
        assert prep[0][1] == len(ids) * 5 * 3                      # segm_lite's 160 x 96 canvas: 5 x 3 tiles of 32 x 32 per position
        blocks = [((q["width"] // 4) * q["height"] + 255) // 256 if q["roi"] != [0, 0, q["width"], q["height"]] else 0 for q in of]
        assert (outside[0][1] if outside else 0) == sum(blocks), (key, outside, blocks)
    assert len([x for x in traces["trace_3"] if "outside_roi_geoms_k" in x[0]]) == 1 and not [x for x in traces["trace_1"] if "outside_roi" in x[0]]
    # the network: exactly the launches (names and grids) of bsx_step_batch_mixed on a one-geometry context with the same n

    def network(t):
        return [x for x in t if not any(s in x[0] for s in ("prep_", "tile_class", "mask_tile", "outside_roi"))]
    net = network(traces["mixed_1"])
    assert len(net) >= 5
    for key in ("trace_1", "trace_2", "trace_3"):
        assert network(traces[key]) == net, key
    assert len(traces["mixed_1"]) == len(traces["trace_1"])


@pytest.mark.parametrize("key", ["r_step", "r_yuyv", "r_ex", "r_streams", "r_mixed", "r_vcam", "r_vcam_mixed", "r_pipelined", "r_pipelined_flush", "r_process",
                                 "r_process_host", "r_composite", "r_profile", "r_stage", "r_tile_stats", "r_live"])
def test_every_other_stepping_entry_point_refuses_a_multi_geometry_context(run, key):
    d, lines = run
    c = d["calls"][key]
    assert c["rc"] == BSX_EINVAL, c
    assert "context has 3 geometries" in c["error"], c["error"]
    assert [l for l in _span(d, lines, key) if l[0] != "neutral"] == [], "%s: a refused call made HIP calls" % key
    assert c["caller_device"] == 0


def test_the_allowed_entry_points_run_on_a_multi_geometry_context(run):
    d, lines = run
    for key in ("a_info", "a_reset", "a_reset_streams", "a_resize", "a_grab", "a_debug_buffer"):
        assert d["calls"][key]["rc"] == 0, (key, d["calls"][key])
        assert d["calls"][key]["caller_device"] == 0
    sets = [int(l[3][2:]) for l in _span(d, lines, "a_reset") if l[1] == "hipMemsetAsync"]
    assert len(sets) == 2 and sets[1] == d["mask_bytes"], sets                        # ofinal, then the whole mask allocation
    resets = [l for l in _span(d, lines, "a_reset_streams") if l[1] == "hipLaunchKernel"]
    assert len(resets) == 3 and all("reset_slots_k" in l[3] for l in resets)          # one launch per class present
    assert all(l[4].endswith(",1,1") for l in resets)                                  # ... of one slot each
    assert all(int(l[2]) == 1 for l in _span(d, lines, "a_reset_streams") if l[0] == "affine")


@pytest.mark.parametrize("key,words", [
    ("dup", ["ids[2] = 0", "repeats ids[0]"]),
    ("out_of_range", ["ids[1] = 6", "out of range"]),
    ("negative_n", ["n = -1", "negative"]),
    ("too_many", ["n = 7", "exceeds", "6 streams"]),
    ("ids_null", ["ids is NULL"]),
    ("items_null", ["items is NULL"]),
    ("batch_flip", ["flags 0x2", "yuyv / no-mask"]),
    ("batch_yuyv_in", ["flags 0x10", "YUYV input"]),
    ("batch_blur", ["flags 0x700", "yuyv / no-mask"]),
    ("setting_blur", ["items[2]", "flags 0x700", "background blur"]),
    ("setting_bit0", ["items[3]", "flags 0x3", "flip / filter-off"]),
    ("frame_null", ["items[1]", "d_frame is NULL"]),
    ("frame_unaligned", ["items[1]", "d_frame", "not 4-byte aligned"]),
    ("out_null", ["items[4]", "d_out is NULL"]),
    ("out_unaligned", ["items[4]", "d_out", "not 4-byte aligned"]),
    ("bg_null", ["items[5]", "d_bg is NULL"]),
    ("bg_unaligned", ["items[5]", "d_bg", "not 4-byte aligned"]),
    ("out_is_frame", ["items[2]", "d_out", "overlaps a frame or background of items[2]"]),
    ("out_overlaps_other_frame", ["items[2]", "overlaps a frame or background of items[0]"]),
    ("out_overlaps_bg", ["items[3]", "overlaps a frame or background of items[1]"]),
    ("out_overlaps_out", ["d_out", "overlaps the output of items["]),
    ("pending", ["pipelined composite is pending"]),
    ("class_off_route", ["items[0]", "stream 1", "642 x 480", "off the fused tile route"]),
    ("odd_width_yuyv", ["items[0]", "YUYV output needs an even width", "641 x 480"]),
    ("onmask", ["onmask"]),
])
def test_refusals_name_the_position_and_value_and_enqueue_nothing(run, key, words):
    d, lines = run
    c = d["calls"][key]
    assert c["rc"] == BSX_EINVAL, c
    for w in words:
        assert w in c["error"], (key, c["error"])
    assert "BSX_" not in c["error"], c["error"]
    assert _span(d, lines, key) == [], "%s: a refused call made HIP calls" % key
    assert c["caller_device"] == 0


def test_an_empty_batch_is_a_no_op(run):
    d, lines = run
    assert d["calls"]["empty"]["rc"] == 0
    assert _span(d, lines, "empty") == []


@pytest.mark.parametrize("key,words", [
    ("new_zero", ["n_geoms = 0"]),
    ("new_nine", ["n_geoms = 9"]),
    ("new_null", ["geoms is NULL"]),
    ("new_bad_size", ["geoms[1]", "0 x 720", "not positive"]),
    ("new_bad_count", ["geoms[1]", "1280 x 720", "n_streams = 0"]),
    ("new_same_size", ["geoms[2]", "640 x 480", "repeats the size of geoms[0]"]),
    ("new_too_many_streams", ["geoms[1]", "1280 x 720", "70000", "65535"]),
    ("new_onmask", ["onmask", "one geometry"]),
    ("new_off_route", ["geoms[1]", "1920 x 1080", "roi.w 1799", "fused tile route"]),
])
def test_bsx_new_geoms_refusals_return_null_and_name_the_class(run, key, words):
    d, lines = run
    c = d["calls"][key]
    assert c["null"], c
    for w in words:
        assert w in c["error"], (key, c["error"])
    assert [l for l in _span(d, lines, key) if l[0] == "affine"] == [], "%s: a refused creation touched the device" % key


def test_step_geoms_refuses_bad_arguments_before_reaching_c(monkeypatch):
    """every tensor is checked against the class of its id — shape, dtype, layout, device — and the lists against the number of ids, before any library call"""
    torch = pytest.importorskip("torch")
    from backscrub_amd import api

    class Fake(api.MaskGen):
        def __init__(self):          # no context: validation happens before any library call
            self.width, self.height, self.n_streams, self.device, self.h = 8, 4, 4, 0, None
            self._geoms = [dict(width=8, height=4, n_streams=2, first_stream=0, roi=[0, 0, 8, 4], in_roi=[0, 0, 8, 4], mask_offset=0),
                           dict(width=16, height=8, n_streams=2, first_stream=2, roi=[0, 0, 16, 8], in_roi=[0, 0, 8, 4], mask_offset=64)]

    class OnDevice(Fake):            # host tensors stand in for device ones: the checks that need no device
        def _on_device(self, t):
            return True

    def no_c():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(api, "lib", no_c)
    mg = OnDevice()
    S = api.StreamSetting
    small, big = torch.zeros((4, 8, 3), dtype=torch.uint8), torch.zeros((8, 16, 3), dtype=torch.uint8)
    with pytest.raises(api.BsxError, match="2 ids for 1 frames"):
        mg.step_geoms([0, 2], [small], [small, big], [S(filter_off=True)] * 2)
    with pytest.raises(api.BsxError, match=r"frames\[1\].*\[8,16,3\].*stream 2"):
        mg.step_geoms([0, 2], [small, small], [small, big], [S(filter_off=True)] * 2)
    with pytest.raises(api.BsxError, match="out of range"):
        mg.step_geoms([0, 4], [small, small], [small, big], [S(filter_off=True)] * 2)
    with pytest.raises(api.BsxError, match=r"settings\[0\]: bgblur"):
        mg.step_geoms([0], [small], [small], [S(bgblur=7)])
    with pytest.raises(api.BsxError, match=r"settings\[0\] is not a StreamSetting"):
        mg.step_geoms([0], [small], [small], [None])
    with pytest.raises(api.BsxError, match=r"outs\[0\].*\[4,8,2\]"):
        mg.step_geoms([0], [small], [small], [S(filter_off=True)], yuyv=True)
    with pytest.raises(api.BsxError, match=r"settings\[1\]: bg is required"):
        mg.step_geoms([0, 2], [small, big], [small, big], [S(filter_off=True), S(flip_h=True)])
    with pytest.raises(api.BsxError, match=r"settings\[1\]\.bg.*\[8,16,3\]"):
        mg.step_geoms([0, 2], [small, big], [small, big], [S(filter_off=True), S(bg=small)])
    with pytest.raises(api.BsxError, match=r"frames\[0\].*\[4,8,3\]"):
        mg.step_geoms([0], [small.to(torch.float32)], [small], [S(filter_off=True)])
    # host tensors are not device tensors
    with pytest.raises(api.BsxError, match=r"frames\[0\] must be a contiguous cuda:0"):
        Fake().step_geoms([0], [small], [small], [S(filter_off=True)])
    with pytest.raises(api.BsxError, match="geometries must be"):
        api.MaskGen.with_geometries("m.tflite", [(640, 480)])


def _survey():
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_regs.sh"), os.path.join(ROOT, "backscrub_amd", "csrc", "kernels_img.hip")], capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0 and "compile failed" not in r.stdout, r.stdout[-500:] + r.stderr[-500:]
    row = re.compile(r"^(\S+)\s+vgpr\+agpr\s+(\d+)\s+accum_offset\s+(\d+)\s+lds\s+(\d+)\s+scratch\s+(\d+)")
    rows = {}
    for line in r.stdout.splitlines():
        m = row.match(line)
        if m:
            rows[m.group(1)] = dict(vgpr=int(m.group(2)), arch_vgpr=int(m.group(3)), lds=int(m.group(4)), scratch=int(m.group(5)))
    return rows


def test_resources_of_the_new_kernels():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not installed")
    rows = _survey()

    def pick(needle):
        hit = {k: v for k, v in rows.items() if needle in k}
        assert hit, needle
        return hit
    new = {}
    for needle in ("prep_geoms_k", "tile_class_geoms_k", "mask_tile_geoms_k", "outside_roi_geoms_k"):
        new.update(pick(needle))
    assert len(pick("prep_geoms_k")) == 3 and len(new) == 6
    for name, r in new.items():
        assert r["scratch"] == 0, "%s spills %d bytes" % (name, r["scratch"])
    for name, r in pick("prep_geoms_k").items():
        assert r["arch_vgpr"] <= 64, "%s: %d registers (prep_fused_k's bound)" % (name, r["arch_vgpr"])
    tile_lds = max(r["lds"] for r in pick("mask_tile_kI").values())
    for name, r in pick("mask_tile_geoms_k").items():
        assert r["lds"] <= tile_lds, "%s: %d B of LDS, mask_tile_k has %d" % (name, r["lds"], tile_lds)
    # the counts other tests pin are unchanged, and the existing instantiations keep their names
    assert len(pick("gauss_blur_k")) == 24 and len(pick("resize_bgr_batch_k")) == 1 and len(pick("vg_mixed_k")) == 4
    assert len(pick("prep_fused_kI")) == 9 and len(pick("mask_tile_kI")) == 9 and len(pick("12tile_class_k")) == 1 and len(pick("outside_roi_mixed_k")) == 1
