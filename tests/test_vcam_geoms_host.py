"""bsx_step_batch_vcam_geoms on a box without a GPU: the library's real host code runs against tests/hip_stub/libhipstub.so (two pretend devices, every HIP call
logged with the calling thread's current device and every kernel launch with its name and grid), driven by tests/hip_stub/drive_vcam_geoms.py for contexts on
device 1 with the caller on device 0.  Asserted:
  * header, both libraries and the binding agree on the new symbol;
  * an accepted call returns 0, makes HIP calls on device 1 only, restores the caller's device, stages ids and descriptors with one hipMemcpyAsync each behind a
    ring event and never synchronises the host;
  * its launch trace is exactly: one prep_geoms_k, the network, one tile_class_geoms_k, one mask_geoms_k, one vg_geoms_k — the same list on contexts of 1, 2 and 3
    classes and on one made by bsx_new — and none of the capture-size composite, outside-ROI, blend, resize or pack kernels; the grids are the sums they must be;
  * rings and tables are allocated once: the second call at an output size makes no hipMalloc and no hipMemcpy, a new output size allocates and uploads;
  * every refusal returns BSX_EINVAL with its words and makes no HIP call; n == 0 is a no-op; the dense and by-id vcam steps still refuse several classes;
  * MaskGen.step_vcam_geoms validates its arguments before the library is reached;
  * the two new kernels' resources (tools/kernel_regs.sh) and the counts the other resource tests pin."""
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
TILE_W, TILE_H = 128, 32          # mask tiles
VT_W, VT_H = 64, 32               # output tiles of the resize pass
IDS = [4, 0, 2, 5, 1, 3]


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
    log = str(tmp_path_factory.mktemp("vcam_geoms") / "hip.log")
    env = dict(os.environ, LD_PRELOAD=stub, BSX_STUB_LOG=log, BSX_STUB_NDEV="2")
    r = subprocess.run([sys.executable, os.path.join(STUB_DIR, "drive_vcam_geoms.py"), model_path("lite"), "1"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert "error" not in d, d
    lines = [l.split() for l in open(log).read().splitlines() if l.strip()]
    return d, lines


def _span(d, lines, key):
    a, b = d["calls"][key]["log"]
    return lines[a:b]


def _apis(d, lines, key):
    return [l[1] for l in _span(d, lines, key) if l[0] == "affine"]


def _kernels(d, lines, key):
    """(kernel name, grid x) of every launch of the call, in order"""
    out = []
    for l in _span(d, lines, key):
        if l[0] == "affine" and l[1] in ("hipLaunchKernel", "hipModuleLaunchKernel"):
            out.append((l[3], int(l[4][2:].split(",")[0])))
    return out


def _tiles(roi):
    return ((roi[2] + TILE_W - 1) // TILE_W) * ((roi[3] + TILE_H - 1) // TILE_H)


def _out_tiles(w, h):
    return ((w + VT_W - 1) // VT_W) * ((h + VT_H - 1) // VT_H)


OK_CALLS = ["trace_1", "trace_2", "trace_3", "trace_new", "trace_3_again", "yuyv", "odd_width", "own_size", "eighth", "subset", "bg_null_filter_off",
            "out_spans_touch"] + ["ring_%d" % i for i in range(6)]
BACK_END = ("prep_", "tile_class", "mask_geoms_k", "vg_geoms_k")


def test_header_library_and_binding_agree_on_the_new_symbol(stub):
    import ctypes
    from backscrub_amd import api, build
    sym = "bsx_step_batch_vcam_geoms"
    entry = [s for s in api.SYMBOLS if s[0] == sym]
    assert len(entry) == 1
    C = ctypes
    assert entry[0][1] is C.c_int and entry[0][2] == [C.c_void_p, C.POINTER(C.c_int), C.POINTER(api._GeomItem), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_uint]
    hdr = open(os.path.join(ROOT, "include", "bsx.h")).read()
    m = re.search(r"^BSX_API int %s\(([^)]*)\);" % sym, hdr, re.M)
    assert m, "the header does not declare %s" % sym
    assert re.sub(r"\s+", " ", m.group(1)) == "bsx_ctx* ctx, const int* ids, const bsx_geom_item* items, int n, int out_w, int out_h, void* stream, unsigned flags"
    for lib in (build.LIB, build.LIB_DBG):
        assert hasattr(ctypes.CDLL(lib), sym), (lib, sym)
    assert hasattr(api.MaskGen, "step_vcam_geoms")
    assert hdr.count("typedef struct bsx_geom_item") == 1 and ctypes.sizeof(api._GeomItem) == 32          # the item is reused as it is


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
    assert d["calls"]["geoms_after"]["rc"] == 0
    assert [n for n, _ in _kernels(d, lines, "geoms_after") if "mask_tile_geoms_k" in n]


def test_rings_and_tables_are_allocated_once(run):
    d, lines = run
    first = _apis(d, lines, "trace_3")
    # the first call at an output size: the id ring (pinned), and per class one table plus the record array; class 0's table is the dense step's
    assert first.count("hipHostMalloc") == 1 and first.count("hipMalloc") == 1 + 3 + 1, first
    again = _apis(d, lines, "trace_3_again")
    for api_name in ("hipMalloc", "hipHostMalloc", "hipMemcpy", "hipFree"):
        assert api_name not in again, "the second call at the same output size made a %s" % api_name
    for key in ["subset"] + ["ring_%d" % i for i in range(6)]:
        apis = _apis(d, lines, key)
        assert "hipHostMalloc" not in apis and "hipMalloc" not in apis and "hipMemcpy" not in apis, key
    for key in ("odd_width", "own_size", "eighth"):          # a new output size: its tables and records, no ring
        apis = _apis(d, lines, key)
        assert apis.count("hipMalloc") == 3 + 1 and "hipHostMalloc" not in apis, (key, apis)
    reused = [a for k in ("ring_%d" % i for i in range(6)) for a in _apis(d, lines, k)]
    assert "hipEventQuery" in reused
    lazy = _apis(d, lines, "trace_1")
    assert lazy.count("hipHostMalloc") == 2                   # a one-class context: descriptor ring and id ring on its first geoms-form step
    # bsx_delete frees what the calls allocated: as many hipFree as hipMalloc over the whole run
    allocs = sum(1 for l in lines if l[0] == "affine" and l[1] == "hipMalloc")
    frees = sum(1 for l in lines if l[0] == "affine" and l[1] == "hipFree")
    assert allocs == frees, (allocs, frees)


def test_the_launch_trace_is_the_sequence_and_does_not_depend_on_the_number_of_classes(run):
    d, lines = run
    traces = {k: _kernels(d, lines, k) for k in ("trace_1", "trace_2", "trace_3", "trace_new", "trace_3_again", "yuyv", "odd_width", "own_size", "eighth")}

    def names(t):
        return [re.sub(r"\d+", "#", n) for n, _ in t]
    assert names(traces["trace_1"]) == names(traces["trace_2"]) == names(traces["trace_3"]) == names(traces["trace_new"]) == names(traces["trace_3_again"])
    excluded = ("mask_tile_geoms_k", "mask_tile_k", "outside_roi", "blend", "resize_bgr", "yuyv_k", "bgr_to_yuyv", "vg_mixed_k", "prep_fused_k", "12tile_class_k",
                "mask_upscale_blur_k", "flip_bgr")
    for key, classes in (("trace_1", "c1"), ("trace_2", "c2"), ("trace_3", "c3"), ("trace_new", "cn"), ("yuyv", "c3"), ("odd_width", "c3"), ("own_size", "c3"),
                         ("eighth", "c3")):
        t = traces[key]
        one = {k: [x for x in t if k in x[0]] for k in ("prep_geoms_k", "tile_class_geoms_k", "mask_geoms_k", "vg_geoms_k")}
        for k, hit in one.items():
            assert len(hit) == 1, (key, k, [x[0] for x in t])
        assert not [x[0] for x in t if any(e in x[0] for e in excluded)], (key, [x[0] for x in t])
        # the order: prep, the network, tile classes, masks, the resize pass
        order = [x[0] for x in t]
        i_prep, i_cls, i_mask, i_vg = (order.index(one[k][0][0]) for k in ("prep_geoms_k", "tile_class_geoms_k", "mask_geoms_k", "vg_geoms_k"))
        assert i_prep == 0 and (i_cls, i_mask, i_vg) == (len(t) - 3, len(t) - 2, len(t) - 1), (key, order)
        assert len(t) - 4 >= 5, "no network between prep and the back end: %s" % order
        info = d["infos"][classes]
        of = [[q for q in info if q["first_stream"] <= s < q["first_stream"] + q["n_streams"]][0] for s in IDS]
        assert one["mask_geoms_k"][0][1] == sum(_tiles(q["roi"]) for q in of), (key, one["mask_geoms_k"])
        assert one["tile_class_geoms_k"][0][1] == len(IDS)
        assert one["prep_geoms_k"][0][1] == len(IDS) * 5 * 3            # segm_lite's 160 x 96 canvas: 5 x 3 tiles of 32 x 32 per position
        ow, oh = {"odd_width": (427, 240), "own_size": (640, 360), "eighth": (160, 90)}.get(key, (426, 240))
        assert one["vg_geoms_k"][0][1] == len(IDS) * _out_tiles(ow, oh), (key, one["vg_geoms_k"])

    def network(t):
        return [x for x in t if not any(s in x[0] for s in BACK_END)]
    assert network(traces["trace_1"]) == network(traces["trace_2"]) == network(traces["trace_3"]) == network(traces["trace_new"])
    # ... and it is the network of the geoms step
    geoms = [x for x in _kernels(d, lines, "geoms_after") if not any(s in x[0] for s in ("prep_", "tile_class", "mask_tile", "outside_roi"))]
    assert geoms == network(traces["trace_3"])
    sub = _kernels(d, lines, "subset")
    assert [x[1] for x in sub if "vg_geoms_k" in x[0]] == [2 * _out_tiles(426, 240)]


@pytest.mark.parametrize("key,words", [
    ("dup", ["ids[2] = 0", "repeats ids[0]"]),
    ("out_of_range", ["ids[1] = 6", "out of range"]),
    ("negative_n", ["n = -1", "negative"]),
    ("too_many", ["n = 7", "exceeds", "6 streams"]),
    ("ids_null", ["ids is NULL"]),
    ("items_null", ["items is NULL"]),
    ("out_w_zero", ["output size 0 x 240", "positive"]),
    ("out_h_negative", ["output size 426 x -1", "positive"]),
    ("batch_no_mask", ["flags 0x8", "has no vcam form"]),
    ("batch_yuyv_in", ["flags 0x10", "YUYV input"]),
    ("batch_flip", ["flags 0x2", "outside yuyv"]),
    ("batch_blur", ["flags 0x700", "outside yuyv"]),
    ("odd_out_w_yuyv", ["YUYV output needs an even width", "out_w = 427"]),
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
    ("out_spans_overlap", ["d_out", "overlaps the output of items["]),
    ("pending", ["pipelined composite is pending"]),
    ("class_off_route", ["items[0]", "stream 1", "642 x 480", "off the fused tile route", "bsx_step_batch_vcam_mixed"]),
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


@pytest.mark.parametrize("key", ["r_vcam", "r_vcam_mixed"])
def test_the_one_size_vcam_steps_keep_refusing_a_multi_geometry_context(run, key):
    d, lines = run
    c = d["calls"][key]
    assert c["rc"] == BSX_EINVAL and "context has 3 geometries" in c["error"], c
    assert [l for l in _span(d, lines, key) if l[0] != "neutral"] == []


def test_step_vcam_geoms_refuses_bad_arguments_before_reaching_c(monkeypatch):
    """every tensor is checked — frames and backgrounds against the class of their id, every out against the shape of outs[0] — before any library call"""
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
    out, out_odd, out_y = torch.zeros((6, 10, 3), dtype=torch.uint8), torch.zeros((6, 9, 2), dtype=torch.uint8), torch.zeros((6, 10, 2), dtype=torch.uint8)
    off = S(filter_off=True)
    with pytest.raises(api.BsxError, match="2 ids for 1 frames"):
        mg.step_vcam_geoms([0, 2], [small], [out, out], [off] * 2)
    with pytest.raises(api.BsxError, match="2 ids for 2 frames, 1 outs"):
        mg.step_vcam_geoms([0, 2], [small, big], [out], [off] * 2)
    with pytest.raises(api.BsxError, match=r"frames\[1\].*\[8,16,3\].*stream 2"):
        mg.step_vcam_geoms([0, 2], [small, small], [out, out.clone()], [off] * 2)
    with pytest.raises(api.BsxError, match="out of range"):
        mg.step_vcam_geoms([0, 4], [small, small], [out, out.clone()], [off] * 2)
    with pytest.raises(api.BsxError, match=r"outs\[1\].*\[6,10,3\].*size of outs\[0\]"):
        mg.step_vcam_geoms([0, 2], [small, big], [out, big.clone()], [off] * 2)
    with pytest.raises(api.BsxError, match=r"outs\[0\].*\[6,10,3\]"):
        mg.step_vcam_geoms([0], [small], [out.to(torch.float32)], [off])
    with pytest.raises(api.BsxError, match=r"outs\[0\].*\[6,12,3\]"):
        mg.step_vcam_geoms([0], [small], [torch.zeros((6, 24, 3), dtype=torch.uint8)[:, ::2]], [off])          # not contiguous
    with pytest.raises(api.BsxError, match=r"outs\[0\].*\[out_h,out_w,2\]"):
        mg.step_vcam_geoms([0], [small], [out], [off], yuyv=True)
    with pytest.raises(api.BsxError, match="even width.*9 wide"):
        mg.step_vcam_geoms([0], [small], [out_odd], [off], yuyv=True)
    with pytest.raises(api.BsxError, match=r"settings\[0\]: bgblur"):
        mg.step_vcam_geoms([0], [small], [out], [S(bgblur=7)])
    with pytest.raises(api.BsxError, match=r"settings\[0\] is not a StreamSetting"):
        mg.step_vcam_geoms([0], [small], [out], [None])
    with pytest.raises(api.BsxError, match=r"settings\[1\]: bg is required"):
        mg.step_vcam_geoms([0, 2], [small, big], [out_y, out_y.clone()], [off, S(flip_h=True)], yuyv=True)
    with pytest.raises(api.BsxError, match=r"settings\[1\]\.bg.*\[8,16,3\]"):
        mg.step_vcam_geoms([0, 2], [small, big], [out, out.clone()], [off, S(bg=small)])
    # host tensors are not device tensors
    with pytest.raises(api.BsxError, match=r"frames\[0\] must be a contiguous cuda:0"):
        Fake().step_vcam_geoms([0], [small], [out], [off])


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


def test_resources_of_the_two_new_kernels_and_the_pinned_counts():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not installed")
    rows = _survey()

    def pick(needle):
        hit = {k: v for k, v in rows.items() if needle in k}
        assert hit, needle
        return hit
    mask, vg = pick("mask_geoms_k"), pick("vg_geoms_k")
    assert len(mask) == 1 and len(vg) == 1
    for name, r in list(mask.items()) + list(vg.items()):
        assert r["scratch"] == 0, "%s spills %d bytes" % (name, r["scratch"])
    tile_lds = max(r["lds"] for r in pick("mask_tile_kI").values())
    assert list(mask.values())[0]["lds"] <= tile_lds, (mask, tile_lds)
    staged_lds = max(r["lds"] for r in pick("vg_mixed_k").values())
    assert staged_lds == 32768
    assert list(vg.values())[0]["lds"] <= staged_lds + 16, (vg, staged_lds)
    # every image kernel keeps scratch == 0
    assert not {k: v["scratch"] for k, v in rows.items() if v["scratch"]}
    # the counts pinned in tests/test_geoms_host.py and tests/test_kernel_resources.py still hold, and the existing kernels keep their names
    assert len(pick("prep_geoms_k")) == 3 and len(pick("tile_class_geoms_k")) == 1 and len(pick("mask_tile_geoms_k")) == 1 and len(pick("outside_roi_geoms_k")) == 1
    assert not [k for k in pick("mask_tile_geoms_k") if "mask_tile_geoms_kI" in k], "mask_tile_geoms_k became a template"
    assert len(pick("gauss_blur_k")) == 24 and len(pick("resize_bgr_batch_k")) == 1 and len(pick("vg_mixed_k")) == 4 and len(pick("vcam_blend_resize_k")) == 4
    assert len(pick("prep_fused_kI")) == 9 and len(pick("mask_tile_kI")) == 9 and len(pick("12tile_class_k")) == 1 and len(pick("outside_roi_mixed_k")) == 1
