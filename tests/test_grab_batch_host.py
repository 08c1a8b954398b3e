"""bsx_resize_bgr_batch and bsx_background_grab_batch on a box without a GPU: the library's real host code runs against tests/hip_stub/libhipstub.so (the
LD_PRELOAD interposer of tests/test_device_order.py: two pretend devices, every HIP call logged with the calling thread's current device and every kernel launch
with its name and grid), driven by tests/hip_stub/drive_grab_batch.py for a context on device 1 with the caller on device 0.  Asserted:
  * a good call — 1, 3 and n_streams images with one, two and three distinct source sizes, through either entry point — returns 0, makes HIP calls on device 1
    only, restores the caller's device, never synchronises the host, copies its descriptor table with hipMemcpyAsync behind a ring event, and makes EXACTLY ONE
    kernel launch, resize_bgr_batch_k, whose grid's second dimension is n;
  * a call uploads one resize table per distinct source size it sees for the first time (none for the identity and the exact-2x mode) and none the second time;
    more calls than the staging ring has entries still return 0;
  * the picture an explicit time names: frame_nos for at = (k + 0.5) / fps equal k mod n_i + 1 for animations of different fps and length, 1 for stills; with the
    clock, two entries naming one animation report one number;
  * each refusal returns BSX_EINVAL with a message that names the position and value, enqueues no HIP call at all and writes no frame number; n == 0 returns 0 and
    enqueues nothing;
  * MaskGen.resize_bgr_batch and grab_backgrounds refuse wrong shapes, dtypes, devices and mixed owners before they reach the library."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT, model_path

STUB_DIR = os.path.join(ROOT, "tests", "hip_stub")
STUB = os.path.join(STUB_DIR, "libhipstub.so")
BSX_EINVAL = -1
W, H, N = 640, 480, 8


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
    log = str(tmp_path_factory.mktemp("grab_batch") / "hip.log")
    env = dict(os.environ, LD_PRELOAD=stub, BSX_STUB_LOG=log, BSX_STUB_NDEV="2")
    r = subprocess.run([sys.executable, os.path.join(STUB_DIR, "drive_grab_batch.py"), model_path("lite"), str(W), str(H), str(N), "1"], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert "error" not in d, d
    lines = [l.split() for l in open(log).read().splitlines() if l.strip()]
    return d, lines


def _span(d, lines, key):
    a, b = d["calls"][key]["log"]
    return lines[a:b]


def _apis(d, lines, key):
    return [l[1] for l in _span(d, lines, key) if l[0] == "affine"]


RSZ = {"rsz_1": 1, "rsz_3": 3, "rsz_n": N, "rsz_1_again": 1, "rsz_3_again": 3, "rsz_n_again": N, "rsz_modes": 3, "rsz_shared_src": 2}
RSZ.update({"rsz_ring_%d" % i: 2 for i in range(6)})
GRAB = {"grab_1": 1, "grab_3": 3, "grab_n": N, "grab_n_again": N, "grab_no_nos": 2, "clock": 5}
GRAB.update({"grab_ring_%d" % i: 2 for i in range(6)})
OK_CALLS = dict(RSZ, **GRAB)


def test_good_calls_run_on_the_contexts_device_only_and_never_synchronise(run):
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
        assert apis.count("hipMemcpyAsync") == 1, "%s: the descriptor table goes to the device in ONE asynchronous copy: %s" % (key, apis)
        assert "hipEventRecord" in apis, "%s: the ring entry is not guarded by an event" % key
        assert apis.index("hipMemcpyAsync") < apis.index("hipLaunchKernel") < len(apis) - 1 - apis[::-1].index("hipEventRecord"), (key, apis)
        assert "hipStreamSynchronize" not in apis and "hipDeviceSynchronize" not in apis and "hipEventSynchronize" not in apis, "%s synchronised the host" % key


def test_exactly_one_launch_whose_grid_has_n_rows(run):
    d, lines = run
    for key, n in OK_CALLS.items():
        launches = [l for l in _span(d, lines, key) if l[0] == "affine" and "Launch" in l[1]]
        assert len(launches) == 1, (key, [l[3] for l in launches])
        assert "resize_bgr_batch_k" in launches[0][3], (key, launches[0][3])
        gx, gy, gz = (int(v) for v in launches[0][4][2:].split(","))
        assert (gy, gz) == (n, 1), (key, launches[0][4])
        assert gx == ((W // 4) * H + 255) // 256, "%s: one lane per four pixels of a row: %s" % (key, launches[0][4])
        assert launches[0][5] == "b=256,1,1"


def test_one_table_upload_per_new_source_size_and_none_the_second_time(run):
    d, lines = run

    def tables(key):                                   # a table is one allocation filled by four synchronous copies (xofs, yofs, xa, ya)
        apis = _apis(d, lines, key)
        assert apis.count("hipMemcpy") % 4 == 0, (key, apis)
        return apis.count("hipMemcpy") // 4

    assert tables("rsz_1") == 1
    assert tables("rsz_3") == 2
    assert tables("rsz_n") == 3
    for key in ("rsz_1_again", "rsz_3_again", "rsz_n_again", "rsz_modes", "rsz_shared_src", "grab_n_again"):
        assert tables(key) == 0, key
    assert tables("grab_1") + tables("grab_3") + tables("grab_n") == 2          # the two stills' sizes; the animations' were seen by the resize calls
    # the ring's own buffers: on the first call only
    assert _apis(d, lines, "rsz_1").count("hipHostMalloc") == 1
    for key in OK_CALLS:
        if key != "rsz_1":
            assert "hipHostMalloc" not in _apis(d, lines, key), key
    reused = [a for i in range(6) for a in _apis(d, lines, "rsz_ring_%d" % i)] + [a for i in range(6) for a in _apis(d, lines, "grab_ring_%d" % i)]
    assert "hipEventQuery" in reused, "entries of the ring are reused behind their events"


def test_an_explicit_time_names_the_picture(run):
    d, _ = run
    assert len(d["picks"]) == 21
    for pk in d["picks"]:
        c = d["calls"][pk["key"]]
        assert c["rc"] == 0, c
        want = pk["k"] % pk["frames"] + 1
        assert c["frame_nos"] == [want, 1, want], (pk, c["frame_nos"])
    assert d["calls"]["grab_n"]["frame_nos"] == [1] * N                          # at = 0: every source shows its first picture
    # at = 0.25 s: a (10 fps) shows picture 2, b (24 fps) picture 6, c (12.5 fps) picture 3 mod 3 = 0
    assert d["calls"]["grab_n_again"]["frame_nos"] == ([3, 1, 7, 1, 1, 3] * N)[:N]


def test_the_clock_is_read_once_for_the_whole_batch(run):
    d, _ = run
    nos = d["calls"]["clock"]["frame_nos"]
    assert nos[1] == 1
    assert nos[0] == nos[3] and nos[2] == nos[4], nos
    assert 1 <= nos[0] <= 5 and 1 <= nos[2] <= 7, nos


@pytest.mark.parametrize("key,words", [
    ("rsz_negative_n", ["n = -1", "negative"]),
    ("rsz_too_many", ["n = 9", "exceeds", "8 streams"]),
    ("rsz_items_null", ["items is NULL"]),
    ("rsz_bad_out_size", ["output size 0 x 480"]),
    ("rsz_null_src", ["items[1]", "d_src is NULL"]),
    ("rsz_null_dst", ["items[2]", "d_dst is NULL"]),
    ("rsz_bad_src_size", ["items[1]", "source size 0 x 7"]),
    ("rsz_dst_overlaps_dst", ["items[2]", "d_dst 0x", "overlaps the destination of items[1]"]),
    ("rsz_dst_overlaps_src", ["items[2]", "d_dst 0x", "overlaps the source picture of items[1]"]),
    ("grab_too_many", ["n = 9", "exceeds", "8 streams"]),
    ("grab_null_entry", ["bgs[2] is NULL"]),
    ("grab_foreign", ["bgs[1]", "another context"]),
    ("grab_bad_size", ["output size 640 x 0"]),
    ("grab_null_out", ["d_bgr_out is NULL"]),
    ("grab_short_stride", ["out_stride = 921599", "640 x 480", "921600"]),
    ("grab_nan", ["at_seconds = ", "nan"]),
    ("grab_inf", ["at_seconds = ", "inf"]),
])
def test_refusals_name_the_position_and_value_and_enqueue_nothing(run, key, words):
    d, lines = run
    c = d["calls"][key]
    assert c["rc"] == BSX_EINVAL, c
    fn = "bsx_resize_bgr_batch" if key.startswith("rsz_") else "bsx_background_grab_batch"
    assert c["error"].startswith("error: %s: " % fn), c["error"]
    for w in words:
        assert w in c["error"], (key, c["error"])
    assert "BSX_" not in c["error"], c["error"]
    assert _span(d, lines, key) == [], "%s: a refused call made HIP calls" % key
    assert c["caller_device"] == 0
    if c["frame_nos"] is not None:
        assert set(c["frame_nos"]) == {d["sentinel"]}, "%s: a refused call wrote frame numbers" % key
    if key.startswith("grab_"):
        assert c["error_thread"] == c["error"]       # also where a caller without a context can read it


@pytest.mark.parametrize("key,words", [("grab_negative_n", ["n = -1", "negative"]), ("grab_bgs_null", ["bgs is NULL"])])
def test_refusals_without_a_context_leave_their_text_with_the_thread(run, key, words):
    d, lines = run
    c = d["calls"][key]
    assert c["rc"] == BSX_EINVAL, c
    for w in words:
        assert w in c["error_thread"], (key, c["error_thread"])
    assert c["error_thread"].startswith("error: bsx_background_grab_batch: ")
    assert _span(d, lines, key) == []
    assert set(c["frame_nos"]) == {d["sentinel"]}


@pytest.mark.parametrize("key", ["rsz_empty", "grab_empty"])
def test_an_empty_batch_is_a_no_op(run, key):
    d, lines = run
    assert d["calls"][key]["rc"] == 0
    assert _span(d, lines, key) == []


def test_header_and_binding_agree_on_the_new_calls():
    import ctypes
    from backscrub_amd import api
    names = {s[0] for s in api.SYMBOLS}
    hdr = open(os.path.join(ROOT, "include", "bsx.h")).read()
    assert "bsx_resize_bgr_batch" in names and "BSX_API int bsx_resize_bgr_batch(" in hdr
    assert "bsx_background_grab_batch" in names and "BSX_API int bsx_background_grab_batch(" in hdr
    assert "typedef struct bsx_resize_item { const uint8_t* d_src; int sw, sh; uint8_t* d_dst; } bsx_resize_item;" in hdr
    assert ctypes.sizeof(api._ResizeItem) == 24
    assert api._ResizeItem.d_dst.offset == 16 and api._ResizeItem.sh.offset == 12
    import backscrub_amd
    assert backscrub_amd.grab_backgrounds is api.grab_backgrounds


def test_python_refuses_bad_arguments_before_reaching_c():
    """shape, dtype, device and "all of one MaskGen" are refused in Python: a MaskGen without a context would crash in the library otherwise"""
    torch = pytest.importorskip("torch")
    from backscrub_amd import api

    class Fake(api.MaskGen):
        def __init__(self):          # no context: validation happens before any library call
            self.width, self.height, self.device, self.n_streams, self.h = 8, 4, 0, 2, None

    class FakeBg(api.Background):
        def __init__(self, mg):
            self.mg, self.h = mg, 1

        def close(self):
            self.h = None

    mg, mg2 = Fake(), Fake()
    cpu = torch.zeros((4, 8, 3), dtype=torch.uint8)
    with pytest.raises(api.BsxError, match=r"srcs\[0\] must be a contiguous cuda:0 uint8"):
        mg.resize_bgr_batch([cpu], 8, 4)
    with pytest.raises(api.BsxError, match=r"srcs\[0\]"):
        mg.resize_bgr_batch(["not a tensor", cpu], 8, 4)
    with pytest.raises(api.BsxError, match="3 images for a context of 2 streams"):
        mg.resize_bgr_batch([cpu] * 3, 8, 4)
    with pytest.raises(api.BsxError, match="output size 0 x 4"):
        mg.resize_bgr_batch([cpu], 0, 4)
    a, b, other = FakeBg(mg), FakeBg(mg), FakeBg(mg2)
    with pytest.raises(api.BsxError, match=r"backgrounds\[1\] belongs to another MaskGen"):
        api.grab_backgrounds([a, other], 8, 4)
    with pytest.raises(api.BsxError, match=r"backgrounds\[1\] is not an open Background"):
        api.grab_backgrounds([a, None], 8, 4)
    with pytest.raises(api.BsxError, match="3 backgrounds for a context of 2 streams"):
        api.grab_backgrounds([a, b, a], 8, 4)
    with pytest.raises(api.BsxError, match="output size 8 x -1"):
        api.grab_backgrounds([a, b], 8, -1)
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(api.BsxError, match="at = "):
            api.grab_backgrounds([a, b], 8, 4, at=bad)
    for bad_out in (torch.zeros((2, 4, 8, 3), dtype=torch.uint8), torch.zeros((2, 4, 8, 3), dtype=torch.float32), torch.zeros((1, 4, 8, 3), dtype=torch.uint8)):
        with pytest.raises(api.BsxError, match="out must be a cuda:0 uint8 tensor"):
            api.grab_backgrounds([a, b], 8, 4, out=bad_out, at=0.0)
