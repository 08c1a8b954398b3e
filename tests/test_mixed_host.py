"""bsx_step_batch_mixed on a box without a GPU: the library's real host code runs against tests/hip_stub/libhipstub.so (the LD_PRELOAD interposer of
tests/test_device_order.py: two pretend devices, every HIP call logged with the calling thread's current device and every kernel launch with its name and grid),
driven by tests/hip_stub/drive_mixed.py for a context on device 1 with the caller on device 0.  Asserted:
  * the dense call, the id call, every batch flag set and batches with 0, 1 and 2 distinct blur sizes return 0, make HIP calls on device 1 only, restore the
    caller's device, never synchronise the host, copy the descriptor table with hipMemcpyAsync behind a ring event, and make exactly ONE blur launch per distinct
    blur size and ONE tile launch;
  * each refusal returns BSX_EINVAL with a message that names the position and value, and enqueues no HIP call at all; n == 0 returns 0 and enqueues nothing;
  * the flag bit of the filter switch stays refused by every other step entry point;
  * MaskGen.step_mixed refuses a wrong-shaped background and a settings list of the wrong length before it reaches the library."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT, model_path

STUB_DIR = os.path.join(ROOT, "tests", "hip_stub")
STUB = os.path.join(STUB_DIR, "libhipstub.so")
BSX_EINVAL = -1


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
    log = str(tmp_path_factory.mktemp("mixed") / "hip.log")
    env = dict(os.environ, LD_PRELOAD=stub, BSX_STUB_LOG=log, BSX_STUB_NDEV="2")
    W, H, n = 640, 480, 4
    r = subprocess.run([sys.executable, os.path.join(STUB_DIR, "drive_mixed.py"), model_path("lite"), str(W), str(H), str(n), "1"], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert "error" not in d, d
    lines = [l.split() for l in open(log).read().splitlines() if l.strip()]
    return d, lines


def _span(d, lines, key):
    a, b = d["calls"][key]["log"]
    return lines[a:b]


def _launches(d, lines, key, needle):
    return [l for l in _span(d, lines, key) if l[0] == "affine" and l[1] == "hipLaunchKernel" and needle in l[3]]


OK_CALLS = ["dense", "ids", "blur0", "blur1", "blur2", "yuyv", "no_mask", "yuyv_in", "yuyv_in_blur", "after_flush"] + ["ring_%d" % i for i in range(6)]


def test_mixed_calls_run_on_the_contexts_device_only(run):
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
        assert "hipMemcpyAsync" in apis, "%s: the descriptor table never went to the device" % key
        assert "hipEventRecord" in apis, "%s: the ring entry is not guarded by an event" % key
        assert "hipStreamSynchronize" not in apis and "hipDeviceSynchronize" not in apis and "hipEventSynchronize" not in apis, "%s synchronised the host" % key
    assert d["pipelined"] == [0, 0]


def test_one_tile_launch_and_one_blur_launch_per_distinct_blur_size(run):
    d, lines = run
    for key in OK_CALLS:
        tiles = _launches(d, lines, key, "mask_tile_k") + _launches(d, lines, key, "mask_upscale_blur_k")
        assert len(tiles) == 1, (key, [l[3] for l in tiles])
        assert "ELb1EEEv" in tiles[0][3], "%s: not the mixed instantiation: %s" % (key, tiles[0][3])
    base = len(_launches(d, lines, "blur0", "gauss_blur_k"))
    assert base == 0
    assert len(_launches(d, lines, "blur1", "gauss_blur_k")) == base + 1
    assert len(_launches(d, lines, "blur2", "gauss_blur_k")) == base + 2
    assert len(_launches(d, lines, "yuyv", "gauss_blur_k")) == 2
    # YUYV frames with a blur stream: converted to BGR first (one conversion launch), then the blur, then the tile launch
    conv = _launches(d, lines, "yuyv_in_blur", "yuyv_to_bgr_k")
    assert len(conv) == 1 and len(_launches(d, lines, "yuyv_in_blur", "gauss_blur_k")) == 1
    assert not _launches(d, lines, "yuyv_in", "yuyv_to_bgr_k"), "YUYV frames without a blur stream are converted on load"
    # the grid of a blur launch covers its group only
    g = _launches(d, lines, "blur1", "gauss_blur_k")[0][4]
    assert g.startswith("g=") and g.endswith(",2"), g


def test_the_descriptor_ring_is_allocated_once(run):
    d, lines = run
    first = [l[1] for l in _span(d, lines, "dense") if l[0] == "affine"]
    assert "hipHostMalloc" in first                  # the descriptor ring, lazily on the first call
    first_ids = [l[1] for l in _span(d, lines, "ids") if l[0] == "affine"]
    assert first_ids.count("hipHostMalloc") == 1     # the id ring, on the first call that has ids
    for key in OK_CALLS[2:]:
        apis = [l[1] for l in _span(d, lines, key) if l[0] == "affine"]
        assert "hipHostMalloc" not in apis, key
    reused = [l[1] for k in ("ring_%d" % i for i in range(6)) for l in _span(d, lines, k) if l[0] == "affine"]
    assert "hipEventQuery" in reused


@pytest.mark.parametrize("key,words", [
    ("dup", ["ids[2] = 0", "repeats ids[0]"]),
    ("out_of_range", ["ids[1] = 4", "out of range"]),
    ("negative_n", ["n = -1", "negative"]),
    ("too_many", ["n = 5", "exceeds", "4 streams"]),
    ("settings_null", ["settings is NULL"]),
    ("batch_flip", ["flags 0x2", "yuyv / no-mask / yuyv-in"]),
    ("batch_bit5", ["flags 0x20", "yuyv / no-mask / yuyv-in"]),
    ("batch_blur", ["flags 0x700"]),
    ("stream_yuyv_bit", ["settings[1]", "flags 0x1", "flip / blur / filter-off"]),
    ("stream_bit6", ["settings[2]", "flags 0x42"]),
    ("even_blur", ["settings[2]", "blur size 8", "odd"]),
    ("big_blur", ["settings[0]", "blur size 33"]),
    ("off_even_blur", ["settings[1]", "blur size 4"]),
    ("null_bg", ["settings[3]", "d_bg is NULL"]),
    ("unaligned_bg", ["settings[3]", "not 4-byte aligned"]),
    ("out_is_frames", ["overlaps the frames"]),
    ("out_overlaps_bg", ["settings[1]", "overlaps the background"]),
    ("unaligned_out", ["fused mask + blend geometry"]),
    ("pending", ["pipelined composite is pending"]),
    ("odd_width_yuyv", ["YUYV output needs an even width"]),
    ("odd_width_yuyv_in", ["YUYV input needs an even capture width"]),
    ("width_not_4", ["fused mask + blend geometry"]),
    ("onmask", ["onmask"]),
    ("ex_bit5", ["unsupported flags 0x20"]),
    ("streams_bit5", ["unsupported flags 0x20"]),
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


@pytest.mark.parametrize("key", ["empty", "empty_ids"])
def test_an_empty_batch_is_a_no_op(run, key):
    d, lines = run
    assert d["calls"][key]["rc"] == 0
    assert _span(d, lines, key) == []


def test_header_and_binding_agree_on_the_new_call():
    from backscrub_amd import api
    names = {s[0] for s in api.SYMBOLS}
    hdr = open(os.path.join(ROOT, "include", "bsx.h")).read()
    assert "bsx_step_batch_mixed" in names and "BSX_API int bsx_step_batch_mixed(" in hdr
    assert "#define BSX_STREAM_FILTER_OFF 32u" in hdr and "typedef struct bsx_stream_setting" in hdr
    import ctypes
    assert ctypes.sizeof(api._StreamSetting) == 16


def test_step_mixed_refuses_bad_arguments_before_reaching_c():
    """a wrong-shaped background, a settings list of the wrong length, a missing background: BsxError before any library call"""
    torch = pytest.importorskip("torch")
    from backscrub_amd import api

    class Fake(api.MaskGen):
        def __init__(self):          # no context: validation happens before any library call
            self.width, self.height, self.device, self.n_streams, self.h = 8, 4, 0, 4, None

        def _n(self, frames, yuyv_in=False):
            return int(frames.shape[0])

        def _step_out(self, out, n, yuyv):
            pass

    mg = Fake()
    frames = torch.zeros((2, 4, 8, 3), dtype=torch.uint8)
    out = torch.zeros((2, 4, 8, 3), dtype=torch.uint8)
    S = api.StreamSetting
    with pytest.raises(api.BsxError, match="settings"):
        mg.step_mixed(frames, out, [S(bgblur=7)])
    with pytest.raises(api.BsxError, match="settings"):
        mg.step_mixed(frames, out, [S(bgblur=7)] * 3)
    with pytest.raises(api.BsxError, match=r"settings\[1\]\.bg"):
        mg.step_mixed(frames, out, [S(bgblur=7), S(bg=torch.zeros((4, 7, 3), dtype=torch.uint8))])
    with pytest.raises(api.BsxError, match=r"settings\[0\]: bg is required"):
        mg.step_mixed(frames, out, [S(flip_h=True), S(filter_off=True)])
    with pytest.raises(api.BsxError, match="ids"):
        mg.step_mixed(frames, out, [S(bgblur=7)] * 2, ids=[0])
