"""bsx_step_batch_vcam_mixed on a box without a GPU: header, library and binding agree on the call; MaskGen.step_vcam_mixed refuses bad arguments before it reaches
the library; the new kernel compiles for gfx950 without scratch inside the image kernels' LDS budget; and the library's real host code, run against
tests/hip_stub/libhipstub.so by tests/hip_stub/drive_vcam_mixed.py (a context on device 1, the caller on device 0):
  * every accepted call returns 0, makes HIP calls on device 1 only, restores the caller's device, copies the descriptor table with hipMemcpyAsync behind a ring
    event, and makes exactly ONE resize-pass launch, ONE blur launch per distinct blur size and NO capture-size composite launch (no blending instantiation
    of the mask tile kernels, no blend*_k);
  * the descriptor ring is allocated once;
  * each refusal returns BSX_EINVAL with a message that names the position and value and enqueues no HIP call at all; n == 0 returns 0 and enqueues nothing."""
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


@pytest.fixture(scope="module")
def built():
    from backscrub_amd import build
    return build.build()


@pytest.fixture(scope="module")
def stub(built):
    src = os.path.join(STUB_DIR, "hip_stub.cpp")
    if not os.path.exists(STUB) or os.path.getmtime(STUB) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", STUB, src])
    return STUB


@pytest.fixture(scope="module")
def run(stub, tmp_path_factory):
    log = str(tmp_path_factory.mktemp("vcam_mixed") / "hip.log")
    env = dict(os.environ, LD_PRELOAD=stub, BSX_STUB_LOG=log, BSX_STUB_NDEV="2")
    W, H, n = 640, 480, 4
    r = subprocess.run([sys.executable, os.path.join(STUB_DIR, "drive_vcam_mixed.py"), model_path("lite"), str(W), str(H), str(n), "1"], env=env,
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


# ---- header, library, binding ---------------------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree_on_the_new_call(built):
    import ctypes
    from backscrub_amd import api
    hdr = open(os.path.join(ROOT, "include", "bsx.h")).read()
    assert re.search(r"BSX_API int bsx_step_batch_vcam_mixed\(bsx_ctx\* ctx, const int\* ids, const uint8_t\* d_frames, const bsx_stream_setting\* settings,\s*"
                     r"uint8_t\* d_out, int out_w, int out_h, int n, void\* stream, unsigned flags\);", hdr)
    assert hdr.count("typedef struct bsx_stream_setting") == 1          # the same struct, not a second one
    assert hasattr(ctypes.CDLL(built), "bsx_step_batch_vcam_mixed")
    from backscrub_amd import build
    assert hasattr(ctypes.CDLL(build.LIB_DBG), "bsx_step_batch_vcam_mixed")
    sym = {s[0]: s for s in api.SYMBOLS}["bsx_step_batch_vcam_mixed"]
    assert sym[1] is ctypes.c_int and len(sym[2]) == 10
    assert sym[2][1] == ctypes.POINTER(ctypes.c_int) and sym[2][3] == ctypes.POINTER(api._StreamSetting)


def test_step_vcam_mixed_refuses_bad_arguments_before_reaching_c(monkeypatch):
    """out_w / out_h come from out's shape and the C side writes n * out_h * out_w * (2 or 3) bytes there: a wrong dtype, channel count, layout, an odd YUYV width,
    too few frames or a host tensor raise in Python, and so do wrong frames, a settings list of the wrong length, a wrong-shaped or missing background and an ids
    list of the wrong length — all before any library call"""
    torch = pytest.importorskip("torch")
    from backscrub_amd import api

    class Fake(api.MaskGen):
        def __init__(self):          # no context: validation happens before any library call
            self.width, self.height, self.n_streams, self.device, self.h = 8, 4, 4, 0, None

    class OnDevice(Fake):            # host tensors stand in for device ones: the checks that need no device
        def _n(self, frames, yuyv_in=False):
            return int(frames.shape[0])

        def _vcam_out(self, out, yuyv):
            pass

    def no_c(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(api, "lib", no_c)
    mg = Fake()
    S = api.StreamSetting
    frames = torch.zeros((2, 4, 8, 3), dtype=torch.uint8)
    two = [S(bgblur=7), S(filter_off=True)]
    good = torch.zeros((2, 6, 10, 3), dtype=torch.uint8)
    bad_out = [(torch.zeros((2, 6, 10, 3), dtype=torch.float32), {}),
               (torch.zeros((2, 6, 10, 2), dtype=torch.uint8), {}),
               (torch.zeros((2, 6, 10, 3), dtype=torch.uint8), {"yuyv": True}),
               (torch.zeros((2, 6, 9, 2), dtype=torch.uint8), {"yuyv": True}),
               (torch.zeros((2, 6, 20, 3), dtype=torch.uint8)[:, :, ::2], {}),
               (torch.zeros((6, 10, 3), dtype=torch.uint8), {}),
               (torch.zeros((2, 0, 10, 3), dtype=torch.uint8), {}),
               (good, {})]                                                   # a host tensor
    for out, kw in bad_out:
        with pytest.raises(api.BsxError, match="out"):
            mg.step_vcam_mixed(frames, out, two, **kw)
    mg = OnDevice()
    with pytest.raises(api.BsxError, match="out holds 1 frames"):
        mg.step_vcam_mixed(frames, good[:1], two)
    with pytest.raises(api.BsxError, match="frames"):
        Fake._n(mg, torch.zeros((2, 4, 8, 3), dtype=torch.uint8), True)      # (the frame check the call makes: BGR-shaped frames announced as YUYV)
    with pytest.raises(api.BsxError, match="settings"):
        mg.step_vcam_mixed(frames, good, [S(bgblur=7)])
    with pytest.raises(api.BsxError, match="settings"):
        mg.step_vcam_mixed(frames, good, [S(bgblur=7)] * 3)
    with pytest.raises(api.BsxError, match=r"settings\[1\] is not"):
        mg.step_vcam_mixed(frames, good, [S(bgblur=7), {"bgblur": 7}])
    with pytest.raises(api.BsxError, match=r"settings\[1\]\.bg"):
        mg.step_vcam_mixed(frames, good, [S(bgblur=7), S(bg=torch.zeros((4, 7, 3), dtype=torch.uint8))])
    with pytest.raises(api.BsxError, match=r"settings\[1\]\.bg"):
        mg.step_vcam_mixed(frames, good, [S(bgblur=7), S(bg=torch.zeros((6, 10, 3), dtype=torch.uint8))])      # a vcam-size image: d_bg is capture-size
    with pytest.raises(api.BsxError, match=r"settings\[0\]: bg is required"):
        mg.step_vcam_mixed(frames, good, [S(flip_h=True), S(filter_off=True)])
    with pytest.raises(api.BsxError, match="ids"):
        mg.step_vcam_mixed(frames, good, two, ids=[0])


# ---- the kernel -----------------------------------------------------------------------------------------------------------------------------------------------
def test_the_new_kernel_has_no_scratch_and_fits_the_lds_budget():
    """every instantiation of vg_mixed_k, picked by its own name: no spill, at most 32 KiB of LDS; and the dense kernel's instantiations stay the four they were"""
    from backscrub_amd import build
    if not os.path.exists(build.HIPCC):
        pytest.skip("hipcc not installed")
    src = os.path.join(ROOT, "backscrub_amd", "csrc", "kernels_img.hip")
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_regs.sh"), src, "vg_mixed_k|vcam"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "compile failed" not in r.stdout, r.stdout[-500:] + r.stderr[-500:]
    rows = re.findall(r"^(\S*vg_mixed_k\S*)\s+vgpr\+agpr\s+(\d+)\s+accum_offset\s+(\d+)\s+lds\s+(\d+)\s+scratch\s+(\d+)", r.stdout, flags=re.M)
    assert len(rows) == 4, r.stdout                                     # {LDS, direct} x {BGR, YUYV} frames
    for name, _, _, lds, scratch in rows:
        assert "vcam" not in name, name
        assert int(scratch) == 0, "%s spills %s bytes" % (name, scratch)
        assert int(lds) <= 32 * 1024, "%s: %s B of LDS" % (name, lds)
    assert {int(lds) for _, _, _, lds, _ in rows} == {0, 32 * 1024}      # the staged form and the direct-tap form
    assert len(re.findall(r"^\S*vcam\S*\s+vgpr", r.stdout, flags=re.M)) == 4


# ---- the host code under the stub -----------------------------------------------------------------------------------------------------------------------------
OK_CALLS = ["dense", "ids", "blur0", "blur1", "blur2", "yuyv", "yuyv_in", "yuyv_in_blur", "unaligned_bg", "subset", "after_flush", "width_not_4",
            "width_not_4_yuyv_in"] + ["ring_%d" % i for i in range(6)]


def test_calls_run_on_the_contexts_device_only(run):
    d, lines = run
    for key in OK_CALLS + ["capture_size"]:
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
    for key in OK_CALLS[2:11]:                                               # (the first call of an output size uploads its table)
        apis = [l[1] for l in _span(d, lines, key) if l[0] == "affine"]
        assert "hipStreamSynchronize" not in apis and "hipDeviceSynchronize" not in apis and "hipEventSynchronize" not in apis, "%s synchronised the host" % key
    assert d["pipelined"] == [0, 0]


def test_one_resize_pass_launch_and_no_capture_size_composite(run):
    d, lines = run
    for key in OK_CALLS:
        span = [l[3] for l in _span(d, lines, key) if l[0] == "affine" and l[1] == "hipLaunchKernel"]
        passes = [k for k in span if "vg_mixed_k" in k]
        assert len(passes) == 1, (key, span)
        assert span[-1] == passes[0], "%s: the resize pass is not the last launch" % key
        for k in span:
            # (the masks themselves are made by the mask pipeline's mask-only launch, mask_tile_k<BLEND = false> or mask_upscale_blur_k<false>, as in the dense
            #  vcam step: that one writes the persistent masks and composites nothing)
            assert not re.search(r"mask_tile_kILb1|mask_upscale_blur_kILb1|blend\w*_k", k), "%s: a capture-size composite launch: %s" % (key, k)
            assert "resize_bgr" not in k and "flip_bgr" not in k and "vcam_blend_resize_k" not in k, (key, k)
        assert not [k for k in span if re.search(r"\d+yuyv_kE", k)], "%s: a separate YUYV pack" % key
    g = _launches(d, lines, "subset", "vg_mixed_k")[0][4]
    assert g == "g=56,2,1", g                                                # 7 x 8 tiles of 64 x 32, grid y = the batch's positions
    # YUYV frames are read by the pass itself (<.., true>), unless a blur stream needs them as BGR first
    assert "ILb0ELb1EE" in _launches(d, lines, "yuyv_in", "vg_mixed_k")[0][3]
    assert "ILb0ELb0EE" in _launches(d, lines, "yuyv_in_blur", "vg_mixed_k")[0][3]
    # the capture size is the mixed step: its ONE tile launch, and no resize pass
    assert not _launches(d, lines, "capture_size", "vg_mixed_k")
    assert len(_launches(d, lines, "capture_size", "mask_tile_k") + _launches(d, lines, "capture_size", "mask_upscale_blur_k")) == 1


def test_one_blur_launch_per_distinct_blur_size(run):
    d, lines = run
    assert len(_launches(d, lines, "blur0", "gauss_blur_k")) == 0
    assert len(_launches(d, lines, "blur1", "gauss_blur_k")) == 1
    assert len(_launches(d, lines, "blur2", "gauss_blur_k")) == 2
    assert len(_launches(d, lines, "yuyv", "gauss_blur_k")) == 2
    assert len(_launches(d, lines, "subset", "gauss_blur_k")) == 1
    conv = _launches(d, lines, "yuyv_in_blur", "yuyv_to_bgr_k")
    assert len(conv) == 1 and len(_launches(d, lines, "yuyv_in_blur", "gauss_blur_k")) == 1
    assert not _launches(d, lines, "yuyv_in", "yuyv_to_bgr_k"), "YUYV frames without a blur stream are converted on load"
    g = _launches(d, lines, "blur1", "gauss_blur_k")[0][4]
    assert g.startswith("g=") and g.endswith(",2"), g                        # the grid of a blur launch covers its group only


def test_the_descriptor_ring_is_allocated_once(run):
    d, lines = run
    first = [l[1] for l in _span(d, lines, "dense") if l[0] == "affine"]
    assert "hipHostMalloc" in first                  # the descriptor ring, lazily on the first call
    first_ids = [l[1] for l in _span(d, lines, "ids") if l[0] == "affine"]
    assert first_ids.count("hipHostMalloc") == 1     # the id ring, on the first call that has ids
    for key in OK_CALLS[2:11] + ["ring_%d" % i for i in range(6)] + ["capture_size"]:
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
    ("batch_flip", ["flags 0x2", "yuyv / yuyv-in"]),
    ("batch_bit5", ["flags 0x20", "yuyv / yuyv-in"]),
    ("batch_blur", ["flags 0x700"]),
    ("no_mask", ["flags 0x8", "no-mask"]),
    ("no_mask_capture_size", ["flags 0x8", "no-mask"]),
    ("stream_yuyv_bit", ["settings[1]", "flags 0x1", "flip / blur / filter-off"]),
    ("stream_bit6", ["settings[2]", "flags 0x42"]),
    ("even_blur", ["settings[2]", "blur size 8", "odd"]),
    ("big_blur", ["settings[0]", "blur size 33"]),
    ("off_even_blur", ["settings[1]", "blur size 4"]),
    ("null_bg", ["settings[3]", "d_bg is NULL"]),
    ("zero_width", ["output size 0 x 240"]),
    ("negative_height", ["output size 426 x -3"]),
    ("odd_yuyv_out", ["YUYV output needs an even width", "out_w = 425"]),
    ("out_is_frames", ["overlaps the frames"]),
    ("out_inside_frames", ["overlaps the frames"]),
    ("out_overlaps_bg", ["settings[1]", "overlaps the background"]),
    ("null_frames", ["null buffer"]),
    ("pending", ["pipelined composite is pending"]),
    ("pending_empty", ["pipelined composite is pending"]),
    ("odd_width_yuyv_in", ["YUYV input needs an even capture width", "width = 641"]),
    ("width_not_4_capture_size", ["fused mask + blend geometry"]),
])
def test_refusals_name_the_position_and_value_and_enqueue_nothing(run, key, words):
    d, lines = run
    c = d["calls"][key]
    assert c["rc"] == BSX_EINVAL, c
    assert "bsx_step_batch_vcam_mixed" in c["error"], c["error"]
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
