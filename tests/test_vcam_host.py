"""CPU-side checks of bsx_step_batch_vcam (the main loop at the virtual camera's geometry): the C ABI declares and exports it, the Python binding validates
its output tensor before reaching C, and its kernel compiles for gfx950 without scratch inside the image kernels' LDS budget."""
import os
import re
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def built():
    from backscrub_amd import build
    return build.build()


def test_header_declares_and_library_exports_the_vcam_step(built):
    import ctypes
    hdr = open(os.path.join(ROOT, "include", "bsx.h")).read()
    assert re.search(r"BSX_API int bsx_step_batch_vcam\(bsx_ctx\* ctx, const uint8_t\* d_frames, const uint8_t\* d_bg, size_t bg_frame_stride,\s*"
                     r"uint8_t\* d_out, int out_w, int out_h, int n, void\* stream, unsigned flags\);", hdr)
    assert hasattr(ctypes.CDLL(built), "bsx_step_batch_vcam")
    from backscrub_amd import api
    assert "bsx_step_batch_vcam" in {s[0] for s in api.SYMBOLS}


def test_step_vcam_rejects_a_bad_out_before_reaching_c(built, monkeypatch):
    """out_w / out_h come from out's shape and the C side writes n * out_h * out_w * (2 or 3) bytes there: wrong dtype, channel count, layout, an odd YUYV
    width or a host tensor must raise in Python, before any library call."""
    import torch
    from backscrub_amd import api

    class Fake(api.MaskGen):
        def __init__(self):          # no context: validation happens before any library call
            self.width, self.height, self.n_streams, self.device, self.h = 8, 4, 2, 0, None

    def no_c(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(api, "lib", no_c)
    mg = Fake()
    frames = torch.zeros((2, 4, 8, 3), dtype=torch.uint8)
    bg = torch.zeros((4, 8, 3), dtype=torch.uint8)
    bad = [(torch.zeros((2, 6, 10, 3), dtype=torch.float32), {}),
           (torch.zeros((2, 6, 10, 2), dtype=torch.uint8), {}),
           (torch.zeros((2, 6, 10, 3), dtype=torch.uint8), {"yuyv": True}),
           (torch.zeros((2, 6, 9, 2), dtype=torch.uint8), {"yuyv": True}),
           (torch.zeros((2, 6, 20, 3), dtype=torch.uint8)[:, :, ::2], {}),
           (torch.zeros((6, 10, 3), dtype=torch.uint8), {}),
           (torch.zeros((2, 0, 10, 3), dtype=torch.uint8), {}),
           (torch.zeros((2, 6, 10, 3), dtype=torch.uint8), {})]          # a host tensor
    for out, kw in bad:
        with pytest.raises(api.BsxError, match="out"):
            mg.step_vcam(frames, bg, out, **kw)


def test_vcam_kernel_has_no_scratch_and_fits_the_lds_budget():
    """Every instantiation of the vcam kernel: no spill, and at most 32 KiB of LDS (five workgroups per CU, like the other image kernels)."""
    from backscrub_amd import build
    if not os.path.exists(build.HIPCC):
        pytest.skip("hipcc not installed")
    src = os.path.join(ROOT, "backscrub_amd", "csrc", "kernels_img.hip")
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_regs.sh"), src, "vcam"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "compile failed" not in r.stdout, r.stdout[-500:] + r.stderr[-500:]
    rows = re.findall(r"^(\S*vcam\S*)\s+vgpr\+agpr\s+(\d+)\s+accum_offset\s+(\d+)\s+lds\s+(\d+)\s+scratch\s+(\d+)", r.stdout, flags=re.M)
    assert len(rows) == 4, r.stdout                                     # {LDS, direct} x {BGR, YUYV} frames
    for name, _, _, lds, scratch in rows:
        assert int(scratch) == 0, "%s spills %s bytes" % (name, scratch)
        assert int(lds) <= 32 * 1024, "%s: %s B of LDS" % (name, lds)
