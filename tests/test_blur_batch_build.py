"""bsx_gaussian_blur_bgr_batch without a GPU: blur_batch_k's compile-time resources against gauss_blur_k's (tools/kernel_regs.sh, the gfx950 assembly hipcc emits
here), the Python wrapper's refusals before the library is reached, and bsx_blur_item's layout in the header against the binding's.

The register rule (tests/test_geoms_yuyv_in_build.py): a gfx950 SIMD has 512 VGPRs per lane, handed out in blocks of 8, and holds at most 8 waves; `next_free_vgpr`
allows min(8, 512 // roundup8(n)) waves.  blur_batch_k is gauss_blur_k's body with eight tap-word counts behind one workgroup-uniform switch: its yardstick is the
parent's own kernel with the most tap words, gauss_blur_k<1, 9>, in the same survey."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "backscrub_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def _waves(vgprs):
    return min(8, 512 // ((vgprs + 7) // 8 * 8))


def test_kernel_resources():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_regs.sh"), os.path.join(CSRC, "kernels_img.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "compile failed" not in r.stdout, r.stdout[-500:] + r.stderr[-500:]
    row = re.compile(r"^(\S+)\s+vgpr\+agpr\s+(\d+)\s+accum_offset\s+(\d+)\s+lds\s+(\d+)\s+scratch\s+(\d+)")
    rows = {}
    for line in r.stdout.splitlines():
        m = row.match(line)
        if m:
            rows[m.group(1)] = dict(vgpr=int(m.group(2)), arch_vgpr=int(m.group(3)), lds=int(m.group(4)), scratch=int(m.group(5)))
    new = [v for k, v in rows.items() if "blur_batch_k" in k]
    assert len(new) == 1, [k for k in rows if "blur_batch_k" in k]
    new = new[0]
    gauss = {k: v for k, v in rows.items() if "gauss_blur_k" in k}
    assert len(gauss) == 24                                                # 3 modes x 8 tap-word counts, as before
    yard = [v for k, v in gauss.items() if "gauss_blur_kILi1ELi9E" in k]
    assert len(yard) == 1
    yard = yard[0]
    print("blur_batch_k: %d VGPRs (%d waves / SIMD), %d B LDS, %d B scratch; gauss_blur_k<1, 9>: %d VGPRs (%d waves / SIMD), %d B LDS" % (
        new["vgpr"], _waves(new["vgpr"]), new["lds"], new["scratch"], yard["vgpr"], _waves(yard["vgpr"]), yard["lds"]))
    assert _waves(64) == 8 and _waves(81) == 5 and _waves(96) == 5 and _waves(97) == 4
    assert new["scratch"] == 0
    assert new["lds"] <= max(v["lds"] for v in gauss.values())
    assert new["lds"] * 5 <= 160 * 1024                                    # five workgroups per CU still fit
    assert _waves(new["vgpr"]) >= _waves(yard["vgpr"]), "%d VGPRs allow %d waves per SIMD, gauss_blur_k<1, 9>'s %d allow %d" % (
        new["vgpr"], _waves(new["vgpr"]), yard["vgpr"], _waves(yard["vgpr"]))


def test_wrapper_refusals_before_the_library():
    import torch
    from backscrub_amd import api

    class Fake(api.MaskGen):
        def __init__(self):          # no context: validation happens before any library call
            self.width, self.height, self.n_streams, self.device, self.h = 8, 4, 4, 0, None

    mg = Fake()
    bgr = torch.zeros((4, 8, 3), dtype=torch.uint8)
    with pytest.raises(api.BsxError, match=r"srcs\[1\]"):
        mg.gaussian_blur_batch([bgr, torch.zeros((4, 8, 3), dtype=torch.float32)], 5)           # wrong dtype
    with pytest.raises(api.BsxError, match=r"srcs\[0\]"):
        mg.gaussian_blur_batch([torch.zeros((1, 4, 8, 3), dtype=torch.uint8)], 5)              # wrong rank
    with pytest.raises(api.BsxError, match=r"srcs\[0\]"):
        mg.gaussian_blur_batch([torch.zeros((4, 8, 4), dtype=torch.uint8)], 5)                 # last dimension 4
    with pytest.raises(api.BsxError, match=r"srcs\[0\]"):
        mg.gaussian_blur_batch([torch.zeros((4, 16, 3), dtype=torch.uint8)[:, ::2]], 5)        # not contiguous
    with pytest.raises(api.BsxError, match="1 ksizes for 2 images"):
        mg.gaussian_blur_batch([bgr, bgr], [5])
    with pytest.raises(api.BsxError, match=r"ksizes\[1\] = 4"):
        mg.gaussian_blur_batch([bgr, bgr], [5, 4])
    with pytest.raises(api.BsxError, match=r"ksizes\[0\] = 33"):
        mg.gaussian_blur_batch([bgr], 33)
    with pytest.raises(api.BsxError, match=r"out\[0\].*\[4,8,3\]"):
        mg.gaussian_blur_batch([bgr], 5, out=[torch.zeros((4, 8, 2), dtype=torch.uint8)])      # an out of the wrong shape
    with pytest.raises(api.BsxError, match="1 outputs for 2 images"):
        mg.gaussian_blur_batch([bgr, bgr], 5, out=[bgr.clone()])
    with pytest.raises(api.BsxError, match="5 images for a context of 4 streams"):
        mg.gaussian_blur_batch([bgr] * 5, 5)
    with pytest.raises(api.BsxError, match=r"srcs\[0\] is on cpu"):                           # right in every other respect: the device is checked last
        mg.gaussian_blur_batch([bgr], 5, out=[bgr.clone()])


def test_the_header_declares_the_item_as_the_binding_lays_it_out(tmp_path):
    from backscrub_amd import api
    hdr = open(os.path.join(ROOT, "include", "bsx.h")).read()
    m = re.search(r"typedef struct bsx_blur_item \{(.*?)\} bsx_blur_item;", hdr, re.S)
    assert m, "bsx.h declares no bsx_blur_item"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [re.sub(r"[^A-Za-z_0-9]", "", name.split()[-1]) for name in decl.split(",")]
    assert fields == [name for name, _t in api._BlurItem._fields_] == ["d_src", "d_dst", "w", "h", "ksize", "flags"]
    assert "BSX_API int bsx_gaussian_blur_bgr_batch(bsx_ctx* ctx, const bsx_blur_item* items, int n, void* stream);" in hdr
    assert [s for s in api.SYMBOLS if s[0] == "bsx_gaussian_blur_bgr_batch"] == [
        ("bsx_gaussian_blur_bgr_batch", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(api._BlurItem), ctypes.c_int, ctypes.c_void_p])]
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang") if subprocess.run(["sh", "-c", "command -v " + c], capture_output=True).returncode == 0), None)
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "item.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bsx.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(bsx_blur_item), offsetof(bsx_blur_item, d_src), offsetof(bsx_blur_item, d_dst),\n'
                   '         offsetof(bsx_blur_item, w), offsetof(bsx_blur_item, h), offsetof(bsx_blur_item, ksize), offsetof(bsx_blur_item, flags));\n  return 0;\n}\n')
    exe = tmp_path / "item"
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True, capture_output=True, text=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    B = api._BlurItem
    assert got == [ctypes.sizeof(B), B.d_src.offset, B.d_dst.offset, B.w.offset, B.h.offset, B.ksize.offset, B.flags.offset], got
    assert ctypes.sizeof(B) == 32
