"""bsx_resize_surfaces_batch without a GPU:
  * header, both libraries and the binding agree on the symbol; ctypes' bsx_resize_surface_item has the size and offsets of the struct compiled from the header;
  * the header comment states the contract;
  * MaskGen.resize_surfaces validates its arguments before the library is reached, the device last;
  * resize_surfaces_k's compile-time resources (tools/kernel_regs.sh, the gfx950 assembly hipcc emits here) beside resize_bgr_batch_k's of the same build: one
    instance, no scratch, no LDS, and at least half that kernel's waves per SIMD — it holds 16 converted taps where the yardstick holds 16 loaded ones.

The register rule (tests/test_blur_batch_build.py): a gfx950 SIMD has 512 VGPRs per lane, handed out in blocks of 8, and holds at most 8 waves; `next_free_vgpr`
allows min(8, 512 // roundup8(n)) waves."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

SYM = "bsx_resize_surfaces_batch"
CSRC = os.path.join(ROOT, "backscrub_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
FIELDS = ["d_y", "d_uv", "d_dst", "pitch_y", "pitch_uv", "sw", "sh", "dw", "dh", "flags", "reserved"]
LDS_DECLARED = 0                # resize_surfaces_k stages nothing


def _waves(vgprs):
    return min(8, 512 // ((vgprs + 7) // 8 * 8))


def test_header_libraries_and_binding_agree_on_the_symbol(tmp_path):
    from backscrub_amd import api, build
    build.build()
    C = ctypes
    hdr = open(os.path.join(ROOT, "include", "bsx.h")).read()
    m = re.search(r"^BSX_API int %s\(([^)]*)\);" % SYM, hdr, re.M)
    assert m, "the header does not declare %s" % SYM
    assert re.sub(r"\s+", " ", m.group(1)) == "bsx_ctx* ctx, const bsx_resize_surface_item* items, int n, void* stream"
    assert [s for s in api.SYMBOLS if s[0] == SYM] == [(SYM, C.c_int, [C.c_void_p, C.POINTER(api._ResizeSurfaceItem), C.c_int, C.c_void_p])]
    assert callable(getattr(api.MaskGen, "resize_surfaces", None))
    # the version script exports the C ABI by its prefix: the symbol must be in the dynamic table of both builds
    for lib in (build.LIB, build.LIB_DBG):
        names = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout.split()
        assert SYM in names, lib
    # the item: the fields the header names, in the binding's order; the struct compiled from the header
    m = re.search(r"typedef struct bsx_resize_surface_item \{(.*?)\} bsx_resize_surface_item;", hdr, re.S)
    assert m, "bsx.h declares no bsx_resize_surface_item"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            fields += [re.sub(r"[^A-Za-z_0-9]", "", name.split()[-1]) for name in decl.strip().split(",")]
    B = api._ResizeSurfaceItem
    assert fields == [name for name, _t in B._fields_] == FIELDS
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bsx.h"\nint main(void) { printf("%zu", sizeof(bsx_resize_surface_item));\n' +
                   "".join('  printf(" %%zu", offsetof(bsx_resize_surface_item, %s));\n' % f for f in FIELDS) + '  printf("\\n"); return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe, str(src)])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert [C.sizeof(B)] + [getattr(B, f).offset for f in FIELDS] == got == [56, 0, 8, 16, 24, 28, 32, 36, 40, 44, 48, 52]


def test_the_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "bsx.h")).read()
    at = hdr.index("Video backgrounds from a decoder")
    text = re.sub(r"\s*\n \*\s*", " ", hdr[at:hdr.index("typedef struct bsx_resize_surface_item")])
    for phrase in ("app/background.cc:181-190", "bsx_nv12_to_bgr(d_y, pitch_y, d_uv, pitch_uv, sw, sh, 1, tmp)", "bsx_resize_bgr(tmp, sw, sh, d_dst, dw, dh, 1)",
                   "proper INTER_LINEAR", "the copy, where sw == dw && sh == dh", "the 2x2 area mean, where both scales are exactly 2", "UV[y >> 1][x & ~1 ..]",
                   "the integers of bsx_yuyv_to_bgr", "every tap is converted first", "No BGR copy of the surface exists anywhere",
                   "Bytes [sw, pitch) of a row are never read", "nothing is read beyond the last row", "one launch", "BSX_MAX_GEOMS distinct (dw, dh) pairs",
                   "any number of distinct source sizes", "items is a HOST array", "n == 0 returns 0 and enqueues nothing", "the same surface may appear in several items",
                   "works on every kind of context", "a non-zero reserved", "a plane of 2 GiB or more", "dw * dh * 3 >= 2^31", "a ninth distinct destination size",
                   "its own included", "byte sw of its last row", "BSX_EDEVICE", "A refused call changes nothing",
                   "Out of scope: BGR sources in this call (bsx_resize_bgr_batch serves them), an NV12 or YUYV destination",
                   "a bsx_background object that holds surfaces", "inside the step's own resize pass", "P010 and I420"):
        assert phrase in text, phrase


def test_wrapper_refusals_before_the_library():
    torch = pytest.importorskip("torch")
    from backscrub_amd import api

    host = []

    class Fake(api.MaskGen):
        """no context (h is None: a library call would fail loudly); host tensors count as on the device, but for the ones listed in `host`"""
        def __init__(self):
            self.width, self.height, self.n_streams, self.device, self.h = 8, 4, 4, 0, None

        def _on_device(self, t):
            return not any(t is h for h in host)

    def u8(*shape):
        return torch.zeros(shape, dtype=torch.uint8)

    def surface(w, h, pitch_y=None, pitch_uv=None):
        py, puv = pitch_y or (w + 3) // 4 * 4, pitch_uv or (w + 3) // 4 * 4
        buf = u8(py * h + puv * (h // 2) + 64)
        off = (-buf.data_ptr()) % 4
        return (torch.as_strided(buf, (h, w), (py, 1), off), torch.as_strided(buf, (h // 2, w), (puv, 1), off + py * h))
    mg = Fake()
    sf, big = surface(8, 4, 16, 12), surface(12, 6)
    with pytest.raises(api.BsxError, match="5 surfaces for a context of 4 streams"):
        mg.resize_surfaces([sf] * 5, (5, 3))
    with pytest.raises(api.BsxError, match="1 sizes for 2 surfaces"):
        mg.resize_surfaces([sf, big], [(5, 3)])
    with pytest.raises(api.BsxError, match="3 sizes for 2 surfaces"):
        mg.resize_surfaces([sf, big], [(5, 3)] * 3)
    with pytest.raises(api.BsxError, match=r"sizes\[1\] must be a pair \(w, h\) of integers"):
        mg.resize_surfaces([sf, big], [(5, 3), (5, 3, 3)])
    with pytest.raises(api.BsxError, match=r"sizes\[0\] must be a pair \(w, h\) of integers"):
        mg.resize_surfaces([sf, big], [(5.0, 3), (5, 3)])
    with pytest.raises(api.BsxError, match=r"sizes\[1\] = 0 x 3 is not positive"):
        mg.resize_surfaces([sf, big], [(5, 3), (0, 3)])
    with pytest.raises(api.BsxError, match=r"sizes\[0\] = 5 x -2 is not positive"):
        mg.resize_surfaces([sf], (5, -2))
    with pytest.raises(api.BsxError, match=r"surfaces\[1\] must be a pair \(y, uv\)"):
        mg.resize_surfaces([sf, sf[0]], (5, 3))
    with pytest.raises(api.BsxError, match=r"surfaces\[0\]: NV12 needs an even width and height \(y is 13 x 6\)"):
        mg.resize_surfaces([surface(13, 6, 16, 16)], (5, 3))
    with pytest.raises(api.BsxError, match=r"surfaces\[1\]: NV12 needs an even width and height \(y is 12 x 7\)"):
        mg.resize_surfaces([sf, (u8(7, 12), u8(3, 12))], (5, 3))
    with pytest.raises(api.BsxError, match=r"surfaces\[0\]: uv must be \[2, 8\] for a y of \[4, 8\] \(it is \[4, 8\]\)"):
        mg.resize_surfaces([(sf[0], u8(4, 8))], (5, 3))
    with pytest.raises(api.BsxError, match=r"surfaces\[0\]: the pitch of y, 8, is below out_w = 12"):
        mg.resize_surfaces([(torch.as_strided(u8(256), (6, 12), (8, 1)), big[1])], (5, 3))
    with pytest.raises(api.BsxError, match=r"surfaces\[0\]: the pitch of uv, 6, is not a multiple of 4"):
        mg.resize_surfaces([(u8(4, 8)[:, :6], u8(2, 6))], (5, 3))
    with pytest.raises(api.BsxError, match=r"surfaces\[0\]: y has an inner stride of 2"):
        mg.resize_surfaces([(u8(6, 24)[:, ::2], big[1])], (5, 3))
    with pytest.raises(api.BsxError, match=r"surfaces\[0\]: y must be a non-empty uint8 tensor of two dimensions \(it is torch.float32 \(4, 8\)\)"):
        mg.resize_surfaces([(sf[0].to(torch.float32), sf[1])], (5, 3))
    base = u8(6 * 16 + 8)
    o = (-base.data_ptr()) % 4 + 2
    with pytest.raises(api.BsxError, match=r"surfaces\[1\]: y at 0x[0-9a-f]+ is not 4-byte aligned"):
        mg.resize_surfaces([sf, (torch.as_strided(base, (6, 12), (16, 1), o), big[1])], (5, 3))
    with pytest.raises(api.BsxError, match="1 outputs for 2 surfaces"):
        mg.resize_surfaces([sf, big], (5, 3), out=[u8(3, 5, 3)])
    with pytest.raises(api.BsxError, match=r"out\[1\] must be a contiguous uint8 tensor \[7,9,3\]"):
        mg.resize_surfaces([sf, big], [(5, 3), (9, 7)], out=[u8(3, 5, 3), u8(9, 7, 3)])       # w and h changed places
    with pytest.raises(api.BsxError, match=r"out\[0\] must be a contiguous uint8 tensor \[3,5,3\]"):
        mg.resize_surfaces([sf], (5, 3), out=[u8(3, 10, 3)[:, ::2]])                           # not contiguous
    with pytest.raises(api.BsxError, match=r"out\[0\] must be a contiguous uint8 tensor \[3,5,3\]"):
        mg.resize_surfaces([sf], (5, 3), out=[torch.zeros((3, 5, 3), dtype=torch.float32)])
    # right in every other respect: the device is checked last — behind a fault of a later surface, and of an output
    uv_host = u8(2, 8)
    host.append(uv_host)
    with pytest.raises(api.BsxError, match=r"surfaces\[1\]: NV12 needs an even width"):
        mg.resize_surfaces([(sf[0], uv_host), surface(13, 6, 16, 16)], (5, 3))
    with pytest.raises(api.BsxError, match=r"out\[0\] must be"):
        mg.resize_surfaces([(sf[0], uv_host)], (5, 3), out=[u8(3, 5, 2)])
    with pytest.raises(api.BsxError, match=r"surfaces\[0\]: uv is on cpu, not on the context's cuda:0"):
        mg.resize_surfaces([(sf[0], uv_host)], (5, 3), out=[u8(3, 5, 3)])
    dst = u8(3, 5, 3)
    host.append(dst)
    with pytest.raises(api.BsxError, match=r"out\[0\] is on cpu, not on the context's cuda:0"):
        mg.resize_surfaces([sf], (5, 3), out=[dst])


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
    new = [v for k, v in rows.items() if "resize_surfaces_k" in k]
    assert len(new) == 1, [k for k in rows if "resize_surfaces_k" in k]
    new = new[0]
    yard = [v for k, v in rows.items() if "resize_bgr_batch_k" in k]
    assert len(yard) == 1
    yard = yard[0]
    print("resize_surfaces_k: %d VGPRs (%d waves / SIMD), %d B LDS, %d B scratch; resize_bgr_batch_k: %d VGPRs (%d waves / SIMD), %d B LDS, %d B scratch" % (
        new["vgpr"], _waves(new["vgpr"]), new["lds"], new["scratch"], yard["vgpr"], _waves(yard["vgpr"]), yard["lds"], yard["scratch"]))
    assert _waves(64) == 8 and _waves(81) == 5 and _waves(96) == 5 and _waves(97) == 4
    assert new["scratch"] == 0
    assert new["lds"] <= LDS_DECLARED
    assert 2 * _waves(new["vgpr"]) >= _waves(yard["vgpr"]), "%d VGPRs allow %d waves per SIMD, resize_bgr_batch_k's %d allow %d" % (
        new["vgpr"], _waves(new["vgpr"]), yard["vgpr"], _waves(yard["vgpr"]))
