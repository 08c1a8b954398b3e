"""BSX_STREAM_YUYV_IN without a GPU: the bit's value in the header and the binding, the four per-format kernels in the gfx950 code objects of both libraries, and
their resources against the two instantiations whose bodies each of them joins (tools/kernel_regs.sh, read as tests/test_geoms_host.py reads it).

The register rule.  A gfx950 SIMD has 512 VGPRs per lane, handed out in blocks of 8, and holds at most 8 waves; a kernel's `next_free_vgpr` (architectural +
accumulation registers) therefore allows min(8, 512 // roundup8(n)) waves.  A per-format kernel chooses per workgroup between the YUYV and the BGR inclusion of
one body, so its allocation is the larger of the two: it may not allow fewer waves than the worse of the existing per-geometry kernel (the BGR body, per position)
and the dense / mixed YUYV instantiation (the YUYV body, per launch).  The counts are printed before they are asserted."""
import os
import re
import struct
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "backscrub_amd", "csrc")
# new kernel -> (the per-geometry kernel, the dense / mixed YUYV instantiations) whose bodies it joins; needles of mangled names
JOINS = {
    "prep_geoms_fmt_kILi1E": ("prep_geoms_kILi1E", ["prep_fused_kILi1ELb1ELb1E"]),
    "prep_geoms_fmt_kILi2E": ("prep_geoms_kILi2E", ["prep_fused_kILi2ELb1ELb1E"]),
    "prep_geoms_fmt_kILi3E": ("prep_geoms_kILi3E", ["prep_fused_kILi3ELb1ELb1E"]),
    "mask_tile_geoms_fmt_k": ("mask_tile_geoms_kE", ["mask_tile_kILb1ELb1ELb0ELb0ELb1E"]),
    "outside_roi_geoms_fmt_k": ("outside_roi_geoms_kE", ["outside_roi_mixed_kE"]),
    "vg_geoms_fmt_k": ("vg_geoms_kI", ["vg_mixed_kILb0ELb1E", "vg_mixed_kILb1ELb1E"]),
}


def test_the_bit_is_64_in_the_header_and_the_binding():
    from backscrub_amd import api
    hdr = open(os.path.join(ROOT, "include", "bsx.h")).read()
    assert re.search(r"^#define BSX_STREAM_YUYV_IN 64u$", hdr, re.M)
    assert api.BSX_STREAM_YUYV_IN == 64
    assert api.StreamSetting(yuyv_in=True).flags() & 64
    assert api.StreamSetting(yuyv_in=True, flip_h=True, filter_off=True).flags() == 64 | 32 | 2
    assert api.StreamSetting().flags() == 0 and not api.StreamSetting(flip_v=True, filter_off=True).flags() & 64
    assert issubclass(api.BsxFrameFormatError, ValueError) and issubclass(api.BsxFrameFormatError, api.BsxError)
    kh = open(os.path.join(CSRC, "kernels.hpp")).read()
    assert "constexpr unsigned kGeomYuyvIn = 64u;" in kh and "static_assert(sizeof(GeomDesc) == 48" in kh


def _gfx950_symbols(lib):
    """names of the FUNC symbols of every gfx950 code object bundled into the library (clang offload bundles: magic, entry count, then offset / size / triple per
    entry; the entries are ELF files)"""
    b = open(lib, "rb").read()
    magic, names, objects = b"__CLANG_OFFLOAD_BUNDLE__", set(), 0
    for m in re.finditer(magic, b):
        base = m.start()
        (n,) = struct.unpack_from("<Q", b, base + len(magic))
        p = base + len(magic) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", b, p)
            triple = b[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if "gfx950" not in triple or size == 0:
                continue
            elf = b[base + off:base + off + size]
            assert elf[:4] == b"\x7fELF" and elf[4] == 2 and struct.unpack_from("<H", elf, 18)[0] == 224, "not a 64-bit AMDGPU ELF: " + triple
            objects += 1
            shoff, = struct.unpack_from("<Q", elf, 0x28)
            shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
            for i in range(shnum):
                sh = struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize)
                if sh[1] != 2:                                              # SHT_SYMTAB
                    continue
                stroff = struct.unpack_from("<IIQQQQIIQQ", elf, shoff + sh[6] * shentsize)[4]
                for k in range(sh[5] // 24):
                    st_name, st_info = struct.unpack_from("<IB", elf, sh[4] + 24 * k)
                    if st_info & 15 == 2:                                   # STT_FUNC
                        end = elf.index(b"\0", stroff + st_name)
                        names.add(elf[stroff + st_name:end].decode())
    return names, objects


def test_the_kernels_are_in_both_libraries():
    from backscrub_amd import build
    build.build()
    for lib in (build.LIB, build.LIB_DBG):
        names, objects = _gfx950_symbols(lib)
        assert objects >= 4, (lib, objects)
        for needle in JOINS:
            assert [n for n in names if needle in n], "%s: no %s in the gfx950 code objects" % (os.path.basename(lib), needle)
        # ... next to the kernels a call of BGR items keeps launching
        for needle in ("prep_geoms_kILi2E", "mask_tile_geoms_kE", "outside_roi_geoms_kE", "vg_geoms_kI", "mask_geoms_kI", "tile_class_geoms_kE"):
            assert [n for n in names if needle in n], (lib, needle)


def _survey():
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_regs.sh"), os.path.join(CSRC, "kernels_img.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "compile failed" not in r.stdout, r.stdout[-500:] + r.stderr[-500:]
    row = re.compile(r"^(\S+)\s+vgpr\+agpr\s+(\d+)\s+accum_offset\s+(\d+)\s+lds\s+(\d+)\s+scratch\s+(\d+)")
    rows = {}
    for line in r.stdout.splitlines():
        m = row.match(line)
        if m:
            rows[m.group(1)] = dict(vgpr=int(m.group(2)), arch_vgpr=int(m.group(3)), lds=int(m.group(4)), scratch=int(m.group(5)))
    return rows


def _waves(vgprs):
    return min(8, 512 // ((vgprs + 7) // 8 * 8))


def test_resources_of_the_per_format_kernels():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not installed")
    rows = _survey()

    def one(needle):
        hit = [(k, v) for k, v in rows.items() if needle in k]
        assert len(hit) == 1, (needle, [k for k, _ in hit])
        return hit[0][1]
    assert _waves(64) == 8 and _waves(65) == 7 and _waves(81) == 5 and _waves(128) == 4
    tile_lds = max(v["lds"] for k, v in rows.items() if "mask_tile_kI" in k)
    failures = []
    for new, (geom, dense) in JOINS.items():
        r, parts = one(new), [one(geom)] + [one(d) for d in dense]
        floor = min(_waves(p["vgpr"]) for p in parts)
        print("%-24s %3d VGPRs (%d waves / SIMD), %5d B LDS, %d B scratch; joins %s -> at least %d waves" % (
            new, r["vgpr"], _waves(r["vgpr"]), r["lds"], r["scratch"], ", ".join("%d VGPRs" % p["vgpr"] for p in parts), floor))
        if r["scratch"]:
            failures.append("%s spills %d bytes" % (new, r["scratch"]))
        if _waves(r["vgpr"]) < floor:
            failures.append("%s: %d VGPRs allow %d waves per SIMD, the bodies it joins allow %d" % (new, r["vgpr"], _waves(r["vgpr"]), floor))
        if r["lds"] > max(p["lds"] for p in parts):
            failures.append("%s: %d B of LDS, above both bodies it joins (%s)" % (new, r["lds"], [p["lds"] for p in parts]))
    assert one("mask_tile_geoms_fmt_k")["lds"] <= tile_lds, "the tile form's LDS is above mask_tile_k's %d" % tile_lds
    assert not failures, failures
    # the counts other tests pin are unchanged: the new names match none of their needles
    for needle, count in (("prep_geoms_k", 3), ("mask_tile_geoms_k", 1), ("outside_roi_geoms_k", 1), ("vg_geoms_k", 1), ("vg_mixed_k", 4), ("prep_fused_kI", 9),
                          ("mask_tile_kI", 9)):
        assert len([k for k in rows if needle in k]) == count, needle
