"""k2's staged weights (csrc/segments.hpp: SegStage / seg_k2_stage, csrc/kernels_seg.hip: seg_k2_k) — what can be checked without a GPU.

seg_k2_k keeps the 1x1 expand's weight tile of the running channel group in LDS, double-buffered, the next group's on its way while this one computes (form >= 1),
and copies the depthwise weights of all groups into LDS with its first loads (form 2), so the expand loop never waits for a global round trip in front of a use.
The planner takes the largest form that keeps k2's workgroups per CU: min(floor(160 KiB / LDS bytes), 6) — 6 is the kernel's waves per SIMD (80 registers), one
wave of every workgroup on each SIMD."""
import os
import re
import subprocess

import pytest

from conftest import ROOT, model_path
from seg_text import seg_kernel_text

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "backscrub_amd", "csrc")
LDS_CU = 160 * 1024
K2_WAVES = 6


@pytest.fixture(scope="module")
def api():
    from backscrub_amd import api as a
    a.lib()
    return a


def k2_constants(src):
    blk = src[src.index("constexpr SegK2 kSegK2 = [] {"):]
    blk = blk[:blk.index("return t; }();")]
    return {k: int(v) for k, v in re.findall(r"t\.([\w.\[\]]+) = (-?\d+)(?:ll|u)?;", blk)}


def wgs_per_cu(lds_bytes, cap=LDS_CU):
    return min(cap // lds_bytes, K2_WAVES)


@pytest.fixture(scope="module")
def compiled(api, tmp_path_factory):
    """model key -> (specialised source, its assembly for gfx950), compiled once"""
    out = {}
    for key in ("lite", "full", "mlkit"):
        src = api.model_seg_source(model_path(key))
        p = tmp_path_factory.mktemp("k2_" + key) / "seg.hip"
        p.write_text(src)
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S", "-o", str(p) + ".s", str(p)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        out[key] = (src, open(str(p) + ".s").read())
    return out


@pytest.mark.parametrize("key", ["lite", "full", "mlkit"])
def test_the_staged_form_keeps_the_workgroups_per_cu(api, key, compiled):
    src, _ = compiled[key]
    k = k2_constants(src)
    assert k["wst.form"] == 2, "the shipped models have room for both parts"
    total, staged = 4 * k["lds_floats"], 4 * k["wst.floats"]
    assert wgs_per_cu(total) == wgs_per_cu(total - staged) == K2_WAVES
    assert k["wst.off"] + k["wst.floats"] == k["lds_floats"] and k["wst.off"] % 4 == 0
    # the block lies behind both tiles and behind the gate prologue's staging area (which aliases the first tile)
    tiles = 2 * (2 * k["TR"] + 1) * k["rw"] * 16
    hdr = open(os.path.join(CSRC, "segments.hpp")).read()
    scratch = int(re.search(r"constexpr int kSegScratchFloats = (\d+);", hdr).group(1))
    gate = eval(re.search(r"constexpr int kSegGateStageFloats = ([^;]+);", hdr).group(1))                  # noqa: S307 — "512 + 2 * (32 * 32 + 32)"
    assert k["wst.off"] == scratch + max(tiles, gate)
    # bsx_model_describe names the form and the bytes on k2's line
    line = [l for l in api.model_describe(model_path(key)).splitlines() if l.startswith("segment k2")][0]
    assert "(weights staged: form %d, %d B)" % (k["wst.form"], staged) in line and "LDS %.1f KiB" % (total / 1024) in line


@pytest.mark.parametrize("key", ["lite", "full", "mlkit"])
def test_the_specialised_source_carries_the_form_and_compiles_within_k2s_budget(key, compiled):
    """0 B of scratch and at most 80 registers (6 waves per SIMD).  The segment kernels take their LDS as the launch's dynamic allocation (lds_floats * 4 bytes,
    launch_seg_k2), so the code object's own LDS size is 0; that the kernel's carve ends exactly where the plan's byte count ends is a static_assert of the
    specialised source, evaluated by this compilation."""
    src, asm = compiled[key]
    k = k2_constants(src)
    assert "t.wst.form = %d; t.wst.off = %d; t.wst.floats = %d; t.wst.stride = %d;" % (k["wst.form"], k["wst.off"], k["wst.floats"], k["wst.stride"]) in src
    assert "d.wst.off + d.wst.floats == d.lds_floats" in src and "static_assert(d.wst.form == 0 ||" in src
    blk = asm[asm.index(".amdhsa_kernel bsx_seg_k2"):]
    blk = blk[:blk.index(".end_amdhsa_kernel")]
    vg = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", blk).group(1))
    sc = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", blk).group(1))
    lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", blk).group(1))
    assert sc == 0 and vg <= 80 and lds == 0, (vg, sc, lds)
    launch = seg_kernel_text()
    assert "seg_launch(fn, seg_k2_instance(h16), d.tiles_y * d.tiles_x, n, (size_t)d.lds_floats * sizeof(float), s, args)" in launch
    # the expand loop reads its 1x1 tiles and depthwise weights from LDS: what is left of global loads is the b0 operands (<= 6), the first copies (3), pw_a's
    # tile + bias (5) and the next group's piece (tile or bias lanes: 2 per group but the last); form 0 has 10 depthwise loads per group alone
    body = asm[asm.index("bsx_seg_k2:"):asm.index(".amdhsa_kernel bsx_seg_k2")]
    ngrp = (k["dw.C"] + 15) // 16
    gate = body[:body.index("s_barrier")]                             # the gate prologue's own loads sit in front of its first barrier
    rest = body[body.index("s_barrier"):]
    assert len(re.findall(r"^\s+global_load_dwordx4 ", rest, re.M)) <= 2 * (ngrp - 1), "weights are still fetched from global memory inside the expand loop"
    assert len(re.findall(r"^\s+ds_read2?_b32 ", rest, re.M)) >= 2 * ngrp and len(re.findall(r"^\s+global_load_dwordx4 ", gate, re.M)) >= 3


# ---- bank model (MI355X LDS: ds_read_b32 = two groups of 32 lanes, bank = dword address mod 32; ds_read_b128 = four groups of 16 lanes over 16-byte slots
#      modulo 16; ds_write_b128 = eight groups of eight consecutive lanes over eight slots) — the same model as tests/test_lds_layouts.py
G32 = [list(range(0, 32)), list(range(32, 64))]
G128 = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
G128 = G128 + [[l + 32 for l in g] for g in G128]
W128 = [list(range(8 * k, 8 * k + 8)) for k in range(8)]


def cycles(groups, unit, nslots, addr_of_lane, active=lambda l: True):
    """LDS-array cycles of one wave instruction; addr_of_lane in floats, unit = floats per bank slot"""
    tot = 0
    for grp in groups:
        slots = {}
        for l in grp:
            if active(l):
                a = addr_of_lane(l)
                assert a % unit == 0
                slots.setdefault((a // unit) % nslots, set()).add(a)
        tot += max([len(v) for v in slots.values()] + [1])
    return tot


@pytest.mark.parametrize("key", ["lite", "full", "mlkit"])
def test_the_staged_reads_and_the_copies_are_conflict_free(key, compiled):
    src, _ = compiled[key]
    k = k2_constants(src)
    kern = seg_kernel_text()
    # the kernel's own index expressions
    read, store = "(4 * g + r) * st.stride + li", "(tid & 15) * st.stride + 4 * (tid >> 4)"
    assert "wr[r] = tb[%s];" % read in kern and "bias_b = ld4(tb + st.bias_off + cq4);" in kern and "const float* tb = sw + (grp & 1) * st.buf_floats;" in kern
    assert "wd[k] = ldv(sw + st.dw_off + k * C + ch);" in kern and "if (tid < 64) st4(dst + %s, v);" % store in kern
    read_at = eval("lambda g, r, li, stride: " + read.replace("st.stride", "stride"))                    # noqa: S307
    store_at = eval("lambda tid, stride: " + store.replace("st.stride", "stride"))                        # noqa: S307
    stride, off, buf = k["wst.stride"], k["wst.off"], k["wst.buf_floats"]
    assert stride % 8 == 4 and stride >= 16 and k["wst.bias_off"] == 16 * stride and buf == 16 * stride + 16
    for b in (0, 1):
        for r in range(4):
            lane = lambda l, s=stride: off + b * buf + read_at(l >> 4, r, l & 15, s)
            assert cycles(G32, 1, 32, lane) == 2                                                           # conflict-free: one cycle per group of 32 lanes
            assert cycles(G32, 1, 32, lambda l: lane(l, 16)) == 4                                          # a dense tile: 2-way
            assert cycles(G32, 1, 32, lambda l: lane(l, k["pw_b.cout_pad"])) == 4                          # the weights' own row length: 2-way
        assert cycles(G128, 4, 16, lambda l: off + b * buf + k["wst.bias_off"] + 4 * (l >> 4)) == 4        # bias: one quad per row of 16 lanes (broadcast)
        # the copy of a tile (ds_write_b128, wave 0): every cell once, eight consecutive lanes on eight slots
        cells = sorted(store_at(t, stride) for t in range(64))
        assert cells == sorted(row * stride + 4 * p for row in range(16) for p in range(4))
        assert cycles(W128, 4, 8, lambda l: off + b * buf + store_at(l, stride)) == 8
    # form 2's depthwise reads: lane = (pixel l >> 2, quad l & 3), channel 16 grp + 4 quad; and the copy (lane t: piece t)
    C = k["dw.C"]
    assert k["wst.dw_off"] == 2 * buf and k["wst.dwb_off"] == k["wst.dw_off"] + 9 * C and k["wst.floats"] == k["wst.dwb_off"] + C
    for grp in range((C + 15) // 16):
        for tap in range(10):                                                                              # nine taps + the bias row (dwb_off = dw_off + 9 C)
            assert cycles(G128, 4, 16, lambda l: off + k["wst.dw_off"] + tap * C + 16 * grp + 4 * (l & 3), lambda l: 16 * grp + 4 * (l & 3) < C) == 4
    for wave in range(4):
        assert cycles(W128, 4, 8, lambda l: off + k["wst.dw_off"] + 4 * (64 * wave + l), lambda l: 4 * (64 * wave + l) < 9 * C) == 8


def test_the_planner_falls_back_form_by_form_as_the_budget_shrinks(tmp_path):
    """seg_k2_stage compiled from the header itself: form 2 where the LDS allows it, then 1, then 0 as the LDS of a CU is taken smaller; never a form that costs
    a workgroup; the debug switch's cap (max_form = 0) gives form 0.  Geometry of the shipped models (C = 72, rows of 96 floats, 20 992 B of tiles)."""
    src = tmp_path / "st.cpp"
    src.write_text('#include <cstdio>\n#include <cstdlib>\n#include "segments.hpp"\nint main(int c, char** v) { int a[6]; for (int i = 0; i < 6; i++) a[i] = atoi(v[i + 1]);\n'
                   '  bsx::SegK2 d; d.dw.C = a[0]; d.pw_b.Cin = 16; d.pw_b.Cout = a[0]; d.pw_b.cout_pad = a[1]; d.pw_b.w_off = 2208; d.pw_b.b_off = 3744; d.dw.w_off = a[5]; d.dw.b_off = 8000;\n'
                   '  const bsx::SegStage s = bsx::seg_k2_stage(d, a[2], a[3], a[4]);\n'
                   '  printf("%d %d %d %d %d %d %d %d\\n", s.form, s.off, s.floats, s.stride, s.buf_floats, s.bias_off, s.dw_off, s.dwb_off); return 0; }\n')
    exe = tmp_path / "st"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", CSRC, str(src), "-o", str(exe)])

    def stage(C=72, pad=96, base=5248, cap=LDS_CU, max_form=2, dw_w_off=4000):
        return [int(x) for x in subprocess.check_output([str(exe)] + [str(x) for x in (C, pad, base, cap, max_form, dw_w_off)]).decode().split()]

    f1 = 2 * (16 * 20 + 16)
    f2 = f1 + 9 * 72 + 72
    floats = {0: 0, 1: f1, 2: f2}
    base = 5248
    # today's tiles: form 2 (26 560 B) keeps 6 workgroups per CU
    assert stage() == [2, base, f2, 20, 336, 320, f1, f1 + 648]
    assert wgs_per_cu(4 * (base + f2)) == wgs_per_cu(4 * base) == 6
    # 2 -> 1 -> 0 as the budget shrinks
    # (from 6 x 20 992 B up: below that form 0 itself loses a workgroup and the question starts again at 5)
    caps = {cap: stage(cap=cap)[0] for cap in range(6 * 4 * base, LDS_CU + 1, 256)}
    assert sorted(set(caps.values())) == [0, 1, 2]
    forms = [caps[c] for c in sorted(caps)]
    assert forms == sorted(forms), "a larger budget never gives a smaller form"
    for cap, form in caps.items():
        assert wgs_per_cu(4 * (base + floats[form]), cap) == wgs_per_cu(4 * base, cap)                       # never at the price of a workgroup
        if form < 2:
            assert wgs_per_cu(4 * (base + floats[form + 1]), cap) < wgs_per_cu(4 * base, cap)               # and the next form would cost one
    assert stage(cap=6 * 4 * (base + f2))[0] == 2 and stage(cap=6 * 4 * (base + f2) - 1)[0] == 1
    assert stage(cap=6 * 4 * (base + f1))[0] == 1 and stage(cap=6 * 4 * (base + f1) - 1)[0] == 0
    assert stage(max_form=1) == [1, base, f1, 20, 336, 320, 0, 0] and stage(max_form=0) == [0] * 8
    # what the copies cannot move in 16-byte pieces, one per lane, is not staged
    assert stage(dw_w_off=4001)[0] == 1 and stage(C=70)[0] == 1 and stage(C=116, pad=128)[0] == 1 and stage(C=72, pad=72)[0] == 0


def test_the_debug_switch_forces_form_0_and_is_not_in_the_release_library(api, monkeypatch, debug_switches):
    from backscrub_amd import build
    assert "form 2" in [l for l in api.model_describe(model_path("lite")).splitlines() if l.startswith("segment k2")][0]
    monkeypatch.setenv("BSX_K2_GLOBAL_W", "1")
    line = [l for l in api.model_describe(model_path("lite")).splitlines() if l.startswith("segment k2")][0]
    assert "LDS 20.5 KiB (weights staged: form 0, 0 B)" in line
    assert "t.wst.form = 0;" in api.model_seg_source(model_path("lite"))
    rel = open(build.LIB, "rb").read()
    assert b"BSX_K2_GLOBAL_W" not in rel and b"BSX_K2_LDS_CAP" not in rel and b"BSX_K2_GLOBAL_W" in open(build.LIB_DBG, "rb").read()
