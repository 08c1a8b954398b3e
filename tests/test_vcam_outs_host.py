"""bsx_step_batch_vcam_geoms_outs on a box without a GPU:
  * header, libbsx.map, both libraries and the binding agree on the symbol; ctypes' bsx_vcam_out has the size and offsets of the struct compiled from the header;
  * MaskGen.step_vcam_geoms_outs validates its arguments before the library is reached;
  * the planner (csrc/vcam_outs_plan.hpp) driven by a stand-alone program built with the host sanitizers: order, groups, workgroup sums, the dword bit, refusals;
  * the two new kernels' resources (tools/kernel_regs.sh) against vg_geoms_k / vg_geoms_fmt_k of the same build."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SYM = "bsx_step_batch_vcam_geoms_outs"
CSRC = os.path.join(ROOT, "backscrub_amd", "csrc")
MAX_SIZES, MAX_PER_ITEM, MAX_CLASSES = 4, 4, 8


# ---- 1. the symbol and the record --------------------------------------------------------------------------------------------------------------------------------
def test_header_map_libraries_and_binding_agree_on_the_symbol(tmp_path):
    from backscrub_amd import api, build
    build.build()
    C = ctypes
    entry = [s for s in api.SYMBOLS if s[0] == SYM]
    assert len(entry) == 1
    assert entry[0][1] is C.c_int and entry[0][2] == [C.c_void_p, C.POINTER(C.c_int), C.POINTER(api._GeomItem), C.c_int, C.POINTER(api._VcamOut), C.c_int, C.c_void_p,
                                                      C.c_uint]
    hdr = open(os.path.join(ROOT, "include", "bsx.h")).read()
    m = re.search(r"^BSX_API int %s\(([^)]*)\);" % SYM, hdr, re.M)
    assert m, "the header does not declare %s" % SYM
    assert re.sub(r"\s+", " ", m.group(1)) == ("bsx_ctx* ctx, const int* ids, const bsx_geom_item* items, int n, const bsx_vcam_out* outs, int m, void* stream, "
                                               "unsigned flags")
    assert re.search(r"^#define BSX_MAX_OUT_SIZES 4\b", hdr, re.M) and re.search(r"^#define BSX_MAX_OUTS_PER_ITEM 4\b", hdr, re.M)
    assert (api.BSX_MAX_OUT_SIZES, api.BSX_MAX_OUTS_PER_ITEM) == (4, 4)
    # the version script exports the C ABI by its prefix: the symbol must be in the dynamic table of both builds
    assert re.search(r"global:\s*bsx_\*;", open(os.path.join(CSRC, "libbsx.map")).read())
    for lib in (build.LIB, build.LIB_DBG):
        names = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout.split()
        assert SYM in names, (lib, SYM)
    assert hasattr(api.MaskGen, "step_vcam_geoms_outs")
    # the record: a struct compiled from the header
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bsx.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(bsx_vcam_out), '
                   'offsetof(bsx_vcam_out, item), offsetof(bsx_vcam_out, out_w), offsetof(bsx_vcam_out, out_h), offsetof(bsx_vcam_out, d_out)); return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe, str(src)])
    want = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    V = api._VcamOut
    assert [C.sizeof(V), V.item.offset, V.out_w.offset, V.out_h.offset, V.d_out.offset] == want == [24, 0, 4, 8, 16]


# ---- 2. the binding's validation ---------------------------------------------------------------------------------------------------------------------------------
def test_the_binding_validates_before_the_library_is_reached():
    torch = pytest.importorskip("torch")
    from backscrub_amd import api

    class Fake(api.MaskGen):
        """no context (h is None: a library call would fail loudly); two classes, 16 x 8 and 32 x 16, two streams each; host tensors count as on the device"""
        def __init__(self):
            self.h, self.device, self.n_streams = None, 0, 4
            self._geoms = [dict(width=16, height=8, n_streams=2, first_stream=0), dict(width=32, height=16, n_streams=2, first_stream=2)]

        def _on_device(self, t):
            return True

    def u8(*shape):
        return torch.zeros(shape, dtype=torch.uint8)
    mg, S = Fake(), api.StreamSetting
    small, big, off = u8(8, 16, 3), u8(16, 32, 3), S(filter_off=True)
    o = u8(6, 10, 3)

    def call(outs, ids=(0, 2), frames=None, settings=None, **kw):
        return mg.step_vcam_geoms_outs(list(ids), frames or [small, big], settings or [off, off], outs, **kw)
    with pytest.raises(api.BsxError, match="2 ids for 1 frames and 2 settings"):
        call([], frames=[small])
    with pytest.raises(api.BsxFrameFormatError, match=r"frames\[1\].*\[16,32,3\]"):
        call([], frames=[small, small])
    with pytest.raises(api.BsxFrameFormatError, match=r"frames\[0\].*\[8,16,2\].*YUYV item"):
        call([], settings=[S(filter_off=True, yuyv_in=True), off])
    with pytest.raises(api.BsxError, match=r"settings\[1\] is not a StreamSetting"):
        call([], settings=[off, None])
    with pytest.raises(api.BsxError, match=r"settings\[0\]: bgblur"):
        call([], settings=[S(bgblur=5), off])
    with pytest.raises(api.BsxError, match=r"settings\[1\]: bg is required"):
        call([], settings=[off, S()])
    with pytest.raises(api.BsxError, match=r"settings\[1\]\.bg.*\[16,32,3\]"):
        call([], settings=[off, S(bg=small)])
    with pytest.raises(api.BsxError, match=r"outs\[0\] must be a pair"):
        call([o])
    for bad in (2, -1, 1.0, True, None):
        with pytest.raises(api.BsxError, match=r"outs\[1\]: item .* is not an index into the call's 2 positions"):
            call([(0, o), (bad, o.clone())])
    with pytest.raises(api.BsxError, match=r"outs\[0\]: the output must be .*\[out_h,out_w,3\]"):
        call([(0, u8(6, 10, 2))])
    with pytest.raises(api.BsxError, match=r"outs\[0\]: the output must be .*\[out_h,out_w,2\]"):
        call([(0, o)], yuyv=True)
    with pytest.raises(api.BsxError, match=r"outs\[1\]: the output must be"):
        call([(0, o), (1, o.to(torch.float32))])
    with pytest.raises(api.BsxError, match=r"outs\[0\]: the output must be"):
        call([(0, u8(6, 20, 3)[:, ::2])])                                  # not contiguous
    with pytest.raises(api.BsxError, match=r"outs\[0\]: the output must be"):
        call([(0, u8(0, 10, 3))])
    with pytest.raises(api.BsxError, match=r"outs\[0\]: YUYV output needs an even width .*9 wide"):
        call([(1, u8(6, 9, 2))], yuyv=True)
    with pytest.raises(api.BsxError, match=r"outs\[4\]: record 5 of position 1"):
        call([(1, o.clone()) for _ in range(5)])
    with pytest.raises(api.BsxError, match=r"outs\[4\]: 14 x 6 is distinct output size 5"):
        call([(j % 2, u8(6, 10 + j, 3)) for j in range(5)])


# ---- 3. the planner, stand-alone under the host sanitizers ----------------------------------------------------------------------------------------------------------
MAIN = r"""
// reads cases from stdin: "n m yuyv null_outs", then n classes, then max(m, 0) records "item w h ptr" (none with null_outs); prints the planner's answer as one line of integers
// "rc bad n_sizes total_wg n_order n_groups | sizes.. | order.. | groups (cls size first count wg0 per ntx words).." and the refusal text on the next line
#include <cstdio>
#include <vector>
#include "vcam_outs_plan.hpp"
int main() {
  int n, m, yuyv, null_outs;
  while (scanf("%d %d %d %d", &n, &m, &yuyv, &null_outs) == 4) {
    std::vector<int> cls((size_t)n);
    for (int& c : cls) if (scanf("%d", &c) != 1) return 2;
    std::vector<bsx_vcam_out> outs((size_t)(m > 0 && !null_outs ? m : 0));      // exactly m records: a read past the end is the sanitizer's to report
    for (bsx_vcam_out& o : outs) {
      unsigned long long p;
      if (scanf("%d %d %d %llu", &o.item, &o.out_w, &o.out_h, &p) != 4) return 2;
      o.d_out = reinterpret_cast<uint8_t*>((uintptr_t)p);
    }
    bsx::VcamOutsPlan plan;
    const int rc = bsx::vcam_outs_plan(cls.data(), n, null_outs ? nullptr : outs.data(), m, yuyv != 0, &plan);
    printf("%d %d %d %ld %zu %zu |", rc, plan.bad, plan.n_sizes, plan.total_wg, plan.order.size(), plan.groups.size());
    for (int s = 0; s < plan.n_sizes; s++) printf(" %d %d", plan.sizes[s][0], plan.sizes[s][1]);
    printf(" |");
    for (int j : plan.order) printf(" %d", j);
    printf(" |");
    for (const bsx::VcamOutsGroup& g : plan.groups) printf(" %d %d %d %d %ld %d %d %d", g.cls, g.size, g.first, g.count, g.wg0, g.per, g.ntx, g.words ? 1 : 0);
    printf("\n%s\n", plan.text);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    d = tmp_path_factory.mktemp("vcam_outs_plan")
    src, exe = d / "main.cpp", str(d / "plan")
    src.write_text(MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC,
                           "-o", exe, str(src)])

    def run(cases):
        """cases: (classes, records or None, m or None, yuyv) -> the planner's answer per case as a dict"""
        text = []
        for classes, recs, m, yuyv in cases:
            null = recs is None
            recs = recs or []
            text.append("%d %d %d %d" % (len(classes), len(recs) if m is None else m, int(yuyv), int(null)))
            text.append(" ".join(str(c) for c in classes))
            text += ["%d %d %d %d" % r for r in recs]
        r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, "the planner's program failed (a sanitizer report?):\n" + r.stderr[-3000:]
        lines = r.stdout.split("\n")
        assert len(lines) == 2 * len(cases) + 1, r.stdout[-500:]
        out = []
        for k in range(len(cases)):
            head, sizes, order, groups = (part.split() for part in lines[2 * k].split("|"))
            rc, bad, n_sizes, total, n_order, n_groups = (int(v) for v in head)
            sizes, order, groups = [int(v) for v in sizes], [int(v) for v in order], [int(v) for v in groups]
            assert len(sizes) == 2 * n_sizes and len(order) == n_order and len(groups) == 8 * n_groups
            out.append(dict(rc=rc, bad=bad, total=total, sizes=list(zip(sizes[::2], sizes[1::2])), order=order, text=lines[2 * k + 1],
                            groups=[dict(zip(("cls", "size", "first", "count", "wg0", "per", "ntx", "words"), groups[8 * g:8 * g + 8])) for g in range(n_groups)]))
        return out
    return run


def _tiles(w, h):
    return ((w + 63) // 64) * ((h + 31) // 32)


def _check_plan(classes, recs, yuyv, p):
    """every property of an accepted plan, from the inputs alone"""
    assert p["rc"] == 0 and p["text"] == "" and p["bad"] == -1, p
    sizes = []
    for _i, w, h, _p in recs:
        if (w, h) not in sizes:
            sizes.append((w, h))
    assert p["sizes"] == sizes                                              # in the order of their first record
    key = [(classes[i], sizes.index((w, h))) for i, w, h, _p in recs]
    assert p["order"] == sorted(range(len(recs)), key=lambda j: key[j])     # (sorted is stable)
    at = wg = 0
    seen = []
    for g in p["groups"]:
        assert g["first"] == at and g["count"] >= 1 and g["wg0"] == wg, (g, at, wg)
        members = p["order"][at:at + g["count"]]
        assert {key[j] for j in members} == {(g["cls"], g["size"])}
        w, h = sizes[g["size"]]
        assert g["ntx"] == (w + 63) // 64 and g["per"] == _tiles(w, h)
        assert g["words"] == int(bool(yuyv) or w % 4 == 0), (g, w, yuyv)
        seen.append((g["cls"], g["size"]))
        at += g["count"]
        wg += g["count"] * g["per"]
    assert at == len(recs) and seen == sorted(set(key)), "the groups do not partition the records in (class, size) order"
    assert p["total"] == wg == sum(_tiles(w, h) for _i, w, h, _p in recs)
    assert len(p["groups"]) <= 32


SIM = [(640, 360), (320, 180), (160, 90)]
RAGGED = [(427, 240), (426, 240), (66, 34), (64, 32)]


def test_planner_orders_groups_and_counts(planner):
    rng = np.random.default_rng(20240)
    cases = []
    six = [0, 0, 1, 1, 2, 2]
    cases.append((six, [(i, w, h, 4096 * (3 * i + k + 1)) for i in range(6) for k, (w, h) in enumerate(SIM)], None, True))           # simulcast
    cases.append((six, [(i, w, h, 4096 * (3 * i + k + 1)) for k, (w, h) in enumerate(SIM) for i in (5, 0, 3, 1, 4, 2)], None, False))
    sp = [(3, 1280, 720, 4096)] + [(i, 320, 180, 8192 + 4096 * i) for i in (0, 2, 5)]                                               # speaker + thumbnails, two silent
    cases.append((six, [sp[j] for j in np.random.default_rng(5).permutation(len(sp))], None, False))
    cases.append((six, [(i, w, h, 4096 * (4 * i + k + 1)) for i in (0, 2, 4) for k, (w, h) in enumerate(RAGGED)], None, False))      # twelve groups, ragged
    cases.append((six, [(i, w, h, 4096 * (4 * i + k + 1)) for i in (4, 2, 0) for k, (w, h) in enumerate([(426, 240), (66, 34), (64, 32), (160, 90)])], None, True))
    cases.append(([1], [(0, 640, 360, 4096), (0, 320, 180, 8192), (0, 640, 360, 12288), (0, 160, 90, 16384)], None, False))           # one item, four records
    cases.append((six, [], None, False))                                                                                            # m == 0
    cases.append((six, None, 0, False))                                                                                             # ... with outs NULL
    cases.append((list(range(8)) * 4, [(i, w, h, 4096 * (1 + i + 32 * k)) for k, (w, h) in enumerate(RAGGED) for i in range(32)], None, False))      # all 32 groups
    for _ in range(300):
        n = int(rng.integers(1, 24))
        classes = [int(c) for c in rng.integers(0, MAX_CLASSES, n)]
        pool = [(int(rng.integers(1, 700)), int(rng.integers(1, 400))) for _ in range(int(rng.integers(1, MAX_SIZES + 1)))]
        yuyv = bool(rng.integers(0, 2))
        if yuyv:
            pool = [(w + (w & 1), h) for w, h in pool]
        recs = []
        for i in rng.permutation(n):
            for _k in range(int(rng.integers(0, MAX_PER_ITEM + 1))):
                w, h = pool[int(rng.integers(0, len(pool)))]
                recs.append((int(i), w, h, 4 * int(rng.integers(1, 1 << 40))))
        recs = [recs[j] for j in rng.permutation(len(recs))]
        cases.append((classes, recs, None, yuyv))
    for (classes, recs, _m, yuyv), p in zip(cases, planner(cases)):
        _check_plan(classes, recs or [], yuyv, p)


def test_planner_refuses_each_bad_record_with_its_index(planner):
    ok = [(0, 640, 360, 4096), (1, 320, 180, 8192), (0, 160, 90, 12288)]
    cls = [0, 3]

    def at(j, rec):
        r = list(ok)
        r.insert(j, rec)
        return r
    cases = [
        (cls, None, 3, False, -1, "outs is NULL with m = 3"),
        (cls, [], -2, False, -1, "m = -2 is negative"),
        (cls, at(2, (2, 64, 32, 16)), None, False, 2, "outs[2]: item 2 is outside [0, 2)"),
        (cls, at(0, (-1, 64, 32, 16)), None, False, 0, "outs[0]: item -1 is outside [0, 2)"),
        (cls, at(3, (1, 0, 32, 16)), None, False, 3, "outs[3]: output size 0 x 32 must be positive"),
        (cls, at(1, (1, 64, -5, 16)), None, False, 1, "outs[1]: output size 64 x -5 must be positive"),
        (cls, at(1, (1, 65, 32, 16)), None, True, 1, "outs[1]: YUYV output needs an even width (out_w = 65)"),
        (cls, at(2, (1, 64, 32, 0)), None, False, 2, "outs[2]: d_out is NULL"),
        (cls, at(2, (1, 64, 32, 4098)), None, False, 2, "outs[2]: d_out 0x1002 is not 4-byte aligned"),
        (cls, ok + [(0, 640, 360, 4096 * k) for k in (5, 6, 7)], None, False, 5, "outs[5]: record 5 of items[0] (at most 4 name one item)"),
        (cls, ok + [(1, 64, 32, 4096 * 5), (1, 66, 34, 4096 * 6)], None, False, 4, "outs[4]: 66 x 34 is distinct output size 5 of the call (at most 4)"),
    ]
    res = planner([c[:4] for c in cases])
    for (_c, _r, _m, _y, bad, text), p in zip(cases, res):
        assert (p["rc"], p["bad"], p["text"]) == (1, bad, text), p
        assert "BSX_" not in p["text"]
    # an odd width is fine without YUYV; 2^31 workgroups or more is the other answer
    fine, huge = planner([(cls, at(1, (1, 65, 32, 16)), None, False), ([0], [(0, 64 * 70000, 32 * 40000, 4096)], None, False)])
    assert fine["rc"] == 0 and huge["rc"] == 2


# ---- 4. kernel resources ---------------------------------------------------------------------------------------------------------------------------------------------
def test_the_new_kernels_take_no_more_than_the_ones_they_mirror():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not installed")
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_regs.sh"), os.path.join(CSRC, "kernels_img.hip"), "vg_outs|vg_geoms"], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0 and "compile failed" not in r.stdout, r.stdout[-500:] + r.stderr[-500:]
    row = re.compile(r"^(\S+)\s+vgpr\+agpr\s+(\d+)\s+accum_offset\s+(\d+)\s+lds\s+(\d+)\s+scratch\s+(\d+)")
    rows = {m.group(1): dict(vgpr=int(m.group(2)), arch_vgpr=int(m.group(3)), lds=int(m.group(4)), scratch=int(m.group(5))) for m in map(row.match, r.stdout.splitlines()) if m}

    def one(needle):
        hit = [v for k, v in rows.items() if needle in k]
        assert len(hit) == 1, (needle, sorted(rows))
        return hit[0]
    for new, old in (("vg_outs_kI", "vg_geoms_kI"), ("vg_outs_fmt_kI", "vg_geoms_fmt_kI")):
        a, b = one(new), one(old)
        print(new, a, old, b)
        assert a["scratch"] == 0, "%s spills %d bytes" % (new, a["scratch"])
        assert a["vgpr"] <= b["vgpr"] and a["arch_vgpr"] <= b["arch_vgpr"] and a["lds"] <= b["lds"], (new, a, old, b)
