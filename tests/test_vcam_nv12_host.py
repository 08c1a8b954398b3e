"""bsx_step_batch_vcam_geoms_outs_nv12 and bsx_bgr_to_nv12 on a box without a GPU:
  * header, both libraries and the binding agree on the two symbols; ctypes' bsx_vcam_out_nv12 has the size and offsets of the struct compiled from the header;
  * MaskGen.step_vcam_geoms_outs_nv12 and MaskGen.bgr_to_nv12 validate their arguments before the library is reached;
  * the planner (csrc/vcam_nv12_plan.hpp) driven by a stand-alone program built with the host sanitizers: order, groups, workgroup sums, every refusal text;
  * the new kernels' resources (tools/kernel_regs.sh): no scratch, LDS not above vg_outs_fmt_k's of the same build."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

STEP, CONV = "bsx_step_batch_vcam_geoms_outs_nv12", "bsx_bgr_to_nv12"
CSRC = os.path.join(ROOT, "backscrub_amd", "csrc")
MAX_SIZES, MAX_PER_ITEM, MAX_CLASSES = 4, 4, 8


# ---- 1. the symbols and the record -------------------------------------------------------------------------------------------------------------------------------
def test_header_libraries_and_binding_agree_on_the_symbols(tmp_path):
    from backscrub_amd import api, build
    build.build()
    C = ctypes
    want = {STEP: [C.c_void_p, C.POINTER(C.c_int), C.POINTER(api._GeomItem), C.c_int, C.POINTER(api._VcamOutNv12), C.c_int, C.c_void_p, C.c_uint],
            CONV: [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]}
    proto = {STEP: "bsx_ctx* ctx, const int* ids, const bsx_geom_item* items, int n, const bsx_vcam_out_nv12* outs, int m, void* stream, unsigned flags /* 0 */",
             CONV: "bsx_ctx* ctx, const uint8_t* d_bgr, int w, int h, int n, uint8_t* d_y, int pitch_y, uint8_t* d_uv, int pitch_uv, void* stream"}
    hdr = open(os.path.join(ROOT, "include", "bsx.h")).read()
    for sym in (STEP, CONV):
        entry = [s for s in api.SYMBOLS if s[0] == sym]
        assert len(entry) == 1 and entry[0][1] is C.c_int and entry[0][2] == want[sym], sym
        m = re.search(r"^BSX_API int %s\(([^)]*)\);" % sym, hdr, re.M)
        assert m, "the header does not declare %s" % sym
        assert re.sub(r"\s+", " ", m.group(1)) == proto[sym]
    # the version script exports the C ABI by its prefix: the symbols must be in the dynamic table of both builds
    assert re.search(r"global:\s*bsx_\*;", open(os.path.join(CSRC, "libbsx.map")).read())
    for lib in (build.LIB, build.LIB_DBG):
        names = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout.split()
        assert STEP in names and CONV in names, lib
    assert hasattr(api.MaskGen, "step_vcam_geoms_outs_nv12") and hasattr(api.MaskGen, "bgr_to_nv12")
    # the record: a struct compiled from the header
    fields = ["item", "out_w", "out_h", "pitch_y", "pitch_uv", "d_y", "d_uv"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bsx.h"\nint main(void) { printf("%zu", sizeof(bsx_vcam_out_nv12));\n' +
                   "".join('  printf(" %%zu", offsetof(bsx_vcam_out_nv12, %s));\n' % f for f in fields) + '  printf("\\n"); return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe, str(src)])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    V = api._VcamOutNv12
    assert [f for f, _t in V._fields_] == fields
    assert [C.sizeof(V)] + [getattr(V, f).offset for f in fields] == got == [40, 0, 4, 8, 12, 16, 24, 32]


# ---- 2. the binding's validation ---------------------------------------------------------------------------------------------------------------------------------
def test_the_binding_validates_before_the_library_is_reached():
    torch = pytest.importorskip("torch")
    from backscrub_amd import api

    host = []

    class Fake(api.MaskGen):
        """no context (h is None: a library call would fail loudly); two classes, 16 x 8 and 32 x 16, two streams each; host tensors count as on the device, but
        for the ones listed in `host`"""
        def __init__(self):
            self.h, self.device, self.n_streams = None, 0, 4
            self._geoms = [dict(width=16, height=8, n_streams=2, first_stream=0), dict(width=32, height=16, n_streams=2, first_stream=2)]

        def _on_device(self, t):
            return not any(t is h for h in host)

    def u8(*shape):
        return torch.zeros(shape, dtype=torch.uint8)

    def surface(w, h, pitch_y=None, pitch_uv=None):
        """(y, uv): views into one allocation laid out as a surface"""
        py, puv = pitch_y or (w + 3) // 4 * 4, pitch_uv or (w + 3) // 4 * 4
        buf = u8(py * h + puv * (h // 2) + 64)
        off = (-buf.data_ptr()) % 4
        return (torch.as_strided(buf, (h, w), (py, 1), off), torch.as_strided(buf, (h // 2, w), (puv, 1), off + py * h))
    mg, S = Fake(), api.StreamSetting
    small, big, off = u8(8, 16, 3), u8(16, 32, 3), S(filter_off=True)

    def call(outs, ids=(0, 2), frames=None, settings=None):
        return mg.step_vcam_geoms_outs_nv12(list(ids), frames or [small, big], settings or [off, off], outs)
    y, uv = surface(12, 6, 16, 32)
    assert mg._nv12_planes("outs[0]", y, uv) == (12, 6, 16, 32)
    assert mg._nv12_planes("outs[0]", *surface(64, 2, 64, 128)) == (64, 2, 64, 128)       # one row pair: the UV plane has one row
    # the items: the messages of step_vcam_geoms_outs
    with pytest.raises(api.BsxError, match="2 ids for 1 frames and 2 settings"):
        call([], frames=[small])
    with pytest.raises(api.BsxFrameFormatError, match=r"frames\[1\].*\[16,32,3\]"):
        call([], frames=[small, small])
    with pytest.raises(api.BsxError, match=r"settings\[0\]: bgblur is not taken by step_vcam_geoms_outs_nv12"):
        call([], settings=[S(bgblur=5), off])
    with pytest.raises(api.BsxError, match=r"settings\[1\]: bg is required"):
        call([], settings=[off, S()])
    # the records
    with pytest.raises(api.BsxError, match=r"outs\[0\] must be a triple"):
        call([(0, y)])
    for bad in (2, -1, 1.0, True, None):
        with pytest.raises(api.BsxError, match=r"outs\[1\]: item .* is not an index into the call's 2 positions"):
            call([(0, y, uv), (bad,) + surface(12, 6)])
    with pytest.raises(api.BsxError, match=r"outs\[0\]: NV12 needs an even width and height \(y is 13 x 6\)"):      # an odd size
        call([(0,) + surface(13, 6, 16, 16)])
    with pytest.raises(api.BsxError, match=r"outs\[1\]: NV12 needs an even width and height \(y is 12 x 7\)"):
        call([(0, y, uv), (1, u8(7, 12), u8(3, 12))])
    with pytest.raises(api.BsxError, match=r"outs\[0\]: the pitch of y, 8, is below out_w = 12"):                   # a pitch below out_w
        call([(0, torch.as_strided(u8(256), (6, 12), (8, 1)), uv)])
    with pytest.raises(api.BsxError, match=r"outs\[0\]: the pitch of uv, 8, is below out_w = 12"):
        call([(0, y, torch.as_strided(u8(256), (3, 12), (8, 1)))])
    with pytest.raises(api.BsxError, match=r"outs\[1\]: the pitch of y, 6, is not a multiple of 4"):                # a pitch of 6
        call([(0, y, uv), (1, u8(4, 6), u8(2, 8)[:, :6])])
    with pytest.raises(api.BsxError, match=r"outs\[0\]: the pitch of uv, 6, is not a multiple of 4"):
        call([(0, u8(4, 8)[:, :6], u8(2, 6))])
    with pytest.raises(api.BsxError, match=r"outs\[0\]: y has an inner stride of 2"):                               # a non-unit inner stride
        call([(0, u8(6, 24)[:, ::2], uv)])
    with pytest.raises(api.BsxError, match=r"outs\[0\]: uv has an inner stride of 2"):
        call([(0, y, u8(3, 24)[:, ::2])])
    with pytest.raises(api.BsxError, match=r"outs\[0\]: uv must be \[3, 12\] for a y of \[6, 12\] \(it is \[6, 12\]\)"):      # a UV view of the wrong height
        call([(0, y, u8(6, 12))])
    with pytest.raises(api.BsxError, match=r"outs\[0\]: uv must be \[3, 12\] for a y of \[6, 12\] \(it is \[3, 6\]\)"):       # ... of half the width
        call([(0, y, u8(3, 6))])
    with pytest.raises(api.BsxError, match=r"outs\[0\]: uv must be a non-empty uint8 tensor of two dimensions \(it is torch.uint8 \(3, 6, 2\)\)"):
        call([(0, y, u8(3, 6, 2))])
    t = u8(6, 12)
    host.append(t)
    with pytest.raises(api.BsxError, match=r"outs\[0\]: y must be on cuda:0 \(it is on cpu\)"):                     # a host tensor
        call([(0, t, uv)])
    t = u8(3, 12)
    host.append(t)
    with pytest.raises(api.BsxError, match=r"outs\[1\]: uv must be on cuda:0 \(it is on cpu\)"):
        call([(1, y, uv), (0, y, t)])
    with pytest.raises(api.BsxError, match=r"outs\[0\]: y must be a non-empty uint8 tensor of two dimensions \(it is torch.float32 \(6, 12\)\)"):
        call([(0, y.to(torch.float32), uv)])
    with pytest.raises(api.BsxError, match=r"outs\[0\]: y must be a non-empty uint8 tensor"):
        call([(0, u8(0, 12), u8(0, 12))])
    base = u8(6 * 16 + 8)
    o = (-base.data_ptr()) % 4 + 2
    with pytest.raises(api.BsxError, match=r"outs\[0\]: y at 0x[0-9a-f]+ is not 4-byte aligned"):
        call([(0, torch.as_strided(base, (6, 12), (16, 1), o), uv)])
    with pytest.raises(api.BsxError, match=r"outs\[4\]: record 5 of position 1"):
        call([(1,) + surface(12, 6) for _ in range(5)])
    with pytest.raises(api.BsxError, match=r"outs\[4\]: 20 x 6 is distinct output size 5"):
        call([(j % 2,) + surface(12 + 2 * j, 6) for j in range(5)])
    # bgr_to_nv12
    with pytest.raises(api.BsxFrameFormatError, match=r"bgr must be a contiguous, non-empty uint8 tensor \[n,h,w,3\]"):
        mg.bgr_to_nv12(u8(6, 12, 3))
    with pytest.raises(api.BsxFrameFormatError, match=r"even width and height \(bgr is 13 x 6\)"):
        mg.bgr_to_nv12(u8(2, 6, 13, 3))
    with pytest.raises(api.BsxFrameFormatError, match=r"even width and height \(bgr is 12 x 5\)"):
        mg.bgr_to_nv12(u8(2, 5, 12, 3))
    with pytest.raises(api.BsxError, match=r"pitch_y = 8 must be a multiple of 4 and at least w = 12"):
        mg.bgr_to_nv12(u8(2, 6, 12, 3), pitch_y=8)
    with pytest.raises(api.BsxError, match=r"pitch_uv = 14 must be a multiple of 4 and at least w = 12"):
        mg.bgr_to_nv12(u8(2, 6, 12, 3), pitch_uv=14)
    t = u8(2, 6, 12, 3)
    host.append(t)
    with pytest.raises(api.BsxError, match=r"bgr must be on cuda:0"):
        mg.bgr_to_nv12(t)


# ---- 3. the planner, stand-alone under the host sanitizers ----------------------------------------------------------------------------------------------------------
MAIN = r"""
// reads cases from stdin: "n m null_outs", then n classes, then max(m, 0) records "item w h pitch_y pitch_uv y uv" (none with null_outs); prints the planner's answer
// as one line of integers "rc bad n_sizes total_wg n_order n_groups | sizes.. | order.. | groups (cls size first count wg0 per ntx words).." and the refusal text on
// the next line
#include <cstdio>
#include <vector>
#include "vcam_nv12_plan.hpp"
int main() {
  int n, m, null_outs;
  while (scanf("%d %d %d", &n, &m, &null_outs) == 3) {
    std::vector<int> cls((size_t)n);
    for (int& c : cls) if (scanf("%d", &c) != 1) return 2;
    std::vector<bsx_vcam_out_nv12> outs((size_t)(m > 0 && !null_outs ? m : 0));      // exactly m records: a read past the end is the sanitizer's to report
    for (bsx_vcam_out_nv12& o : outs) {
      unsigned long long y, uv;
      if (scanf("%d %d %d %d %d %llu %llu", &o.item, &o.out_w, &o.out_h, &o.pitch_y, &o.pitch_uv, &y, &uv) != 7) return 2;
      o.d_y = reinterpret_cast<uint8_t*>((uintptr_t)y);
      o.d_uv = reinterpret_cast<uint8_t*>((uintptr_t)uv);
    }
    bsx::VcamOutsPlan plan;
    const int rc = bsx::vcam_nv12_plan(cls.data(), n, null_outs ? nullptr : outs.data(), m, &plan);
    printf("%d %d %d %ld %zu %zu |", rc, plan.bad, plan.n_sizes, plan.total_wg, plan.order.size(), plan.groups.size());
    for (int s = 0; s < plan.n_sizes; s++) printf(" %d %d", plan.sizes[s][0], plan.sizes[s][1]);
    printf(" |");
    for (int j : plan.order) printf(" %d", j);
    printf(" |");
    for (const bsx::VcamOutsGroup& g : plan.groups) printf(" %d %d %d %d %ld %d %d %d", g.cls, g.size, g.first, g.count, g.wg0, g.per, g.ntx, g.words ? 1 : 0);
    printf("\n%s\n", plan.text);
  }
  printf("%zu %zu %zu\n", bsx::vcam_nv12_extent(256, 90, 160), bsx::vcam_nv12_extent(64, 1, 64), bsx::vcam_nv12_extent(1 << 30, 1 << 15, 1 << 30));
  return 0;
}
"""


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    d = tmp_path_factory.mktemp("vcam_nv12_plan")
    src, exe = d / "main.cpp", str(d / "plan")
    src.write_text(MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC,
                           "-o", exe, str(src)])

    def run(cases):
        """cases: (classes, records or None, m or None) -> the planner's answer per case as a dict"""
        text = []
        for classes, recs, m in cases:
            null = recs is None
            recs = recs or []
            text.append("%d %d %d" % (len(classes), len(recs) if m is None else m, int(null)))
            text.append(" ".join(str(c) for c in classes))
            text += ["%d %d %d %d %d %d %d" % r for r in recs]
        r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, "the planner's program failed (a sanitizer report?):\n" + r.stderr[-3000:]
        lines = r.stdout.split("\n")
        assert len(lines) == 2 * len(cases) + 2, r.stdout[-500:]
        assert [int(v) for v in lines[-2].split()] == [256 * 89 + 160, 64, (1 << 30) * ((1 << 15) - 1) + (1 << 30)]      # the overlap extent, in size_t
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


def _check_plan(classes, recs, p):
    """every property of an accepted plan, from the inputs alone"""
    assert p["rc"] == 0 and p["text"] == "" and p["bad"] == -1, p
    sizes = []
    for r in recs:
        if (r[1], r[2]) not in sizes:
            sizes.append((r[1], r[2]))
    assert p["sizes"] == sizes                                              # in the order of their first record
    key = [(classes[r[0]], sizes.index((r[1], r[2]))) for r in recs]
    assert p["order"] == sorted(range(len(recs)), key=lambda j: key[j])     # (sorted is stable)
    at = wg = 0
    seen = []
    for g in p["groups"]:
        assert g["first"] == at and g["count"] >= 1 and g["wg0"] == wg, (g, at, wg)
        members = p["order"][at:at + g["count"]]
        assert {key[j] for j in members} == {(g["cls"], g["size"])}
        w, h = sizes[g["size"]]
        assert g["ntx"] == (w + 63) // 64 and g["per"] == _tiles(w, h)      # the tile stays 64 x 32
        seen.append((g["cls"], g["size"]))
        at += g["count"]
        wg += g["count"] * g["per"]
    assert at == len(recs) and seen == sorted(set(key)), "the groups do not partition the records in (class, size) order"
    assert p["total"] == wg == sum(_tiles(r[1], r[2]) for r in recs)
    assert len(p["groups"]) <= 32


SIM = [(640, 360), (320, 180), (160, 90)]
RAGGED = [(318, 178), (426, 240), (66, 34), (64, 2)]


def _rec(i, w, h, k, pitch_y=None, pitch_uv=None):
    """record: item i at w x h, surface number k — planes 16 MiB apart"""
    return (i, w, h, pitch_y or (w + 3) // 4 * 4, pitch_uv or (w + 3) // 4 * 4, (2 * k + 1) << 24, (2 * k + 2) << 24)


def test_planner_orders_groups_and_counts(planner):
    rng = np.random.default_rng(20241)
    cases = []
    six = [0, 0, 1, 1, 2, 2]
    cases.append((six, [_rec(i, w, h, 3 * i + k, 256 if w == 160 else None) for i in range(6) for k, (w, h) in enumerate(SIM)], None))      # simulcast
    cases.append((six, [_rec(i, w, h, 3 * i + k) for k, (w, h) in enumerate(SIM) for i in (5, 0, 3, 1, 4, 2)], None))
    cases.append((six, [_rec(i, w, h, 4 * i + k, pitch_uv=512) for i in (0, 2, 4) for k, (w, h) in enumerate(RAGGED)], None))                 # twelve groups, ragged
    cases.append(([1], [_rec(0, 640, 360, 0), _rec(0, 320, 180, 1), _rec(0, 640, 360, 2), _rec(0, 160, 90, 3)], None))                        # one item, four records
    cases.append((six, [], None))                                                                                                           # m == 0
    cases.append((six, None, 0))                                                                                                            # ... with outs NULL
    cases.append((list(range(8)) * 4, [_rec(i, w, h, i + 32 * k) for k, (w, h) in enumerate(RAGGED) for i in range(32)], None))               # all 32 groups
    for _ in range(300):
        n = int(rng.integers(1, 24))
        classes = [int(c) for c in rng.integers(0, MAX_CLASSES, n)]
        pool = [(2 * int(rng.integers(1, 350)), 2 * int(rng.integers(1, 200))) for _ in range(int(rng.integers(1, MAX_SIZES + 1)))]
        recs = []
        for i in rng.permutation(n):
            for _k in range(int(rng.integers(0, MAX_PER_ITEM + 1))):
                w, h = pool[int(rng.integers(0, len(pool)))]
                recs.append(_rec(int(i), w, h, len(recs), (w + 3) // 4 * 4 + 4 * int(rng.integers(0, 64)), (w + 3) // 4 * 4 + 4 * int(rng.integers(0, 64))))
        recs = [recs[j] for j in rng.permutation(len(recs))]
        cases.append((classes, recs, None))
    for (classes, recs, _m), p in zip(cases, planner(cases)):
        _check_plan(classes, recs or [], p)


def test_planner_refuses_each_bad_record_with_its_index(planner):
    ok = [_rec(0, 640, 360, 0), _rec(1, 320, 180, 1), _rec(0, 160, 90, 2, 256, 256)]
    cls = [0, 3]
    Y, UV = 9 << 24, 10 << 24

    def at(j, rec):
        r = list(ok)
        r.insert(j, rec)
        return r
    cases = [
        (cls, None, 3, -1, "outs is NULL with m = 3"),
        (cls, [], -2, -1, "m = -2 is negative"),
        (cls, at(2, (2, 64, 32, 64, 64, Y, UV)), None, 2, "outs[2]: item 2 is outside [0, 2)"),
        (cls, at(0, (-1, 64, 32, 64, 64, Y, UV)), None, 0, "outs[0]: item -1 is outside [0, 2)"),
        (cls, at(3, (1, 0, 32, 64, 64, Y, UV)), None, 3, "outs[3]: output size 0 x 32 must be positive"),
        (cls, at(1, (1, 64, -6, 64, 64, Y, UV)), None, 1, "outs[1]: output size 64 x -6 must be positive"),
        (cls, at(1, (1, 65, 32, 68, 68, Y, UV)), None, 1, "outs[1]: NV12 output needs an even width and height (65 x 32)"),
        (cls, at(3, (1, 64, 33, 64, 64, Y, UV)), None, 3, "outs[3]: NV12 output needs an even width and height (64 x 33)"),
        (cls, at(0, (1, 64, 32, 60, 64, Y, UV)), None, 0, "outs[0]: pitch_y = 60 is below out_w = 64"),
        (cls, at(2, (1, 64, 32, 66, 64, Y, UV)), None, 2, "outs[2]: pitch_y = 66 is not a multiple of 4"),
        (cls, at(2, (1, 64, 32, 64, 0, Y, UV)), None, 2, "outs[2]: pitch_uv = 0 is below out_w = 64"),
        (cls, at(1, (1, 6, 4, 8, 6, Y, UV)), None, 1, "outs[1]: pitch_uv = 6 is not a multiple of 4"),
        (cls, at(2, (1, 64, 32, 64, 64, 0, UV)), None, 2, "outs[2]: d_y is NULL"),
        (cls, at(2, (1, 64, 32, 64, 64, 4098, UV)), None, 2, "outs[2]: d_y 0x1002 is not 4-byte aligned"),
        (cls, at(3, (1, 64, 32, 64, 64, Y, 0)), None, 3, "outs[3]: d_uv is NULL"),
        (cls, at(0, (1, 64, 32, 64, 64, Y, 4097)), None, 0, "outs[0]: d_uv 0x1001 is not 4-byte aligned"),
        (cls, ok + [_rec(0, 640, 360, k) for k in (5, 6, 7)], None, 5, "outs[5]: record 5 of items[0] (at most 4 name one item)"),
        (cls, ok + [_rec(1, 64, 32, 5), _rec(1, 66, 34, 6)], None, 4, "outs[4]: 66 x 34 is distinct output size 5 of the call (at most 4)"),
    ]
    res = planner([c[:3] for c in cases])
    for (_c, _r, _m, bad, text), p in zip(cases, res):
        assert (p["rc"], p["bad"], p["text"]) == (1, bad, text), p
        assert "BSX_" not in p["text"]
    # 2^31 workgroups or more is the other answer
    huge, = planner([([0], [_rec(0, 64 * 70000, 32 * 40000, 0)], None)])
    assert huge["rc"] == 2


# ---- 4. kernel resources ---------------------------------------------------------------------------------------------------------------------------------------------
def test_the_new_kernels_use_no_scratch_and_no_more_lds():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not installed")
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_regs.sh"), os.path.join(CSRC, "kernels_img.hip"), "vg_outs|bgr_to_nv12"], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0 and "compile failed" not in r.stdout, r.stdout[-500:] + r.stderr[-500:]
    row = re.compile(r"^(\S+)\s+vgpr\+agpr\s+(\d+)\s+accum_offset\s+(\d+)\s+lds\s+(\d+)\s+scratch\s+(\d+)")
    rows = {m.group(1): dict(vgpr=int(m.group(2)), arch_vgpr=int(m.group(3)), lds=int(m.group(4)), scratch=int(m.group(5))) for m in map(row.match, r.stdout.splitlines()) if m}

    def some(needle, count):
        hit = [v for k, v in rows.items() if needle in k]
        assert len(hit) == count, (needle, sorted(rows))
        return hit
    limit = some("vg_outs_fmt_kI", 1)[0]["lds"]
    for new, count in (("vg_outs_nv12_kI", 1), ("vg_outs_nv12_fmt_kI", 1), ("bgr_to_nv12_kI", 2)):
        for a in some(new, count):
            print(new, a, "lds limit", limit)
            assert a["scratch"] == 0, "%s spills %d bytes" % (new, a["scratch"])
            assert a["lds"] <= limit, (new, a, limit)
