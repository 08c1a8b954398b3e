"""The planners of the n-picture image batches (csrc/picture_batch_plan.hpp) that the two surfaces files do not drive — bsx_gaussian_blur_bgr_batch and
bsx_resize_bgr_batch, and the overlap rule of bsx_gaussian_blur_surfaces_batch — on a box without a GPU: a stand-alone program built with the host sanitizers and run
directly.  Every refusal with its exact text and index (the texts are the ones the calls have always given: tests/test_gpu_blur_batch.py and
tests/test_grab_batch_host.py match parts of them through the library), which of two broken rules a call names, the three overlap kinds, and an accepted plan — the
classes in the order of first appearance, the stable order, the ragged grid and the tile columns — against a restatement in Python."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "backscrub_amd", "csrc")
MAX_SIZES = 8
YIN = 0x40      # BSX_STREAM_YUYV_IN
BLUR, RESIZE, BLUR_SURFACES = 0, 1, 2

MAIN = r"""
// reads cases from stdin: "call n n_streams null_items dw dh", then (none with null_items) max(n, 0) items — call 0, bsx_gaussian_blur_bgr_batch: "src dst w h ksize
// flags"; 1, bsx_resize_bgr_batch (to dw x dh): "src sw sh dst"; 2, bsx_gaussian_blur_surfaces_batch: "y uv dst pitch_y pitch_uv w h ksize flags".  Prints the plan as
// one line of integers "rc bad n_sizes n_cls | cls.. | order.. | sizes.. | pos[9] | wg[9] | per[8] | ntx[8]" and the refusal text on the next line
#include <cstdio>
#include <vector>
#include "picture_batch_plan.hpp"
template <class T> T* ptr(unsigned long long v) { return reinterpret_cast<T*>((uintptr_t)v); }
int main() {
  static_assert(BSX_STREAM_YUYV_IN == 0x40, "the flag of the header");
  int call, n, n_streams, null_items, dw, dh;
  bsx::PictureBatchPlan plan;                                  // one plan for every case, as a context keeps one: nothing of a case may survive into the next
  while (scanf("%d %d %d %d %d %d", &call, &n, &n_streams, &null_items, &dw, &dh) == 6) {
    const size_t m = (size_t)(n > 0 && !null_items ? n : 0);   // exactly n items: a read past the end is the sanitizer's to report
    std::vector<bsx_blur_item> blur(call == 0 ? m : 0);
    std::vector<bsx_resize_item> resize(call == 1 ? m : 0);
    std::vector<bsx_blur_surface_item> surf(call == 2 ? m : 0);
    unsigned long long a, b, c;
    for (bsx_blur_item& it : blur) {
      if (scanf("%llu %llu %d %d %d %u", &a, &b, &it.w, &it.h, &it.ksize, &it.flags) != 6) return 2;
      it.d_src = ptr<const uint8_t>(a); it.d_dst = ptr<uint8_t>(b);
    }
    for (bsx_resize_item& it : resize) {
      if (scanf("%llu %d %d %llu", &a, &it.sw, &it.sh, &b) != 4) return 2;
      it.d_src = ptr<const uint8_t>(a); it.d_dst = ptr<uint8_t>(b);
    }
    for (bsx_blur_surface_item& it : surf) {
      if (scanf("%llu %llu %llu %d %d %d %d %d %u", &a, &b, &c, &it.pitch_y, &it.pitch_uv, &it.w, &it.h, &it.ksize, &it.flags) != 9) return 2;
      it.d_y = ptr<const uint8_t>(a); it.d_uv = ptr<const uint8_t>(b); it.d_dst = ptr<uint8_t>(c);
    }
    const int rc = call == 0 ? bsx::blur_bgr_batch_plan(null_items ? nullptr : blur.data(), n, n_streams, &plan)
                 : call == 1 ? bsx::resize_bgr_batch_plan(null_items ? nullptr : resize.data(), n, n_streams, dw, dh, &plan)
                             : bsx::blur_surfaces_plan(null_items ? nullptr : surf.data(), n, n_streams, &plan);
    printf("%d %d %d %zu |", rc, plan.bad, plan.n_sizes, plan.cls.size());
    for (int v : plan.cls) printf(" %d", v);
    printf(" |");
    for (int v : plan.order) printf(" %d", v);
    printf(" |");
    for (int s = 0; s < plan.n_sizes; s++) printf(" %d %d", plan.sizes[s][0], plan.sizes[s][1]);
    printf(" |");
    for (int v : plan.pos) printf(" %d", v);
    printf(" |");
    for (int v : plan.wg) printf(" %d", v);
    printf(" |");
    for (int v : plan.per) printf(" %d", v);
    printf(" |");
    for (int v : plan.ntx) printf(" %d", v);
    printf("\n%s\n", plan.text);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    d = tmp_path_factory.mktemp("picture_batch_plan")
    src, exe = d / "main.cpp", str(d / "plan")
    src.write_text(MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC,
                           "-o", exe, str(src)])

    def run(call, cases):
        """cases: (items or None, n or None, n_streams[, dw, dh]) -> the planner's answer per case as a dict"""
        text = []
        for items, n, n_streams, *out in cases:
            null = items is None
            items = items or []
            text.append("%d %d %d %d %d %d" % ((call, len(items) if n is None else n, n_streams, int(null)) + (tuple(out) or (0, 0))))
            text += [" ".join("%d" % v for v in it) for it in items]
        r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, "the planner's program failed (a sanitizer report?):\n" + r.stderr[-3000:]
        lines = r.stdout.split("\n")
        assert len(lines) == 2 * len(cases) + 1, r.stdout[-500:]
        res = []
        for k in range(len(cases)):
            head, cls, order, sizes, pos, wg, per, ntx = ([int(v) for v in part.split()] for part in lines[2 * k].split("|"))
            rc, bad, n_sizes, n_cls = head
            assert len(cls) == n_cls and len(sizes) == 2 * n_sizes and len(pos) == len(wg) == MAX_SIZES + 1 and len(per) == len(ntx) == MAX_SIZES
            res.append(dict(rc=rc, bad=bad, cls=cls, order=order, sizes=list(zip(sizes[::2], sizes[1::2])), pos=pos, wg=wg, per=per, ntx=ntx, text=lines[2 * k + 1]))
        return res
    return run


def _refused(planner, call, cases):
    """cases: (items, n, n_streams[, dw, dh], bad, text)"""
    for (*_c, bad, text), p in zip(cases, planner(call, [c[:-2] for c in cases])):
        assert p["rc"] == 1 and p["bad"] == bad and p["text"] == text, (text, p)


# ---- bsx_gaussian_blur_bgr_batch: items (src, dst, w, h, ksize, flags) ------------------------------------------------------------------------------------------------
def _blur(w, h, k, slot, flags=0):
    """picture number `slot`: its source and its destination in regions of their own, 4 GiB apart"""
    return ((2 * slot + 2) << 32, (2 * slot + 3) << 32, w, h, k, flags)


def _check_blur_plan(items, p):
    """every property of an accepted plan, from the items alone"""
    assert p["rc"] == 0 and p["text"] == "" and p["bad"] == -1, p
    sizes = []
    for it in items:
        if (it[2], it[3]) not in sizes:
            sizes.append((it[2], it[3]))
    assert p["sizes"] == sizes                                                       # numbered in the order of first appearance
    assert p["cls"] == [sizes.index((it[2], it[3])) for it in items]
    assert p["order"] == sorted(range(len(items)), key=lambda i: p["cls"][i])        # (sorted is stable)
    pos, wg = [0], [0]
    for g in range(MAX_SIZES):
        w, h = sizes[g] if g < len(sizes) else (0, 0)
        ntx, per = (w + 63) // 64, ((w + 63) // 64) * ((h + 15) // 16)
        cnt = sum(1 for c in p["cls"] if c == g)
        assert (g < len(sizes)) == (cnt > 0)
        assert p["ntx"][g] == ntx and p["per"][g] == per, (g, sizes, p)
        pos.append(pos[-1] + cnt)
        wg.append(wg[-1] + cnt * per)
    assert p["pos"] == pos and p["wg"] == wg, (p, pos, wg)
    assert pos[-1] == len(items) and wg[-1] == sum(((it[2] + 63) // 64) * ((it[3] + 15) // 16) for it in items)


def test_blur_batch_numbers_classes_orders_stably_and_builds_the_ragged_grid(planner):
    rng = np.random.default_rng(20261)
    # the GPU test's shape: sizes interleaved, BGR and YUYV mixed, the first size again at the end
    fleet = [(640, 480), (66, 18), (64, 16), (20, 12), (2, 2), (41, 30), (130, 70), (322, 242)]
    cases = [([_blur(w, h, 5, s, YIN if w % 2 == 0 and s % 2 else 0) for s, (w, h) in enumerate(fleet)] + [_blur(640, 480, 9, 8)], None, 16)]
    cases.append(([_blur(w, h, 25, s) for s, (w, h) in enumerate([(7, 5), (9, 3)] * 4)], None, 8))       # A B A B ...: n == n_streams
    cases.append(([], None, 4))                                                                          # n == 0
    cases.append((None, 0, 4))                                                                           # ... with items NULL
    cases.append(([_blur(1, 1, 1, 0)], None, 1))
    for _ in range(200):
        pool = [(int(rng.integers(1, 300)), int(rng.integers(1, 200))) for _ in range(int(rng.integers(1, MAX_SIZES + 1)))]
        items = []
        for s in range(int(rng.integers(1, 40))):
            w, h = pool[int(rng.integers(0, len(pool)))]
            items.append(_blur(w, h, 1 + 2 * int(rng.integers(0, 16)), s, YIN if w % 2 == 0 and rng.integers(0, 2) else 0))
        cases.append((items, None, len(items) + int(rng.integers(0, 3))))
    got = planner(BLUR, cases)
    for (items, _n, _ns), p in zip(cases, got):
        _check_blur_plan(items or [], p)
    # the second case, spelled out: two classes of four, 1 x 1 tiles
    p = got[1]
    assert p["cls"] == [0, 1] * 4 and p["order"] == [0, 2, 4, 6, 1, 3, 5, 7] and p["pos"] == [0, 4] + [8] * 7 and p["wg"] == [0, 4] + [8] * 7
    assert p["per"] == [1, 1] + [0] * 6 and p["ntx"] == [1, 1] + [0] * 6


def test_blur_batch_refuses_each_bad_item_with_its_index(planner):
    ok = [_blur(64, 16, 25, 0), _blur(66, 18, 5, 1, YIN), _blur(64, 16, 9, 2)]
    S, D = 40 << 32, 41 << 32

    def at(i, **kw):
        """the good call with one more item at place i: 8 x 6 BGR, ksize 5, fields replaced"""
        f = dict(src=S, dst=D, w=8, h=6, k=5, flags=0)
        f.update(kw)
        r = list(ok)
        r.insert(i, (f["src"], f["dst"], f["w"], f["h"], f["k"], f["flags"]))
        return r
    _refused(planner, BLUR, [
        ([], -2, 8, -1, "n = -2 is negative"),
        (ok, None, 2, -1, "n = 3 exceeds the context's 2 streams"),
        (None, 3, 8, -1, "items is NULL"),
        (at(2, w=0), None, 8, 2, "items[2]: size 0 x 6 is not positive"),
        (at(0, h=-6), None, 8, 0, "items[0]: size 8 x -6 is not positive"),
        (at(1, k=0), None, 8, 1, "items[1]: ksize 0 is not an odd number of 1 .. 31"),
        (at(1, k=2), None, 8, 1, "items[1]: ksize 2 is not an odd number of 1 .. 31"),
        (at(3, k=33), None, 8, 3, "items[3]: ksize 33 is not an odd number of 1 .. 31"),
        (at(2, src=0), None, 8, 2, "items[2]: d_src is NULL"),
        (at(3, dst=0), None, 8, 3, "items[3]: d_dst is NULL"),
        (at(1, flags=1), None, 8, 1, "items[1]: flags 0x1 has bits outside yuyv-in (0x40)"),
        (at(1, flags=0x140), None, 8, 1, "items[1]: flags 0x140 has bits outside yuyv-in (0x40)"),
        (at(1, w=7, flags=YIN), None, 8, 1, "items[1]: a YUYV source needs an even width (w = 7)"),
        (at(1, src=S + 2, flags=YIN), None, 8, 1, "items[1]: YUYV d_src 0x%x is not 4-byte aligned" % (S + 2)),
        # w * h * 3 == 2^31 + 2^16
        (at(2, w=32768, h=21846), None, 8, 2, "items[2]: size 32768 x 21846 is beyond the kernel's 32-bit offsets (w * h * 3 < 2^31)"),
        # two rules broken: the call names the one it judges first — size, ksize, d_src, d_dst, flags, the YUYV width, the YUYV address, the extent
        (at(1, w=0, k=2), None, 8, 1, "items[1]: size 0 x 6 is not positive"),
        (at(1, k=2, src=0), None, 8, 1, "items[1]: ksize 2 is not an odd number of 1 .. 31"),
        (at(1, dst=0, flags=1), None, 8, 1, "items[1]: d_dst is NULL"),
        (at(1, w=7, flags=YIN | 1), None, 8, 1, "items[1]: flags 0x41 has bits outside yuyv-in (0x40)"),
        (at(1, w=7, src=S + 2, flags=YIN), None, 8, 1, "items[1]: a YUYV source needs an even width (w = 7)"),
        (at(0, w=32768, h=21846, src=S + 1, flags=YIN), None, 8, 0, "items[0]: YUYV d_src 0x%x is not 4-byte aligned" % (S + 1)),
        (at(0, k=4) + [(S, D, 8, 0, 5, 0)], None, 8, 0, "items[0]: ksize 4 is not an odd number of 1 .. 31"),      # the items in index order
    ])
    # accepted: a BGR source of any alignment and of odd width; 65532 x 10922 x 3 = 2^31 - 262136 bytes
    fine = [(at(1, src=S + 1, w=7), None, 8), (at(1, w=65532, h=10922), None, 8), (at(3, flags=YIN), None, 4)]
    for (items, _n, _ns), p in zip(fine, planner(BLUR, fine)):
        _check_blur_plan(items, p)


def test_blur_batch_takes_eight_sizes_and_refuses_a_ninth(planner):
    sizes = [(8 + 4 * i, 6 + 2 * i) for i in range(9)]
    eight = [_blur(w, h, 5, s) for s, (w, h) in enumerate(sizes[:8])]
    cases = [(eight + [_blur(*sizes[0], 7, 9)], None, 16), (eight + [_blur(*sizes[3], 5, 9), _blur(*sizes[8], 5, 10)], None, 16), ([_blur(*sizes[8], 5, 10)] + eight, None, 16)]
    a, b, c = planner(BLUR, cases)
    _check_blur_plan(cases[0][0], a)
    assert b["rc"] == 1 and b["bad"] == 9 and b["text"] == "items[9]: 40 x 22 is distinct size 9 of the call (at most 8)"
    assert c["rc"] == 1 and c["bad"] == 8 and c["text"] == "items[8]: 36 x 20 is distinct size 9 of the call (at most 8)"


def test_blur_batch_overlaps(planner):
    B = 1 << 36
    px = 64 * 16
    good = (B, B + (1 << 20), 64, 16, 5, 0)                    # source [B, B + 3072), destination [B + 1 MiB, + 3072)
    ysrc = B + (1 << 24)
    _refused(planner, BLUR, [
        # a destination over its own source by one byte, BGR and YUYV (a YUYV source ends after w * h * 2 bytes)
        ([(B, B + px * 3 - 1, 64, 16, 5, 0)], None, 8, 0, "items[0]: d_dst 0x%x overlaps the source of items[0] (0x%x)" % (B + px * 3 - 1, B)),
        ([(B, B + px * 2 - 1, 64, 16, 5, YIN)], None, 8, 0, "items[0]: d_dst 0x%x overlaps the source of items[0] (0x%x)" % (B + px * 2 - 1, B)),
        # ... over another item's source, judged on the YUYV source's 2 bytes per pixel
        ([(ysrc, B + (1 << 25), 64, 16, 5, YIN), (B, ysrc + px * 2 - 1, 2, 2, 3, 0)], None, 8, 1,
         "items[1]: d_dst 0x%x overlaps the source of items[0] (0x%x)" % (ysrc + px * 2 - 1, ysrc)),
        ([good, (ysrc, B + 5, 2, 2, 3, YIN)], None, 8, 1, "items[1]: d_dst 0x%x overlaps the source of items[0] (0x%x)" % (B + 5, B)),
        # ... over another destination by one byte
        ([good, (B, B + (1 << 20) + px * 3 - 1, 2, 2, 3, 0)], None, 8, 1,
         "items[1]: d_dst 0x%x overlaps the destination of items[0] (0x%x)" % (B + (1 << 20) + px * 3 - 1, B + (1 << 20))),
    ])
    # allowed: a destination right behind a YUYV source's last byte (inside what a BGR source of the size would span), right behind a BGR source, one source twice
    fine = [
        [(B, B + px * 2, 64, 16, 5, YIN)],
        [(ysrc, B + (1 << 25), 64, 16, 5, YIN), (B, ysrc + px * 2, 2, 2, 3, 0)],
        [(B, B + px * 3, 64, 16, 5, 0)],
        [good, (B, B + (1 << 21), 64, 16, 9, 0)],
    ]
    for items, p in zip(fine, planner(BLUR, [(items, None, 8) for items in fine])):
        _check_blur_plan(items, p)
    # ... and the second of them is refused where the source is BGR: the same addresses, 3 bytes per pixel
    (p,) = planner(BLUR, [([(ysrc, B + (1 << 25), 64, 16, 5, 0), (B, ysrc + px * 2, 2, 2, 3, 0)], None, 8)])
    assert p["rc"] == 1 and p["bad"] == 1 and "overlaps the source of items[0]" in p["text"]


def test_blur_batch_grid_of_2_to_the_31_workgroups_is_too_large(planner):
    # 32766 x 21844 px is 512 x 1366 = 699392 tiles; 3071 of them make 2^31 + 334080 workgroups, 3070 stay below.  One source for all; the destinations 4 GiB apart
    assert 699392 * 3070 < 2 ** 31 <= 699392 * 3071
    big = [(1 << 32, (2 + i) << 32, 32766, 21844, 3, 0) for i in range(3071)]
    a, b = planner(BLUR, [(big, None, 4096), (big[:3070], None, 4096)])
    assert a["rc"] == 2 and a["text"] == ""
    _check_blur_plan(big[:3070], b)


# ---- bsx_resize_bgr_batch: items (src, sw, sh, dst), every one to dw x dh ---------------------------------------------------------------------------------------------
def _rsz(sw, sh, slot):
    return ((2 * slot + 2) << 32, sw, sh, (2 * slot + 3) << 32)


def _check_resize_plan(items, dw, dh, p):
    """one class, the caller's order, no ragged grid (the launch is (blocks, n) at dw x dh)"""
    n = len(items)
    assert p["rc"] == 0 and p["text"] == "" and p["bad"] == -1, p
    assert p["cls"] == [0] * n and p["order"] == list(range(n)) and p["sizes"] == ([(dw, dh)] if n else [])
    assert p["pos"] == [0] + [n] * MAX_SIZES and p["wg"] == [0] * (MAX_SIZES + 1) and p["per"] == [0] * MAX_SIZES and p["ntx"] == [0] * MAX_SIZES


def test_resize_batch_accepts_any_mix_of_source_sizes(planner):
    many = [_rsz(3 + s, 2 + s % 5, s) for s in range(12)]       # twelve source sizes: they are not classes
    cases = [(many, None, 12, 20, 12), ([_rsz(1, 1, 0)], None, 1, 1, 1), ([], None, 4, 20, 12), (None, 0, 4, 20, 12), ([], None, 4, 0, -3),      # (n == 0 asks no output size)
             ([_rsz(6, 4, 0), ((2 << 32) + 1, 6, 4, 9 << 32)], None, 2, 5, 3)]                                                               # one picture twice, any alignment
    for (items, _n, _ns, dw, dh), p in zip(cases, planner(RESIZE, cases)):
        _check_resize_plan(items or [], dw, dh, p)


def test_resize_batch_refusals(planner):
    ok = [_rsz(6, 4, 0), _rsz(8, 8, 1), _rsz(6, 4, 2)]
    B = 1 << 36
    bgr = 20 * 12 * 3

    def with_(i, item):
        return ok[:i] + [item] + ok[i + 1:]
    _refused(planner, RESIZE, [
        ([], -1, 8, 20, 12, -1, "n = -1 is negative"),
        (ok * 3, None, 8, 20, 12, -1, "n = 9 exceeds the context's 8 streams"),
        (None, 3, 8, 20, 12, -1, "items is NULL"),
        (ok, None, 8, 0, 12, -1, "output size 0 x 12 is not positive"),
        (ok, None, 8, 20, -1, -1, "output size 20 x -1 is not positive"),
        (with_(1, (0, 8, 8, 5 << 32)), None, 8, 20, 12, 1, "items[1]: d_src is NULL"),
        (with_(2, (6 << 32, 6, 4, 0)), None, 8, 20, 12, 2, "items[2]: d_dst is NULL"),
        (with_(1, (4 << 32, 0, 8, 5 << 32)), None, 8, 20, 12, 1, "items[1]: source size 0 x 8 is not positive"),
        (with_(0, (2 << 32, 6, -4, 3 << 32)), None, 8, 20, 12, 0, "items[0]: source size 6 x -4 is not positive"),
        # two rules broken: n before items before the output size before the items, an item's pointers before its size
        (None, 9, 8, 0, 0, -1, "n = 9 exceeds the context's 8 streams"),
        (None, 3, 8, 0, 0, -1, "items is NULL"),
        (with_(1, (0, 0, 8, 0)), None, 8, 0, 12, -1, "output size 0 x 12 is not positive"),
        (with_(1, (4 << 32, 0, 8, 0)), None, 8, 20, 12, 1, "items[1]: d_dst is NULL"),
        # a destination over another destination and over a source picture, each by one byte; over its own source
        ([(B, 6, 4, B + (1 << 20)), (B, 6, 4, B + (2 << 20)), (B, 6, 4, B + (2 << 20) + bgr - 1)], None, 8, 20, 12, 2,
         "items[2]: d_dst 0x%x overlaps the destination of items[1] (0x%x)" % (B + (2 << 20) + bgr - 1, B + (2 << 20))),
        ([(B, 6, 4, B + (1 << 20)), (B + 4096, 6, 4, B + (2 << 20)), (B, 6, 4, B + 4096 + 6 * 4 * 3 - 1)], None, 8, 20, 12, 2,
         "items[2]: d_dst 0x%x overlaps the source picture of items[1] (0x%x)" % (B + 4096 + 71, B + 4096)),
        ([(B, 6, 4, B + 71)], None, 8, 20, 12, 0, "items[0]: d_dst 0x%x overlaps the source picture of items[0] (0x%x)" % (B + 71, B)),
    ])
    fine = [([(B, 6, 4, B + 72), (B, 6, 4, B + 72 + bgr)], None, 8, 20, 12)]      # right behind the source's last byte, right behind the other destination's
    for (items, _n, _ns, dw, dh), p in zip(fine, planner(RESIZE, fine)):
        _check_resize_plan(items, dw, dh, p)


# ---- bsx_gaussian_blur_surfaces_batch: the rule test_blur_surfaces_host.py leaves out.  Items (y, uv, dst, pitch_y, pitch_uv, w, h, ksize, flags) ---------------------
def test_blur_surfaces_overlaps_are_judged_last_on_the_extent_to_w_of_the_last_row(planner):
    B = 1 << 36
    # surface A: 64 x 16 at pitches of 128 — Y [B, B + 1984), UV [B + 2048, B + 3008); 64 x 16 x 3 = 3072 bytes of destination
    def a(dst, w=64, h=16):
        return (B, B + 2048, dst, 128, 128, w, h, 5, 0)
    other = (B + (1 << 20), B + (1 << 20) + 4096, B + (1 << 21), 64, 64, 64, 16, 5, 0)      # another surface, its destination [B + 2 MiB, + 3072)
    _refused(planner, BLUR_SURFACES, [
        ([a(B + 1983)], None, 8, 0, "items[0]: d_dst 0x%x overlaps the Y plane of items[0] (0x%x)" % (B + 1983, B)),
        ([a(B + 3007)], None, 8, 0, "items[0]: d_dst 0x%x overlaps the UV plane of items[0] (0x%x)" % (B + 3007, B + 2048)),
        ([other, a(B + (1 << 21) + 3071)], None, 8, 1, "items[1]: d_dst 0x%x overlaps the destination of items[0] (0x%x)" % (B + (1 << 21) + 3071, B + (1 << 21))),
        ([a(B + (1 << 22)), other[:2] + (B + 100,) + other[3:]], None, 8, 1, "items[1]: d_dst 0x%x overlaps the Y plane of items[0] (0x%x)" % (B + 100, B)),
        ([a(B + (1 << 22)), other[:2] + (B + 3007,) + other[3:]], None, 8, 1, "items[1]: d_dst 0x%x overlaps the UV plane of items[0] (0x%x)" % (B + 3007, B + 2048)),
        ([a(B + (1 << 22)), a(B + 3008), (B, B + 2048, 0, 128, 128, 64, 16, 5, 0)], None, 8, 2, "items[2]: d_dst is NULL"),      # an item's own rules first
    ])
    # allowed: a 2 x 2 destination (12 bytes) in the padding [w, pitch) of the Y plane's last row; right behind the UV plane's last byte; two items on one surface
    fine = [[(B, B + 2048, B + 1984 + 2, 128, 128, 2, 2, 5, 0)], [a(B + 3008)], [a(B + (1 << 22)), a(B + (1 << 23))]]
    for items, p in zip(fine, planner(BLUR_SURFACES, [(items, None, 8) for items in fine])):
        assert p["rc"] == 0 and p["text"] == "" and p["bad"] == -1 and p["order"] == list(range(len(items))), p
    # this call judges the grid before the overlaps: 3071 surfaces of 699392 tiles, all on one destination, are too large before they are overlapping
    big = [(1 << 32, 2 << 32, 3 << 32, 32768, 32768, 32766, 21844, 3, 0)] * 3071
    a_, b_ = planner(BLUR_SURFACES, [(big, None, 4096), (big[:2], None, 4096)])
    assert a_["rc"] == 2 and a_["text"] == ""
    assert b_["rc"] == 1 and "overlaps the destination of items[" in b_["text"]      # (equal addresses: which of the two is named first is the sort's choice)
