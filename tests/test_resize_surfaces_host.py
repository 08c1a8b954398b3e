"""bsx_resize_surfaces_batch's planner (csrc/picture_batch_plan.hpp) on a box without a GPU, driven by a stand-alone program built with the host sanitizers and run
directly: the destination-size classes numbered in the order of their first item, the stable order of interleaved classes, the ragged grid (GeomSpans) against a
restatement in Python, every refusal with its text and index, eight output sizes accepted and a ninth refused, a grid of 2^31 workgroups, and the overlaps — judged on
a plane's extent to byte sw of its last row."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "backscrub_amd", "csrc")
MAX_SIZES = 8

MAIN = r"""
// reads cases from stdin: "n n_streams null_items", then (none with null_items) max(n, 0) items "y uv dst pitch_y pitch_uv sw sh dw dh flags reserved"; prints the
// planner's answer as one line of integers "rc bad n_sizes n_cls | cls.. | order.. | sizes.. | pos[9] | wg[9] | per[8]" and the refusal text on the next line
#include <cstdio>
#include <vector>
#include "picture_batch_plan.hpp"
int main() {
  static_assert(sizeof(bsx_resize_surface_item) == 56, "the item of the header");
  int n, n_streams, null_items;
  while (scanf("%d %d %d", &n, &n_streams, &null_items) == 3) {
    std::vector<bsx_resize_surface_item> items((size_t)(n > 0 && !null_items ? n : 0));      // exactly n items: a read past the end is the sanitizer's to report
    for (bsx_resize_surface_item& it : items) {
      unsigned long long y, uv, dst;
      if (scanf("%llu %llu %llu %d %d %d %d %d %d %u %d", &y, &uv, &dst, &it.pitch_y, &it.pitch_uv, &it.sw, &it.sh, &it.dw, &it.dh, &it.flags, &it.reserved) != 11) return 2;
      it.d_y = reinterpret_cast<const uint8_t*>((uintptr_t)y);
      it.d_uv = reinterpret_cast<const uint8_t*>((uintptr_t)uv);
      it.d_dst = reinterpret_cast<uint8_t*>((uintptr_t)dst);
    }
    bsx::PictureBatchPlan plan;
    const int rc = bsx::resize_surfaces_plan(null_items ? nullptr : items.data(), n, n_streams, &plan);
    printf("%d %d %d %zu |", rc, plan.bad, plan.n_sizes, plan.cls.size());
    for (int c : plan.cls) printf(" %d", c);
    printf(" |");
    for (int q : plan.order) printf(" %d", q);
    printf(" |");
    for (int s = 0; s < plan.n_sizes; s++) printf(" %d %d", plan.sizes[s][0], plan.sizes[s][1]);
    printf(" |");
    for (int v : plan.pos) printf(" %d", v);
    printf(" |");
    for (int v : plan.wg) printf(" %d", v);
    printf(" |");
    for (int v : plan.per) printf(" %d", v);
    printf("\n%s\n", plan.text);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    d = tmp_path_factory.mktemp("resize_surfaces_plan")
    src, exe = d / "main.cpp", str(d / "plan")
    src.write_text(MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC,
                           "-o", exe, str(src)])

    def run(cases):
        """cases: (items or None, n or None, n_streams) -> the planner's answer per case as a dict"""
        text = []
        for items, n, n_streams in cases:
            null = items is None
            items = items or []
            text.append("%d %d %d" % (len(items) if n is None else n, n_streams, int(null)))
            text += ["%d %d %d %d %d %d %d %d %d %d %d" % it for it in items]
        r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, "the planner's program failed (a sanitizer report?):\n" + r.stderr[-3000:]
        lines = r.stdout.split("\n")
        assert len(lines) == 2 * len(cases) + 1, r.stdout[-500:]
        out = []
        for k in range(len(cases)):
            head, cls, order, sizes, pos, wg, per = ([int(v) for v in part.split()] for part in lines[2 * k].split("|"))
            rc, bad, n_sizes, n_cls = head
            assert len(cls) == n_cls and len(sizes) == 2 * n_sizes and len(pos) == len(wg) == MAX_SIZES + 1 and len(per) == MAX_SIZES
            out.append(dict(rc=rc, bad=bad, cls=cls, order=order, sizes=list(zip(sizes[::2], sizes[1::2])), pos=pos, wg=wg, per=per, text=lines[2 * k + 1]))
        return out
    return run


def _item(sw, sh, dw, dh, slot, pitch_y=None, pitch_uv=None, flags=0, reserved=0, dslot=None):
    """surface number `slot`: its planes 64 MiB apart; the destination in a region of its own, 8 MiB per `dslot` (default: one per call of this function)"""
    base = (slot + 1) << 28
    if dslot is None:
        dslot = _item.next
        _item.next += 1
    return (base, base + (1 << 26), (1 << 40) + (dslot << 23), pitch_y or (sw + 3) // 4 * 4, pitch_uv or (sw + 3) // 4 * 4, sw, sh, dw, dh, flags, reserved)


_item.next = 0


def _per(dw, dh):
    return ((dw + 3) // 4 * dh + 255) // 256


def _check_plan(items, p):
    """every property of an accepted plan, from the items alone: class numbering in the order of first appearance, the stable order, GeomSpans"""
    assert p["rc"] == 0 and p["text"] == "" and p["bad"] == -1, p
    sizes = []
    for it in items:
        if (it[7], it[8]) not in sizes:
            sizes.append((it[7], it[8]))
    assert p["sizes"] == sizes
    assert p["cls"] == [sizes.index((it[7], it[8])) for it in items]
    assert p["order"] == sorted(range(len(items)), key=lambda i: p["cls"][i])      # (sorted is stable)
    pos, wg = [0], [0]
    for g in range(MAX_SIZES):
        live = g < len(sizes)
        per = _per(*sizes[g]) if live else 0
        cnt = sum(1 for c in p["cls"] if c == g)
        assert live == (cnt > 0)
        assert p["per"][g] == per, (g, sizes, p)
        pos.append(pos[-1] + cnt)
        wg.append(wg[-1] + cnt * per)
    assert p["pos"] == pos and p["wg"] == wg, (p, pos, wg)
    assert pos[-1] == len(items) and wg[-1] == sum(_per(it[7], it[8]) for it in items)


# the GPU test's fleet (tests/test_gpu_resize_surfaces.py): (sw, sh, pitch_y, pitch_uv, dw, dh, surface)
FLEET = [(2, 2, 4, 4, 5, 3, 0), (322, 182, 384, 328, 160, 96, 1), (6, 4, 8, 8, 6, 4, 2), (66, 34, 128, 72, 20, 12, 3), (24, 12, 24, 24, 12, 6, 4),
         (322, 182, 384, 328, 160, 96, 5), (18, 10, 20, 20, 20, 12, 6), (66, 34, 128, 72, 21, 11, 3), (16, 8, 16, 16, 36, 20, 7), (66, 34, 128, 72, 160, 96, 3)]


def test_planner_numbers_classes_orders_stably_and_builds_the_ragged_grid(planner):
    rng = np.random.default_rng(20251)
    fleet = [_item(sw, sh, dw, dh, s, py, puv) for sw, sh, py, puv, dw, dh, s in FLEET]
    cases = [(fleet, None, 16)]
    cases.append(([_item(1920, 1080, 1920, 1080, 0, 2048)] + [_item(1280, 720, 160, 90, 1 + s) for s in range(30)] + [_item(1920, 1080, 1920, 1080, 0, 2048)], None, 32))
    cases.append(([_item(1280, 720, w, h, s % 2) for s, (w, h) in enumerate([(640, 480), (1280, 720)] * 4)], None, 8))       # A B A B ...: n == n_streams
    cases.append(([], None, 4))                                                                                 # n == 0
    cases.append((None, 0, 4))                                                                                  # ... with items NULL
    cases.append(([_item(2, 2, 1, 1, 0, 4, 4)], None, 1))
    for _ in range(300):
        pool = [(int(rng.integers(1, 2000)), int(rng.integers(1, 1200))) for _ in range(int(rng.integers(1, MAX_SIZES + 1)))]
        n = int(rng.integers(1, 40))
        items = []
        for s in range(n):
            dw, dh = pool[int(rng.integers(0, len(pool)))]
            sw, sh = 2 * int(rng.integers(1, 1000)), 2 * int(rng.integers(1, 600))
            items.append(_item(sw, sh, dw, dh, int(rng.integers(0, 12)), (sw + 3) // 4 * 4 + 4 * int(rng.integers(0, 64)), (sw + 3) // 4 * 4 + 4 * int(rng.integers(0, 64))))
        cases.append((items, None, n + int(rng.integers(0, 3))))
    got = planner(cases)
    for (items, _n, _ns), p in zip(cases, got):
        _check_plan(items or [], p)
    # the fleet, spelled out: seven classes in the order of their first item; 160 x 96 has three positions of 15 workgroups
    p = got[0]
    assert p["sizes"] == [(5, 3), (160, 96), (6, 4), (20, 12), (12, 6), (21, 11), (36, 20)]
    assert p["cls"] == [0, 1, 2, 3, 4, 1, 3, 5, 6, 1] and p["order"] == [0, 1, 5, 9, 2, 3, 6, 4, 7, 8]
    assert p["per"] == [1, 15, 1, 1, 1, 1, 1, 0] and p["pos"] == [0, 1, 4, 5, 7, 8, 9, 10, 10] and p["wg"] == [0, 1, 46, 47, 49, 50, 51, 52, 52]


def test_planner_refuses_each_bad_item_with_its_index(planner):
    ok = [_item(1280, 720, 640, 480, 0, 1408, 1344), _item(66, 18, 20, 12, 1, 68, 72), _item(1280, 720, 320, 240, 0, 1408, 1344)]
    Y, UV, D = 9 << 28, (9 << 28) + (1 << 26), (9 << 28) + (2 << 26)
    names = ("y", "uv", "dst", "pitch_y", "pitch_uv", "sw", "sh", "dw", "dh", "flags", "reserved")

    def at(i, **kw):
        """the good call with one more item at place i: 64 x 32 -> 20 x 12, tight pitches, fields replaced"""
        f = dict(y=Y, uv=UV, dst=D, pitch_y=64, pitch_uv=64, sw=64, sh=32, dw=20, dh=12, flags=0, reserved=0)
        f.update(kw)
        r = list(ok)
        r.insert(i, tuple(f[k] for k in names))
        return r
    G = 1 << 30
    cases = [
        ([], -2, 8, -1, "n = -2 is negative"),
        (ok, None, 2, -1, "n = 3 exceeds the context's 2 streams"),
        (None, 3, 8, -1, "items is NULL"),
        (at(2, y=0), None, 8, 2, "items[2]: d_y is NULL"),
        (at(2, uv=0), None, 8, 2, "items[2]: d_uv is NULL"),
        (at(3, dst=0), None, 8, 3, "items[3]: d_dst is NULL"),
        (at(1, y=Y + 2), None, 8, 1, "items[1]: d_y 0x%x is not 4-byte aligned" % (Y + 2)),
        (at(1, uv=UV + 1), None, 8, 1, "items[1]: d_uv 0x%x is not 4-byte aligned" % (UV + 1)),
        (at(2, sw=0), None, 8, 2, "items[2]: source size 0 x 32 is not positive"),
        (at(0, sh=-6), None, 8, 0, "items[0]: source size 64 x -6 is not positive"),
        (at(1, sw=65, pitch_y=68, pitch_uv=68), None, 8, 1, "items[1]: NV12 needs an even width and height (65 x 32)"),
        (at(3, sh=33), None, 8, 3, "items[3]: NV12 needs an even width and height (64 x 33)"),
        (at(0, pitch_y=60), None, 8, 0, "items[0]: pitch_y = 60 is below sw = 64"),
        (at(2, pitch_y=66), None, 8, 2, "items[2]: pitch_y = 66 is not a multiple of 4"),
        (at(2, pitch_uv=0), None, 8, 2, "items[2]: pitch_uv = 0 is below sw = 64"),
        (at(3, pitch_uv=70), None, 8, 3, "items[3]: pitch_uv = 70 is not a multiple of 4"),
        (at(1, dw=0), None, 8, 1, "items[1]: output size 0 x 12 is not positive"),
        (at(3, dh=-1), None, 8, 3, "items[3]: output size 20 x -1 is not positive"),
        (at(1, flags=1), None, 8, 1, "items[1]: flags 0x1: this call takes no flags"),
        (at(1, flags=64), None, 8, 1, "items[1]: flags 0x40: this call takes no flags"),
        (at(2, reserved=7), None, 8, 2, "items[2]: reserved = 7 is not 0"),
        (at(2, reserved=-1), None, 8, 2, "items[2]: reserved = -1 is not 0"),
        # planes past 2^31 bytes by their pitch alone (65536 x 32769 + 64, 131072 x 16385 + 64)
        (at(1, sh=32770, pitch_y=65536), None, 8, 1, "items[1]: the Y plane (32770 rows of pitch_y = 65536) extends over 2 GiB or more"),
        (at(1, sh=32772, pitch_uv=2 * 65536), None, 8, 1, "items[1]: the UV plane (16386 rows of pitch_uv = 131072) extends over 2 GiB or more"),
        (at(0, sh=2, pitch_y=2 * G - 4), None, 8, 0, "items[0]: the Y plane (2 rows of pitch_y = 2147483644) extends over 2 GiB or more"),
        # dw * dh * 3 == 2^31 + 2^16
        (at(2, dw=32768, dh=21846), None, 8, 2, "items[2]: output size 32768 x 21846 is beyond the kernel's 32-bit offsets (dw * dh * 3 < 2^31)"),
    ]
    got = planner([(items, n, ns) for items, n, ns, _bad, _text in cases])
    for (items, n, ns, bad, text), p in zip(cases, got):
        assert p["rc"] == 1 and p["bad"] == bad and p["text"] == text, (text, p)
    # just below the limits: a Y plane of 65532 x 32767 + 64 bytes; 65532 x 10922 x 3 = 2^31 - 262136 bytes of BGR (the destinations far from every plane)
    fine = [(at(1, sh=32768, pitch_y=65536 - 4, dst=1 << 45), None, 8), (at(1, dw=65532, dh=10922, dst=1 << 44), None, 8)]
    for (items, _n, _ns), p in zip(fine, planner(fine)):
        _check_plan(items, p)


def test_eight_sizes_pass_and_a_ninth_is_refused(planner):
    sizes = [(8 + 3 * i, 5 + 2 * i) for i in range(9)]
    eight = [_item(64 + 2 * s, 32, w, h, s) for s, (w, h) in enumerate(sizes[:8])]      # eight source sizes too
    again = _item(400, 300, *sizes[3], 9)                                               # a ninth source size into the fourth output size: no new class
    ninth = _item(64, 32, *sizes[8], 8)
    cases = [(eight + [again], None, 16), (eight + [again, ninth], None, 16), ([ninth] + eight, None, 16)]
    a, b, c = planner(cases)
    _check_plan(cases[0][0], a)
    assert a["cls"][8] == 3
    assert b["rc"] == 1 and b["bad"] == 9 and b["text"] == "items[9]: 32 x 21 is distinct output size 9 of the call (at most 8)"
    assert c["rc"] == 1 and c["bad"] == 8 and c["text"] == "items[8]: 29 x 19 is distinct output size 9 of the call (at most 8)"


def test_a_grid_of_2_to_the_31_workgroups_is_too_large(planner):
    # 32766 x 21844 px is 8192 x 21844 groups of four = 699008 workgroups; 3073 of them make 2^31 + 567936, 3072 stay below.  The destinations must not overlap: 2 GiB apart
    per = _per(32766, 21844)
    assert per == 699008 and per * 3072 < 2 ** 31 <= per * 3073
    big = [_item(64, 32, 32766, 21844, 0, dslot=256 * i) for i in range(3073)]
    a, b = planner([(big, None, 4096), (big[:3072], None, 4096)])
    assert a["rc"] == 2 and a["text"] == ""
    _check_plan(big[:3072], b)


def test_overlaps_are_judged_on_the_extent_to_sw_of_the_last_row(planner):
    B = 1 << 36
    # surface A: 64 x 16 at pitches of 128 — Y [B, B + 1984), UV [B + 2048, B + 3008); 20 x 12 x 3 = 720 bytes of destination
    def a(dst, dw=20, dh=12):
        return (B, B + 2048, dst, 128, 128, 64, 16, dw, dh, 0, 0)
    other = (B + (1 << 20), B + (1 << 20) + 4096, B + (1 << 21), 64, 64, 64, 16, 20, 12, 0, 0)      # another surface, its destination [B + 2 MiB, + 720)
    cases = [
        ([a(B + 1984 - 1)], 0, "items[0]: d_dst 0x%x overlaps the Y plane of items[0] (0x%x)" % (B + 1983, B)),                # its own Y plane, by one byte
        ([a(B + 1986, 7, 3)], 0, "items[0]: d_dst 0x%x overlaps the UV plane of items[0] (0x%x)" % (B + 1986, B + 2048)),      # 63 bytes from inside the Y plane's padding: its own UV plane, by its last byte
        ([other, a(B + (1 << 21) + 719)], 1, "items[1]: d_dst 0x%x overlaps the destination of items[0] (0x%x)" % (B + (1 << 21) + 719, B + (1 << 21))),
        ([a(B + (1 << 22)), (other[0], other[1], B + 3007) + other[3:]], 1,
         "items[1]: d_dst 0x%x overlaps the UV plane of items[0] (0x%x)" % (B + 3007, B + 2048)),                               # another item's plane, by one byte
        ([a(B + (1 << 22)), (other[0], other[1], B + 100) + other[3:]], 1, "items[1]: d_dst 0x%x overlaps the Y plane of items[0] (0x%x)" % (B + 100, B)),
    ]
    for (items, bad, text), p in zip(cases, planner([(items, None, 8) for items, _b, _t in cases])):
        assert p["rc"] == 1 and p["bad"] == bad and p["text"] == text, (text, p)
    # allowed: a destination in the padding [sw, pitch) of the Y plane's last row (64 bytes: 5 x 4 x 3 = 60), its own surface's or another's; right behind the UV
    # plane's last byte; two items on one surface
    fine = [
        [a(B + 1984, 5, 4)],
        [a(B + (1 << 22)), (other[0], other[1], B + 1984) + other[3:7] + (5, 4, 0, 0)],
        [a(B + 3008)],
        [a(B + (1 << 22)), a(B + (1 << 23), 36, 20)],
    ]
    for items, p in zip(fine, planner([(items, None, 8) for items in fine])):
        _check_plan(items, p)
    # ... and one byte earlier it is not
    (p,) = planner([([a(B + 1983, 5, 4)], None, 8)])
    assert p["rc"] == 1 and "overlaps the Y plane of items[0]" in p["text"]
