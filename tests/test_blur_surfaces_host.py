"""bsx_gaussian_blur_surfaces_batch's planner (csrc/picture_batch_plan.hpp; its overlap rule: test_picture_batch_host.py) on a box without a GPU, driven by a stand-alone program built with the host sanitizers and run
directly: every refusal with its text and index, the size classes of accepted calls whose sizes are interleaved, the ragged grid (GeomSpans) and the tiles per row
(BlurTileCols) against a restatement in Python, eight sizes accepted and a ninth refused."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "backscrub_amd", "csrc")
MAX_SIZES = 8

MAIN = r"""
// reads cases from stdin: "n n_streams null_items", then (none with null_items) max(n, 0) items "y uv dst pitch_y pitch_uv w h ksize flags"; prints the planner's
// answer as one line of integers "rc bad n_sizes n_cls | cls.. | sizes.. | pos[9] | wg[9] | per[8] | ntx[8]" and the refusal text on the next line
#include <cstdio>
#include <vector>
#include "picture_batch_plan.hpp"
int main() {
  static_assert(sizeof(bsx_blur_surface_item) == 48, "the item of the header");
  int n, n_streams, null_items;
  while (scanf("%d %d %d", &n, &n_streams, &null_items) == 3) {
    std::vector<bsx_blur_surface_item> items((size_t)(n > 0 && !null_items ? n : 0));      // exactly n items: a read past the end is the sanitizer's to report
    for (bsx_blur_surface_item& it : items) {
      unsigned long long y, uv, dst;
      if (scanf("%llu %llu %llu %d %d %d %d %d %u", &y, &uv, &dst, &it.pitch_y, &it.pitch_uv, &it.w, &it.h, &it.ksize, &it.flags) != 9) return 2;
      it.d_y = reinterpret_cast<const uint8_t*>((uintptr_t)y);
      it.d_uv = reinterpret_cast<const uint8_t*>((uintptr_t)uv);
      it.d_dst = reinterpret_cast<uint8_t*>((uintptr_t)dst);
    }
    bsx::PictureBatchPlan plan;      // (blur_surfaces_grid: the call's plan without its last rule, the overlaps — the surfaces of these cases share addresses)
    const int rc = bsx::blur_surfaces_grid(null_items ? nullptr : items.data(), n, n_streams, &plan);
    printf("%d %d %d %zu |", rc, plan.bad, plan.n_sizes, plan.cls.size());
    for (int c : plan.cls) printf(" %d", c);
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
    d = tmp_path_factory.mktemp("blur_surfaces_plan")
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
            text += ["%d %d %d %d %d %d %d %d %d" % it for it in items]
        r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, "the planner's program failed (a sanitizer report?):\n" + r.stderr[-3000:]
        lines = r.stdout.split("\n")
        assert len(lines) == 2 * len(cases) + 1, r.stdout[-500:]
        out = []
        for k in range(len(cases)):
            head, cls, sizes, pos, wg, per, ntx = ([int(v) for v in part.split()] for part in lines[2 * k].split("|"))
            rc, bad, n_sizes, n_cls = head
            assert len(cls) == n_cls and len(sizes) == 2 * n_sizes and len(pos) == len(wg) == MAX_SIZES + 1 and len(per) == len(ntx) == MAX_SIZES
            out.append(dict(rc=rc, bad=bad, cls=cls, sizes=list(zip(sizes[::2], sizes[1::2])), pos=pos, wg=wg, per=per, ntx=ntx, text=lines[2 * k + 1]))
        return out
    return run


def _item(w, h, k, slot, pitch_y=None, pitch_uv=None, flags=0):
    """surface number `slot`: planes and destination 64 MiB apart"""
    base = (slot + 1) << 28
    return (base, base + (1 << 26), base + (2 << 26), pitch_y or (w + 3) // 4 * 4, pitch_uv or (w + 3) // 4 * 4, w, h, k, flags)


def _check_plan(items, p):
    """every property of an accepted plan, from the items alone: class numbering in the order of first appearance, GeomSpans and tiles per row"""
    assert p["rc"] == 0 and p["text"] == "" and p["bad"] == -1, p
    sizes = []
    for it in items:
        if (it[5], it[6]) not in sizes:
            sizes.append((it[5], it[6]))
    assert p["sizes"] == sizes
    assert p["cls"] == [sizes.index((it[5], it[6])) for it in items]
    pos, wg = [0], [0]
    for g in range(MAX_SIZES):
        live = g < len(sizes)
        w, h = sizes[g] if live else (0, 0)
        ntx, per = (w + 63) // 64, ((w + 63) // 64) * ((h + 15) // 16)
        cnt = sum(1 for c in p["cls"] if c == g)
        assert live == (cnt > 0)
        assert p["ntx"][g] == ntx and p["per"][g] == per, (g, sizes, p)
        pos.append(pos[-1] + cnt)
        wg.append(wg[-1] + cnt * per)
    assert p["pos"] == pos and p["wg"] == wg, (p, pos, wg)
    assert pos[-1] == len(items) and wg[-1] == sum(((it[5] + 63) // 64) * ((it[6] + 15) // 16) for it in items)


FLEET = [(640, 480), (66, 18), (64, 16), (20, 12), (2, 2), (40, 30), (130, 70), (322, 242)]


def test_planner_numbers_classes_and_builds_the_ragged_grid(planner):
    rng = np.random.default_rng(20243)
    cases = []
    # the GPU test's call: eight sizes interleaved, the first size again at the end
    nine = [_item(w, h, 5, s, (w + 3) // 4 * 4 + 64) for s, (w, h) in enumerate(FLEET)] + [_item(640, 480, 9, 0, 704)]
    cases.append((nine, None, 16))
    cases.append(([_item(1920, 1080, 25, 0, 2048)] + [_item(160, 90, 7, 1 + s) for s in range(30)] + [_item(1920, 1080, 7, 0, 2048)], None, 32))      # one large among many small
    cases.append(([_item(w, h, 25, s) for s, (w, h) in enumerate([(640, 480), (1280, 720)] * 4)], None, 8))       # A B A B ...: n == n_streams
    cases.append(([], None, 4))                                                                                 # n == 0
    cases.append((None, 0, 4))                                                                                  # ... with items NULL
    cases.append(([_item(2, 2, 1, 0, 4, 4)], None, 1))
    for _ in range(300):
        pool = [(2 * int(rng.integers(1, 1000)), 2 * int(rng.integers(1, 600))) for _ in range(int(rng.integers(1, MAX_SIZES + 1)))]
        n = int(rng.integers(1, 40))
        items = []
        for s in range(n):
            w, h = pool[int(rng.integers(0, len(pool)))]
            items.append(_item(w, h, 1 + 2 * int(rng.integers(0, 16)), int(rng.integers(0, 12)), (w + 3) // 4 * 4 + 4 * int(rng.integers(0, 64)),
                               (w + 3) // 4 * 4 + 4 * int(rng.integers(0, 64))))
        cases.append((items, None, n + int(rng.integers(0, 3))))
    for (items, _n, _ns), p in zip(cases, planner(cases)):
        _check_plan(items or [], p)


def test_planner_refuses_each_bad_item_with_its_index(planner):
    ok = [_item(640, 480, 25, 0, 768, 704), _item(66, 18, 5, 1, 68, 72), _item(640, 480, 9, 0, 768, 704)]
    Y, UV, D = 9 << 28, (9 << 28) + (1 << 26), (9 << 28) + (2 << 26)

    def at(i, **kw):
        """the good call with one more item at place i: 64 x 32, ksize 5, tight pitches, fields replaced"""
        f = dict(y=Y, uv=UV, dst=D, pitch_y=64, pitch_uv=64, w=64, h=32, k=5, flags=0)
        f.update(kw)
        r = list(ok)
        r.insert(i, (f["y"], f["uv"], f["dst"], f["pitch_y"], f["pitch_uv"], f["w"], f["h"], f["k"], f["flags"]))
        return r
    G = 1 << 30
    cases = [
        ([], -2, 8, -1, "n = -2 is negative"),
        (ok, None, 2, -1, "n = 3 exceeds the context's 2 streams"),
        (None, 3, 8, -1, "items is NULL"),
        (at(2, w=0), None, 8, 2, "items[2]: size 0 x 32 is not positive"),
        (at(0, h=-6), None, 8, 0, "items[0]: size 64 x -6 is not positive"),
        (at(1, w=65, pitch_y=68, pitch_uv=68), None, 8, 1, "items[1]: NV12 needs an even width and height (65 x 32)"),
        (at(3, h=33), None, 8, 3, "items[3]: NV12 needs an even width and height (64 x 33)"),
        (at(1, k=4), None, 8, 1, "items[1]: ksize 4 is not an odd number of 1 .. 31"),
        (at(1, k=0), None, 8, 1, "items[1]: ksize 0 is not an odd number of 1 .. 31"),
        (at(3, k=-1), None, 8, 3, "items[3]: ksize -1 is not an odd number of 1 .. 31"),
        (at(0, k=33), None, 8, 0, "items[0]: ksize 33 is not an odd number of 1 .. 31"),
        (at(2, y=0), None, 8, 2, "items[2]: d_y is NULL"),
        (at(2, uv=0), None, 8, 2, "items[2]: d_uv is NULL"),
        (at(3, dst=0), None, 8, 3, "items[3]: d_dst is NULL"),
        (at(1, y=Y + 2), None, 8, 1, "items[1]: d_y 0x%x is not 4-byte aligned" % (Y + 2)),
        (at(1, uv=UV + 1), None, 8, 1, "items[1]: d_uv 0x%x is not 4-byte aligned" % (UV + 1)),
        (at(0, pitch_y=60), None, 8, 0, "items[0]: pitch_y = 60 is below w = 64"),
        (at(2, pitch_y=66), None, 8, 2, "items[2]: pitch_y = 66 is not a multiple of 4"),
        (at(2, pitch_uv=0), None, 8, 2, "items[2]: pitch_uv = 0 is below w = 64"),
        (at(3, pitch_uv=70), None, 8, 3, "items[3]: pitch_uv = 70 is not a multiple of 4"),
        (at(1, flags=1), None, 8, 1, "items[1]: flags 0x1: this call takes no flags"),
        (at(1, flags=64), None, 8, 1, "items[1]: flags 0x40: this call takes no flags"),
        # w * h * 3 == 2^31 + ...: 32768 x 21846 x 3 = 2^31 + 2^16; the planes (715 MiB) are within bounds
        (at(2, w=32768, h=21846, pitch_y=32768, pitch_uv=32768), None, 8, 2, "items[2]: size 32768 x 21846 is beyond the kernel's 32-bit offsets (w * h * 3 < 2^31)"),
        # planes past 2^31 bytes by their pitch alone (65536 x 32769 + 64, 131072 x 16385 + 64); w * h * 3 is small
        (at(1, w=64, h=32770, pitch_y=65536, pitch_uv=64), None, 8, 1, "items[1]: the Y plane (32770 rows of pitch_y = 65536) extends over 2 GiB or more"),
        (at(1, w=64, h=32772, pitch_y=64, pitch_uv=2 * 65536), None, 8, 1, "items[1]: the UV plane (16386 rows of pitch_uv = 131072) extends over 2 GiB or more"),
        (at(0, w=64, h=2, pitch_y=2 * G - 4, pitch_uv=64), None, 8, 0, "items[0]: the Y plane (2 rows of pitch_y = 2147483644) extends over 2 GiB or more"),
    ]
    got = planner([(items, n, ns) for items, n, ns, _bad, _text in cases])
    for (items, n, ns, bad, text), p in zip(cases, got):
        assert p["rc"] == 1 and p["bad"] == bad and p["text"] == text, (text, p)
    # just below the limits: a Y plane of 65532 x 32767 + 64 bytes; 65532 x 10922 x 3 = 2^31 - 262136 bytes of BGR
    fine = [(at(1, w=64, h=32768, pitch_y=65536 - 4, pitch_uv=64), None, 8), (at(1, w=65532, h=10922, pitch_y=65536, pitch_uv=65536), None, 8)]
    for (items, _n, _ns), p in zip(fine, planner(fine)):
        _check_plan(items, p)


def test_eight_sizes_pass_and_a_ninth_is_refused(planner):
    sizes = [(8 + 4 * i, 6 + 2 * i) for i in range(9)]
    eight = [_item(w, h, 5, s) for s, (w, h) in enumerate(sizes[:8])]
    cases = [(eight + [eight[0]], None, 16), (eight + [eight[3], _item(*sizes[8], 5, 8)], None, 16), ([_item(*sizes[8], 5, 8)] + eight, None, 16)]
    a, b, c = planner(cases)
    _check_plan(cases[0][0], a)
    assert b["rc"] == 1 and b["bad"] == 9 and b["text"] == "items[9]: 40 x 22 is distinct size 9 of the call (at most 8)"
    assert c["rc"] == 1 and c["bad"] == 8 and c["text"] == "items[8]: 36 x 20 is distinct size 9 of the call (at most 8)"


def test_a_grid_of_2_to_the_31_workgroups_is_too_large(planner):
    # 32766 x 21844 px is 512 x 1366 = 699392 tiles; 3071 of them make 2^31 + 334080 workgroups, 3070 stay below
    big = _item(32766, 21844, 3, 0, 32768, 32768)
    assert 699392 * 3070 < 2 ** 31 <= 699392 * 3071
    a, b = planner([([big] * 3071, None, 4096), ([big] * 3070, None, 4096)])
    assert a["rc"] == 2 and a["text"] == ""
    _check_plan([big] * 3070, b)
