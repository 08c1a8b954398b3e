"""A/B of one tick of a server with 64 x 640x480, 64 x 1280x720 and 64 x 1920x1080 segm_lite cameras, in one process on one GPU.  segm_lite's ROI at 1920x1080 is
(60, 0, 1799, 1080): off the 4-pixel grid, so bsx_new_geoms refuses that size and bsx_new_geoms_ex(BSX_GEOMS_EDGE_ROI) takes it.

  A   what a server has without the flag: a two-class context (640x480 + 1280x720) stepped with ONE bsx_step_batch_geoms call, plus a one-geometry 1920x1080
      context stepped with bsx_step_batch_streams (the unfused step: that geometry is off the fused tile route), on the same HIP stream one after the other
  B   ONE edge context of the three classes, ONE bsx_step_batch_geoms call

and, on the edge context alone, a call of the 64 1920x1080 streams only (the edge launcher's kernels) next to a call of the 64 1280x720 streams only (the
word-route launcher's): ms per frame of each whole call.  The tile launches themselves are read from a kernel trace of --steps-only E (1080p only) and
--steps-only W (720p only).

The protocol is tools/geoms_ab.py's: raw C ABI with prepared arguments; warm-up; leg A against itself, alternating, for the run-to-run spread; then A and B
alternating; a window repeats its leg until at least --window seconds have passed between two device events.  Both legs see the same frames every tick, and the
outputs are compared by digest.  Prints ONE JSON line.

    python tools/geoms_edge_ab.py [--rounds 7] [--window 0.05] [--per-class 64] [--out FILE]
    python tools/geoms_edge_ab.py --steps-only E --steps 10          # no timing: warm-up, then that many ticks of one leg (A, B, E or W)
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = [(640, 480), (1280, 720), (1920, 1080)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.05)
    ap.add_argument("--per-class", type=int, default=64)
    ap.add_argument("--steps-only", default=None, choices=["A", "B", "E", "W"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("geoms_edge_ab needs a GPU (torch.cuda.is_available() is False): nothing is measured on the CPU")
    import backscrub_amd
    from backscrub_amd import api, synth
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import model_path
    L = api.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = args.per_class
    path = model_path("lite")
    geoms = [(w, h, n) for w, h in SIZES]
    edge = backscrub_amd.MaskGen.with_geometries(path, geoms, edge_roi=True)
    assert edge.geometries()[2]["roi"] == [60, 0, 1799, 1080], edge.geometries()[2]["roi"]
    two = backscrub_amd.MaskGen.with_geometries(path, geoms[:2])
    fhd = backscrub_amd.MaskGen(path, 1920, 1080, n_streams=n)
    frames = [torch.from_numpy(synth.frames(n, w, h, t=0, distinct=4)).cuda() for w, h, _n in geoms]
    bgs = [torch.from_numpy(synth.background(w, h, seed=21 + g)).cuda() for g, (w, h, _n) in enumerate(geoms)]      # one background per class
    out_a = [torch.zeros_like(f) for f in frames]
    out_b = [torch.zeros_like(f) for f in frames]

    def geom_items(classes, outs, seed):
        """ids and items of one geoms call for every stream of the context's first len(classes) classes (`classes` = 0, 1, ..: stream g * n + k), interleaved"""
        order = [int(i) for i in np.random.default_rng(seed).permutation(n * len(classes))]
        ids = (C.c_int * len(order))(*order)
        items = (api._GeomItem * len(order))()
        for i, s in enumerate(order):
            g, k = classes[s // n], s % n
            items[i].d_frame, items[i].d_out = frames[g][k].data_ptr(), outs[g][k].data_ptr()
            items[i].setting.d_bg, items[i].setting.flags = bgs[g].data_ptr(), 0
        return ids, items, len(order)

    ids_two, items_two, n_two = geom_items([0, 1], out_a, 11)
    ids_all, items_all, n_all = geom_items([0, 1, 2], out_b, 11)
    ids_fhd = (C.c_int * n)(*range(n))
    # one class of the edge context alone: the streams of class g are ids [g * n, (g + 1) * n)
    scratch = [None, torch.zeros_like(frames[1]), torch.zeros_like(frames[2])]
    only = {}
    for name, g in (("W", 1), ("E", 2)):
        ids = (C.c_int * n)(*range(g * n, (g + 1) * n))
        items = (api._GeomItem * n)()
        for k in range(n):
            items[k].d_frame, items[k].d_out = frames[g][k].data_ptr(), scratch[g][k].data_ptr()
            items[k].setting.d_bg, items[k].setting.flags = bgs[g].data_ptr(), 0
        only[name] = (ids, items)
    step_geoms, step_streams = L.bsx_step_batch_geoms, L.bsx_step_batch_streams

    def need(rc, h, what):
        if rc != 0:
            raise SystemExit("%s failed: %s" % (what, (L.bsx_last_error(h) or b"").decode()))

    def leg_a():
        need(step_geoms(two.h, ids_two, items_two, n_two, stream, 0), two.h, "leg A (geoms)")
        need(step_streams(fhd.h, ids_fhd, C.c_void_p(frames[2].data_ptr()), C.c_void_p(bgs[2].data_ptr()), 0, C.c_void_p(out_a[2].data_ptr()), n, stream, 0), fhd.h,
             "leg A (1920x1080)")

    def leg_b():
        need(step_geoms(edge.h, ids_all, items_all, n_all, stream, 0), edge.h, "leg B")

    def leg_only(name):
        def run():
            need(step_geoms(edge.h, only[name][0], only[name][1], n, stream, 0), edge.h, "leg " + name)
        return run
    legs = {"A": leg_a, "B": leg_b, "E": leg_only("E"), "W": leg_only("W")}

    def timed(fn, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(k):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / k

    def digest(outs):
        hsh = hashlib.sha256()
        for o in outs:
            hsh.update(o.cpu().numpy().tobytes())
        return hsh.hexdigest()[:16]

    for _ in range(6):                                                # warm-up: tables, rings, code objects; the temporal states settle (the frames do not change)
        leg_a()
        leg_b()
    torch.cuda.synchronize()
    if args.steps_only:
        for _ in range(3):
            legs[args.steps_only]()
        for _ in range(args.steps):
            legs[args.steps_only]()
        torch.cuda.synchronize()
        result = dict(leg=args.steps_only, ticks=args.steps)
        ok = True
    else:
        da, db = digest(out_a), digest(out_b)                         # (before the one-class legs advance the edge context alone)
        states = torch.equal(edge.ofinal()[:2 * n], two.ofinal()) and torch.equal(edge.ofinal()[2 * n:], fhd.ofinal())
        ks = {name: max(3, int(args.window / (timed(fn, 3) / 1e3)) + 1) for name, fn in legs.items()}
        aa = []
        for _ in range(args.rounds):                                  # A against itself: the spread
            aa.append(timed(leg_a, ks["A"]))
            aa.append(timed(leg_a, ks["A"]))
        spread = max(aa) - min(aa)
        ms = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k in ("A", "B", "E", "W"):
                ms[k].append(timed(legs[k], ks[k]))
        torch.cuda.synchronize()
        med = {k: statistics.median(v) for k, v in ms.items()}

        def leg(k, **more):
            return dict(median_ms=round(med[k], 5), min_ms=round(min(ms[k]), 5), max_ms=round(max(ms[k]), 5), ticks_per_window=ks[k], **more)
        result = dict(
            model="lite", classes=[list(g) for g in geoms], streams=3 * n,
            A=leg("A", contexts=2, calls=2), B=leg("B", contexts=1, calls=1),
            a_vs_a=dict(median_ms=round(statistics.median(aa), 5), min_ms=round(min(aa), 5), max_ms=round(max(aa), 5), spread_ms=round(spread, 5)),
            b_over_a=round(med["B"] / med["A"], 4), a_minus_b_ms=round(med["A"] - med["B"], 5), b_faster_than_a_by_more_than_the_spread=bool(med["A"] - med["B"] > spread),
            difference_inside_spread=bool(abs(med["B"] - med["A"]) <= spread),
            edge_class_only=leg("E", size=[1920, 1080], ms_per_frame=round(med["E"] / n, 6), us_per_megapixel=round(1e3 * med["E"] / (n * 1920 * 1080 / 1e6), 4)),
            word_class_only=leg("W", size=[1280, 720], ms_per_frame=round(med["W"] / n, 6), us_per_megapixel=round(1e3 * med["W"] / (n * 1280 * 720 / 1e6), 4)),
            digest_a=da, digest_b=db, digests_equal=da == db, temporal_states_equal=bool(states))
        ok = da == db and bool(states)
    for c in (edge, two, fhd):
        c.close()
    line = json.dumps(dict(tool="geoms_edge_ab", device=torch.cuda.get_device_name(0), rounds=args.rounds, window_s=args.window, result=result))
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not ok:
        raise SystemExit("the two legs' outputs differ")


if __name__ == "__main__":
    main()
