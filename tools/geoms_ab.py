"""A/B of one tick of a server whose cameras have different capture sizes, in one process on one GPU:

  A   one context per size, each stepped with bsx_step_batch_mixed on the same HIP stream one after the other (what such a server had to do before
      bsx_new_geoms; code the multi-geometry step does not touch)
  B   ONE context of several geometry classes, ONE bsx_step_batch_geoms call: one prep launch, one pass of the network, one tile launch

Mixes (--mix):
  M1  segm_lite, 256 streams = 128 x 640x480 + 64 x 1280x720 + 64 x 640x360
  M2  MLKit,     256 streams =  96 x 640x480 + 96 x 1280x720 + 64 x 1920x1080
  M3  segm_lite, 8 sizes x 4 streams: few cameras of many sizes
  U   segm_lite, ONE size, 256 x 640x480: leg A is bsx_step_batch_mixed on the same data (the cost of reading the geometry per position)

Both legs go through the raw C ABI with their arguments prepared.  Per mix: warm-up (every table exists, the rings are allocated); then leg A against ITSELF,
alternating, which gives the run-to-run spread of this machine in this run (max - min of its windows' ms per tick); then A and B alternating.  A window repeats
its leg until at least --window seconds have passed between two device events; ms per tick = window / repetitions.  Both legs see the same frames every tick,
so their temporal states settle on the same values and the outputs are compared by digest.  Prints ONE JSON line.

    python tools/geoms_ab.py [--mix M1,M2,M3,U] [--rounds 7] [--window 0.05] [--out FILE]
    python tools/geoms_ab.py --mix M1 --steps-only B --steps 10        # no timing: warm-up, then that many ticks of one leg (for a kernel trace)
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

MIXES = {
    "M1": ("lite", [(640, 480, 128), (1280, 720, 64), (640, 360, 64)]),
    "M2": ("mlkit", [(640, 480, 96), (1280, 720, 96), (1920, 1080, 64)]),
    "M3": ("lite", [(w, h, 4) for w, h in ((320, 240), (640, 360), (640, 480), (800, 600), (960, 720), (1024, 768), (1280, 720), (1280, 960))]),
    "U": ("lite", [(640, 480, 256)]),
}
FLIP_H = 2
FLAG_CYCLE = [0, 0, FLIP_H, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mix", default="M1,M2,M3,U")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.05)
    ap.add_argument("--steps-only", default=None, choices=["A", "B"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("geoms_ab needs a GPU (torch.cuda.is_available() is False): nothing is measured on the CPU")
    import backscrub_amd
    from backscrub_amd import api, synth
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import model_path
    L = api.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    results = {}
    ok = True
    for mix in args.mix.split(","):
        key, geoms = MIXES[mix]
        path = model_path(key)
        multi = backscrub_amd.MaskGen.with_geometries(path, geoms)
        singles = [backscrub_amd.MaskGen(path, w, h, n_streams=n) for w, h, n in geoms]
        first = [g["first_stream"] for g in multi.geometries()]
        total = sum(n for _, _, n in geoms)
        frames = [torch.from_numpy(synth.frames(n, w, h, t=0, distinct=4)).cuda() for w, h, n in geoms]
        gallery = [torch.from_numpy(np.stack([synth.background(w, h, seed=21 + k) for k in range(2)])).cuda() for w, h, _n in geoms]
        out_a = [torch.zeros_like(f) for f in frames]
        out_b = [torch.zeros_like(f) for f in frames]
        # leg A: per class the packed arrays of the mixed step; leg B: one item per stream, the ids interleaving the classes
        sett = []
        for g, (w, h, n) in enumerate(geoms):
            st = (api._StreamSetting * n)()
            for k in range(n):
                st[k].d_bg, st[k].flags = gallery[g][(first[g] + k) % 2].data_ptr(), FLAG_CYCLE[(first[g] + k) % 4]
            sett.append(st)
        order = [int(i) for i in np.random.default_rng(11).permutation(total)]
        ids = (C.c_int * total)(*order)
        items = (api._GeomItem * total)()
        for i, s in enumerate(order):
            g = max(j for j, f0 in enumerate(first) if f0 <= s)
            k = s - first[g]
            items[i].d_frame, items[i].d_out = frames[g][k].data_ptr(), out_b[g][k].data_ptr()
            items[i].setting.d_bg, items[i].setting.flags = sett[g][k].d_bg, sett[g][k].flags
        a_args = [(singles[g].h, None, C.c_void_p(frames[g].data_ptr()), sett[g], C.c_void_p(out_a[g].data_ptr()), n) for g, (_w, _h, n) in enumerate(geoms)]
        mixed, step_geoms = L.bsx_step_batch_mixed, L.bsx_step_batch_geoms

        def leg_a():
            for h_, i_, f_, s_, o_, n_ in a_args:
                if mixed(h_, i_, f_, s_, o_, n_, stream, 0) != 0:
                    raise SystemExit("leg A failed: %s" % (L.bsx_last_error(h_) or b"").decode())

        def leg_b():
            if step_geoms(multi.h, ids, items, total, stream, 0) != 0:
                raise SystemExit("leg B failed: %s" % (L.bsx_last_error(multi.h) or b"").decode())

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

        for _ in range(6):                                            # warm-up: tables, rings, code objects; the temporal states settle (the frames do not change)
            leg_a()
            leg_b()
        torch.cuda.synchronize()
        if args.steps_only:
            fn = leg_a if args.steps_only == "A" else leg_b
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            results[mix] = dict(leg=args.steps_only, ticks=args.steps, warm_up_ticks_of_each_leg=6)
        else:
            ks = {name: max(3, int(args.window / (timed(fn, 3) / 1e3)) + 1) for name, fn in (("A", leg_a), ("B", leg_b))}
            aa = []
            for _ in range(args.rounds):                              # A against itself: the spread
                aa.append(timed(leg_a, ks["A"]))
                aa.append(timed(leg_a, ks["A"]))
            spread = max(aa) - min(aa)
            ms = {"A": [], "B": []}
            for _ in range(args.rounds):
                ms["A"].append(timed(leg_a, ks["A"]))
                ms["B"].append(timed(leg_b, ks["B"]))
            torch.cuda.synchronize()
            da, db = digest(out_a), digest(out_b)
            states = all(torch.equal(multi.ofinal()[first[g]:first[g] + n], singles[g].ofinal()) for g, (_w, _h, n) in enumerate(geoms))
            med = {k: statistics.median(v) for k, v in ms.items()}
            results[mix] = dict(
                model=key, classes=[list(g) for g in geoms], streams=total,
                A=dict(median_ms=round(med["A"], 5), min_ms=round(min(ms["A"]), 5), max_ms=round(max(ms["A"]), 5), ticks_per_window=ks["A"], contexts=len(geoms)),
                B=dict(median_ms=round(med["B"], 5), min_ms=round(min(ms["B"]), 5), max_ms=round(max(ms["B"]), 5), ticks_per_window=ks["B"], contexts=1),
                a_vs_a=dict(median_ms=round(statistics.median(aa), 5), min_ms=round(min(aa), 5), max_ms=round(max(aa), 5), spread_ms=round(spread, 5)),
                b_over_a=round(med["B"] / med["A"], 4), a_minus_b_ms=round(med["A"] - med["B"], 5),
                b_not_slower_than_a_plus_spread=bool(med["B"] <= med["A"] + spread), b_within_10_percent_of_a=bool(med["B"] <= 1.10 * med["A"]),
                difference_inside_spread=bool(abs(med["B"] - med["A"]) <= spread),
                digest_a=da, digest_b=db, digests_equal=da == db, temporal_states_equal=bool(states))
            ok = ok and da == db and states
        for c in [multi] + singles:
            c.close()
        del frames, out_a, out_b, gallery
        torch.cuda.empty_cache()
    line = json.dumps(dict(tool="geoms_ab", device=torch.cuda.get_device_name(0), rounds=args.rounds, window_s=args.window, mixes=results))
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not ok:
        raise SystemExit("the two legs' outputs differ")


if __name__ == "__main__":
    main()
