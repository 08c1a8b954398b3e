"""A/B of one tick of a server whose cameras have different capture sizes and whose participants all leave at ONE size, in one process on one GPU, same build,
same fleet:

  A   bsx_step_batch_geoms into capture-size BGR scratch images, then per class one bsx_resize_bgr to the output size [and one bsx_bgr_to_yuyv] — what such a
      server had to do before bsx_step_batch_vcam_geoms
  B   ONE bsx_step_batch_vcam_geoms call: the same front, one masks-only tile launch, one resize pass; no capture-size composite is stored

Fleets (--mix):
  M1  segm_lite, 256 streams = 128 x 640x480 + 64 x 1280x720 + 64 x 640x360  ->  640x360  (identity for one class, exact 2x for another)
  M2  MLKit,     256 streams =  96 x 640x480 + 96 x 1280x720 + 64 x 1920x1080 -> 854x480
  M3  segm_lite, 8 sizes x 4 streams -> 426x240: few cameras of many sizes

Each leg has a context of its own (both made the same way), so neither advances the other's temporal state.  Both go through the raw C ABI with their arguments
prepared.  Per fleet and output format: warm-up (every table exists, the rings are allocated); then leg A against ITSELF, alternating, which gives the run-to-run
spread of this machine in this run (max - min of its windows' ms per tick); then A and B alternating.  A window repeats its leg until at least --window seconds
have passed between two device events; ms per tick = window / repetitions.  Both legs see the same frames every tick, so their temporal states settle on the same
values and the outputs are compared by digest.  Prints ONE JSON line.  No bar is set: the figures are recorded, whichever way they fall.

    python tools/vcam_geoms_ab.py [--mix M1,M2,M3] [--formats bgr,yuyv] [--rounds 7] [--window 0.05] [--out FILE]
    python tools/vcam_geoms_ab.py --mix M1 --steps-only B --steps 10        # no timing: warm-up, then that many ticks of one leg (for a kernel trace)
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
    "M1": ("lite", [(640, 480, 128), (1280, 720, 64), (640, 360, 64)], (640, 360)),
    "M2": ("mlkit", [(640, 480, 96), (1280, 720, 96), (1920, 1080, 64)], (854, 480)),
    "M3": ("lite", [(w, h, 4) for w, h in ((320, 240), (640, 360), (640, 480), (800, 600), (960, 720), (1024, 768), (1280, 720), (1280, 960))], (426, 240)),
}
FLIP_H = 2
FLAG_CYCLE = [0, 0, FLIP_H, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mix", default="M1,M2,M3")
    ap.add_argument("--formats", default="bgr,yuyv")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.05)
    ap.add_argument("--steps-only", default=None, choices=["A", "B"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("vcam_geoms_ab needs a GPU (torch.cuda.is_available() is False): nothing is measured on the CPU")
    import backscrub_amd
    from backscrub_amd import api, synth
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import model_path
    L = api.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    results = {}
    ok = True
    for mix in args.mix.split(","):
        key, geoms, (ow, oh) = MIXES[mix]
        path = model_path(key)
        total = sum(n for _, _, n in geoms)
        frames = [torch.from_numpy(synth.frames(n, w, h, t=0, distinct=4)).cuda() for w, h, n in geoms]
        gallery = [torch.from_numpy(np.stack([synth.background(w, h, seed=21 + k) for k in range(2)])).cuda() for w, h, _n in geoms]
        order = [int(i) for i in np.random.default_rng(11).permutation(total)]
        for fmt in args.formats.split(","):
            yuyv = fmt == "yuyv"
            ctx_a, ctx_b = (backscrub_amd.MaskGen.with_geometries(path, geoms) for _ in range(2))
            first = [g["first_stream"] for g in ctx_a.geometries()]
            comp = [torch.zeros_like(f) for f in frames]                                       # leg A's capture-size scratch
            bgr = [torch.zeros((n, oh, ow, 3), dtype=torch.uint8, device="cuda") for _w, _h, n in geoms]
            out_a = [torch.zeros((n, oh, ow, 2), dtype=torch.uint8, device="cuda") for _w, _h, n in geoms] if yuyv else bgr
            out_b = [torch.zeros_like(o) for o in out_a]
            ids = (C.c_int * total)(*order)
            items_a, items_b = (api._GeomItem * total)(), (api._GeomItem * total)()
            for i, s in enumerate(order):
                g = max(j for j, f0 in enumerate(first) if f0 <= s)
                k = s - first[g]
                for items, dst in ((items_a, comp), (items_b, out_b)):
                    items[i].d_frame, items[i].d_out = frames[g][k].data_ptr(), dst[g][k].data_ptr()
                    items[i].setting.d_bg, items[i].setting.flags = gallery[g][s % 2].data_ptr(), FLAG_CYCLE[s % 4]
            P = lambda t: C.c_void_p(t.data_ptr())                    # noqa: E731
            rsz = [(P(comp[g]), w, h, P(bgr[g]), n) for g, (w, h, n) in enumerate(geoms)]
            pack = [(P(bgr[g]), P(out_a[g]), n) for g, (_w, _h, n) in enumerate(geoms)] if yuyv else []
            step_geoms, resize, to_yuyv, step_vcam = L.bsx_step_batch_geoms, L.bsx_resize_bgr, L.bsx_bgr_to_yuyv, L.bsx_step_batch_vcam_geoms

            def leg_a():
                rc = step_geoms(ctx_a.h, ids, items_a, total, stream, 0)
                for src, w, h, dst, n in rsz:
                    rc = rc or resize(ctx_a.h, src, w, h, dst, ow, oh, n, stream)
                for src, dst, n in pack:
                    rc = rc or to_yuyv(ctx_a.h, src, dst, ow, oh, n, stream)
                if rc != 0:
                    raise SystemExit("leg A failed: %s" % (L.bsx_last_error(ctx_a.h) or b"").decode())

            def leg_b():
                if step_vcam(ctx_b.h, ids, items_b, total, ow, oh, stream, 1 if yuyv else 0) != 0:
                    raise SystemExit("leg B failed: %s" % (L.bsx_last_error(ctx_b.h) or b"").decode())

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

            for _ in range(6):                                        # warm-up: tables, rings, code objects; the temporal states settle (the frames do not change)
                leg_a()
                leg_b()
            torch.cuda.synchronize()
            name = "%s/%s" % (mix, fmt)
            if args.steps_only:
                fn = leg_a if args.steps_only == "A" else leg_b
                for _ in range(args.steps):
                    fn()
                torch.cuda.synchronize()
                results[name] = dict(leg=args.steps_only, ticks=args.steps, warm_up_ticks_of_each_leg=6)
            else:
                ks = {leg: max(3, int(args.window / (timed(fn, 3) / 1e3)) + 1) for leg, fn in (("A", leg_a), ("B", leg_b))}
                aa = []
                for _ in range(args.rounds):                          # A against itself: the spread
                    aa.append(timed(leg_a, ks["A"]))
                    aa.append(timed(leg_a, ks["A"]))
                spread = max(aa) - min(aa)
                ms = {"A": [], "B": []}
                for _ in range(args.rounds):
                    ms["A"].append(timed(leg_a, ks["A"]))
                    ms["B"].append(timed(leg_b, ks["B"]))
                torch.cuda.synchronize()
                da, db = digest(out_a), digest(out_b)
                states = bool(torch.equal(ctx_a.ofinal(), ctx_b.ofinal()))
                med = {k: statistics.median(v) for k, v in ms.items()}
                results[name] = dict(
                    model=key, classes=[list(g) for g in geoms], streams=total, out=[ow, oh], format=fmt,
                    A=dict(median_ms=round(med["A"], 5), min_ms=round(min(ms["A"]), 5), max_ms=round(max(ms["A"]), 5), ticks_per_window=ks["A"],
                           calls_per_tick=1 + len(rsz) + len(pack)),
                    B=dict(median_ms=round(med["B"], 5), min_ms=round(min(ms["B"]), 5), max_ms=round(max(ms["B"]), 5), ticks_per_window=ks["B"], calls_per_tick=1),
                    a_vs_a=dict(median_ms=round(statistics.median(aa), 5), min_ms=round(min(aa), 5), max_ms=round(max(aa), 5), spread_ms=round(spread, 5)),
                    b_over_a=round(med["B"] / med["A"], 4), a_minus_b_ms=round(med["A"] - med["B"], 5),
                    difference_inside_spread=bool(abs(med["B"] - med["A"]) <= spread),
                    digest_a=da, digest_b=db, digests_equal=da == db, temporal_states_equal=states)
                ok = ok and da == db and states
            for c in (ctx_a, ctx_b):
                c.close()
            del comp, bgr, out_a, out_b
            torch.cuda.empty_cache()
        del frames, gallery
        torch.cuda.empty_cache()
    line = json.dumps(dict(tool="vcam_geoms_ab", device=torch.cuda.get_device_name(0), rounds=args.rounds, window_s=args.window, fleets=results))
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not ok:
        raise SystemExit("the two legs' outputs differ")


if __name__ == "__main__":
    main()
