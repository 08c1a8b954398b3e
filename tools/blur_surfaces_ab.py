"""A/B of the blur half of one tick of a simulcast forwarder in blur mode (`-p bgblur` without `-b`: every camera's background is a blur of its own frame) whose
frames are NV12 decoder surfaces of different capture sizes and blur sizes, in one process on one GPU (the fleets M1, M2, M3 of tools/geoms_ab.py):

  A   what such a caller does with the older entry points: one bsx_nv12_to_bgr per capture size into a BGR scratch — which needs the surfaces of a size to lie one
      behind the other, as they do here — then ONE bsx_gaussian_blur_bgr_batch over the scratch: classes + 1 launches
  B   ONE bsx_gaussian_blur_surfaces_batch: one launch, the surfaces converted as they are staged, no BGR scratch

The surfaces are pitched (pitch_y = w + 128, pitch_uv = w + 64).  --ksizes: the blur sizes, dealt to contiguous runs of each class (25,7: the first half of a class
blurs with 25, the second with 7).  Items go stream by stream in a seeded order that interleaves the classes, the same order in both legs.

Derived traffic: a pixel costs leg A 1.5 + 3 bytes for the conversion and 3 + 3 for the blur, leg B 1.5 + 3.  Protocol (docs/design/11-blur-batch.md, 11.2): the
outputs of the two legs are compared by digest BEFORE anything is timed; warm-up; leg A against ITSELF, alternating, for the run-to-run spread; then A and B
alternating; a window repeats its leg until at least --window seconds lie between two device events; medians of --rounds windows.  The bar: B takes no longer than A
plus A's own spread.  Prints ONE JSON line.

    python tools/blur_surfaces_ab.py [--mix M1,M2,M3] [--ksizes 25,7] [--rounds 7] [--window 0.2] [--out FILE]
    python tools/blur_surfaces_ab.py --mix M1 --steps-only B --steps 10        # no timing: warm-up, then that many calls of one leg (for a kernel trace)
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

WARMUP = 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mix", default="M1,M2,M3")
    ap.add_argument("--ksizes", default="25,7")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--steps-only", default=None, choices=["A", "B"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("blur_surfaces_ab needs a GPU (torch.cuda.is_available() is False): nothing is measured on the CPU")
    import backscrub_amd
    from backscrub_amd import api, synth
    from tools.geoms_ab import MIXES
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import model_path
    L = api.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ksizes = [int(k) for k in args.ksizes.split(",")]
    results = {}
    ok = True
    for mix in args.mix.split(","):
        _key, geoms = MIXES[mix]
        total = sum(n for _, _, n in geoms)
        ctx = backscrub_amd.MaskGen(model_path("lite"), 640, 480, n_streams=total)           # the blur calls take their own sizes: any context of enough streams
        surf, scratch, out_a, out_b, pitch = [], [], [], [], []
        for w, h, n in geoms:                                                                # per class: n surfaces one behind the other (leg A needs that), pitched
            frames = torch.from_numpy(synth.frames(n, w, h, t=0, distinct=4)).cuda()
            pitch.append((w + 128, w + 64))
            surf.append(ctx.bgr_to_nv12(frames, *pitch[-1]))
            scratch.append(torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda"))
            out_a.append(torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda"))
            out_b.append(torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda"))
            del frames
        conv = [(C.c_void_p(surf[g][0].data_ptr()), pitch[g][0], C.c_void_p(surf[g][1].data_ptr()), pitch[g][1], w, h, n, C.c_void_p(scratch[g].data_ptr()))
                for g, (w, h, n) in enumerate(geoms)]
        ksize_of = {}
        for g, (_w, _h, n) in enumerate(geoms):
            for j, k in enumerate(ksizes):
                for s in range(n * j // len(ksizes), n * (j + 1) // len(ksizes)):
                    ksize_of[(g, s)] = k
        order = [(g, s) for g, (_w, _h, n) in enumerate(geoms) for s in range(n)]
        order = [order[i] for i in np.random.default_rng(11).permutation(total)]
        items_a = (api._BlurItem * total)()
        items_b = (api._BlurSurfaceItem * total)()
        for i, (g, s) in enumerate(order):
            w, h, _n = geoms[g]
            a, b = items_a[i], items_b[i]
            a.d_src, a.d_dst, a.w, a.h, a.ksize, a.flags = scratch[g][s].data_ptr(), out_a[g][s].data_ptr(), w, h, ksize_of[(g, s)], 0
            b.d_y, b.d_uv, b.d_dst = surf[g][0][s].data_ptr(), surf[g][1][s].data_ptr(), out_b[g][s].data_ptr()
            b.pitch_y, b.pitch_uv, b.w, b.h, b.ksize, b.flags = pitch[g][0], pitch[g][1], w, h, ksize_of[(g, s)], 0
        to_bgr, blur_batch, blur_surfaces = L.bsx_nv12_to_bgr, L.bsx_gaussian_blur_bgr_batch, L.bsx_gaussian_blur_surfaces_batch

        def leg_a():
            for c in conv:
                if to_bgr(ctx.h, *c, stream) != 0:
                    raise SystemExit("leg A failed: %s" % (L.bsx_last_error(ctx.h) or b"").decode())
            if blur_batch(ctx.h, items_a, total, stream) != 0:
                raise SystemExit("leg A failed: %s" % (L.bsx_last_error(ctx.h) or b"").decode())

        def leg_b():
            if blur_surfaces(ctx.h, items_b, total, stream) != 0:
                raise SystemExit("leg B failed: %s" % (L.bsx_last_error(ctx.h) or b"").decode())

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

        leg_a()                                                       # the outputs first: nothing is timed before the two legs agree
        leg_b()
        torch.cuda.synchronize()
        da, db = digest(out_a), digest(out_b)
        if da != db:
            raise SystemExit("%s: the two legs' outputs differ (%s, %s)" % (mix, da, db))
        for _ in range(WARMUP):                                       # warm-up: the ring, the coefficient table, code objects
            leg_a()
            leg_b()
        torch.cuda.synchronize()
        if args.steps_only:
            for _ in range(args.steps):
                (leg_a if args.steps_only == "A" else leg_b)()
            torch.cuda.synchronize()
            results[mix] = dict(leg=args.steps_only, steps=args.steps, warmup_calls_of_each_leg=WARMUP + 1, launches_per_call=len(conv) + 1 if args.steps_only == "A" else 1)
            ctx.close()
            continue
        ks = {name: max(3, int(args.window / (timed(fn, 3) / 1e3)) + 1) for name, fn in (("A", leg_a), ("B", leg_b))}
        aa = []
        for _ in range(args.rounds):                                  # A against itself: the spread
            aa.append(timed(leg_a, ks["A"]))
            aa.append(timed(leg_a, ks["A"]))
        spread = max(aa) - min(aa)
        ms = {"A": [], "B": []}
        for _ in range(args.rounds):
            ms["A"].append(timed(leg_a, ks["A"]))
            ms["B"].append(timed(leg_b, ks["B"]))
        torch.cuda.synchronize()
        da2, db2 = digest(out_a), digest(out_b)
        med = {k: statistics.median(v) for k, v in ms.items()}
        px = sum(w * h * n for w, h, n in geoms)
        results[mix] = dict(
            classes=[list(g) for g in geoms], streams=total, ksizes=ksizes, pitches=[list(p) for p in pitch],
            launches_in_a=len(conv) + 1, conversion_launches_in_a=len(conv), launches_in_b=1,
            bytes_in_a=21 * px // 2, bytes_in_b=9 * px // 2, bgr_scratch_bytes_in_a=3 * px,
            A=dict(median_ms=round(med["A"], 5), min_ms=round(min(ms["A"]), 5), max_ms=round(max(ms["A"]), 5), calls_per_window=ks["A"]),
            B=dict(median_ms=round(med["B"], 5), min_ms=round(min(ms["B"]), 5), max_ms=round(max(ms["B"]), 5), calls_per_window=ks["B"]),
            a_vs_a=dict(median_ms=round(statistics.median(aa), 5), min_ms=round(min(aa), 5), max_ms=round(max(aa), 5), spread_ms=round(spread, 5)),
            b_over_a=round(med["B"] / med["A"], 4), a_minus_b_ms=round(med["A"] - med["B"], 5),
            b_no_slower_than_a_plus_spread=bool(med["B"] <= med["A"] + spread),
            digest_a=da, digest_b=db, digests_equal=da == db and da2 == db2 == da)
        ok = ok and da2 == db2 == da
        ctx.close()
        del surf, scratch, out_a, out_b
        torch.cuda.empty_cache()
    line = json.dumps(dict(tool="blur_surfaces_ab", device=torch.cuda.get_device_name(0), rounds=args.rounds, window_s=args.window, mixes=results))
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not ok:
        raise SystemExit("the two legs' outputs differ")


if __name__ == "__main__":
    main()
