"""A/B of the background half of one tick of a gallery / SFU server whose cameras composite over VIDEO backgrounds that a hardware decoder leaves as NV12 surfaces
at the video's native size (app/background.cc:181-190: cv::resize on every grab), in one process on one GPU:

  A   what such a caller does with the older entry points: one bsx_nv12_to_bgr per distinct source size into a native-size BGR scratch — which needs the surfaces of
      a size to lie one behind the other, as they do here — then one bsx_resize_bgr_batch per destination size over the scratch: sources + destinations launches
  B   ONE bsx_resize_surfaces_batch: one launch, every tap converted as it is read, no BGR scratch

Fleets:
  V1  64 cameras each at 640x480, 1280x720 and 1920x1080, every camera with its own 1920x1080 background surface: 192 items
  V2  8 videos of 1280x720, each resized to those three sizes: 24 items on shared sources
  V3  256 x 640x480 from 256 surfaces of 1280x720: one destination size, the case where the ragged grid only costs

The surfaces are pitched (pitch_y = sw + 128, pitch_uv = sw + 64).  Items go in a seeded order that interleaves the destination sizes, the same order in both legs
(leg A's batches keep that order within a size).

Derived traffic (upper bounds, in pixels S of a source and D of a destination, S' = min(S, 4 D) the taps a resize can touch): leg A 4.5 S per distinct surface plus
3 S' + 3 D per item, leg B 1.5 S' + 3 D per item.  Protocol (docs/design/11-blur-batch.md, 11.2): the outputs of the two legs are compared by digest BEFORE anything
is timed; warm-up; leg A against ITSELF, alternating, for the run-to-run spread; then A and B alternating; a window repeats its leg until at least --window seconds
lie between two device events; medians of --rounds windows.  The bar on V1 and V2: B is faster than A by more than A's own spread.  Prints ONE JSON line.

    python tools/resize_surfaces_ab.py [--mix V1,V2,V3] [--rounds 7] [--window 0.2] [--out FILE]
    python tools/resize_surfaces_ab.py --mix V2 --steps-only B --steps 10        # no timing: warm-up, then that many calls of one leg (for a kernel trace)
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
VGA, HD, FHD = (640, 480), (1280, 720), (1920, 1080)
# name -> (source size, number of surfaces, [(destination size, [surface of every item of that size])])
FLEETS = {
    "V1": (FHD, 192, [(VGA, list(range(0, 64))), (HD, list(range(64, 128))), (FHD, list(range(128, 192)))]),
    "V2": (HD, 8, [(VGA, list(range(8))), (HD, list(range(8))), (FHD, list(range(8)))]),
    "V3": (HD, 256, [(VGA, list(range(256)))]),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mix", default="V1,V2,V3")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--steps-only", default=None, choices=["A", "B"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("resize_surfaces_ab needs a GPU (torch.cuda.is_available() is False): nothing is measured on the CPU")
    import backscrub_amd
    from backscrub_amd import api, synth
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import model_path
    L = api.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    results = {}
    ok = True
    for mix in args.mix.split(","):
        (sw, sh), n_surf, dests = FLEETS[mix]
        total = sum(len(who) for _z, who in dests)
        ctx = backscrub_amd.MaskGen(model_path("lite"), 640, 480, n_streams=max(total, n_surf))      # the calls take their own sizes: any context of enough streams
        pitch = (sw + 128, sw + 64)
        four = torch.from_numpy(synth.frames(4, sw, sh, t=0, distinct=4)).cuda()
        y4, uv4 = ctx.bgr_to_nv12(four, *pitch)
        # n_surf surfaces one behind the other (leg A needs that), pitched; the padding holds a pattern
        ybuf = torch.full((n_surf, sh, pitch[0]), 0x5A, dtype=torch.uint8, device="cuda")
        uvbuf = torch.full((n_surf, sh // 2, pitch[1]), 0x5A, dtype=torch.uint8, device="cuda")
        idx = torch.arange(n_surf, device="cuda") % 4
        ybuf[:, :, :sw] = y4[idx]
        uvbuf[:, :, :sw] = uv4[idx]
        del four, y4, uv4
        scratch = torch.zeros((n_surf, sh, sw, 3), dtype=torch.uint8, device="cuda")
        out_a = [torch.zeros((len(who), dh, dw, 3), dtype=torch.uint8, device="cuda") for (dw, dh), who in dests]
        out_b = [torch.zeros((len(who), dh, dw, 3), dtype=torch.uint8, device="cuda") for (dw, dh), who in dests]
        conv = (C.c_void_p(ybuf.data_ptr()), pitch[0], C.c_void_p(uvbuf.data_ptr()), pitch[1], sw, sh, n_surf, C.c_void_p(scratch.data_ptr()))
        order = [(g, j) for g, (_z, who) in enumerate(dests) for j in range(len(who))]
        order = [order[i] for i in np.random.default_rng(11).permutation(total)]
        items_b = (api._ResizeSurfaceItem * total)()
        per_size = [[] for _ in dests]
        for i, (g, j) in enumerate(order):
            (dw, dh), who = dests[g]
            s = who[j]
            b = items_b[i]
            b.d_y, b.d_uv, b.d_dst = ybuf[s].data_ptr(), uvbuf[s].data_ptr(), out_b[g][j].data_ptr()
            b.pitch_y, b.pitch_uv, b.sw, b.sh, b.dw, b.dh, b.flags, b.reserved = pitch[0], pitch[1], sw, sh, dw, dh, 0, 0
            per_size[g].append((scratch[s].data_ptr(), out_a[g][j].data_ptr()))
        items_a = []
        for g, pairs in enumerate(per_size):
            arr = (api._ResizeItem * len(pairs))()
            for a, (src, dst) in zip(arr, pairs):
                a.d_src, a.sw, a.sh, a.d_dst = src, sw, sh, dst
            items_a.append((arr, len(pairs), dests[g][0][0], dests[g][0][1]))
        to_bgr, resize_batch, resize_surfaces = L.bsx_nv12_to_bgr, L.bsx_resize_bgr_batch, L.bsx_resize_surfaces_batch

        def leg_a():
            if to_bgr(ctx.h, *conv, stream) != 0:
                raise SystemExit("leg A failed: %s" % (L.bsx_last_error(ctx.h) or b"").decode())
            for arr, n, dw, dh in items_a:
                if resize_batch(ctx.h, arr, n, dw, dh, stream) != 0:
                    raise SystemExit("leg A failed: %s" % (L.bsx_last_error(ctx.h) or b"").decode())

        def leg_b():
            if resize_surfaces(ctx.h, items_b, total, stream) != 0:
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
        for _ in range(WARMUP):                                       # warm-up: the ring, the tables, code objects
            leg_a()
            leg_b()
        torch.cuda.synchronize()
        launches_a = 1 + len(dests)
        if args.steps_only:
            for _ in range(args.steps):
                (leg_a if args.steps_only == "A" else leg_b)()
            torch.cuda.synchronize()
            results[mix] = dict(leg=args.steps_only, steps=args.steps, warmup_calls_of_each_leg=WARMUP + 1, launches_per_call=launches_a if args.steps_only == "A" else 1)
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
        S = sw * sh
        taps = sum(len(who) * min(S, 4 * dw * dh) for (dw, dh), who in dests)
        D = sum(len(who) * dw * dh for (dw, dh), who in dests)
        bytes_a, bytes_b = 9 * S * n_surf // 2 + 3 * taps + 3 * D, 3 * taps // 2 + 3 * D
        results[mix] = dict(
            source=[sw, sh], surfaces=n_surf, items=total, destinations=[[dw, dh, len(who)] for (dw, dh), who in dests], pitches=list(pitch),
            launches_in_a=launches_a, conversion_launches_in_a=1, launches_in_b=1,
            mb_in_a=round(bytes_a / 1e6, 1), mb_in_b=round(bytes_b / 1e6, 1), bgr_scratch_bytes_in_a=3 * S * n_surf,
            A=dict(median_ms=round(med["A"], 5), min_ms=round(min(ms["A"]), 5), max_ms=round(max(ms["A"]), 5), calls_per_window=ks["A"]),
            B=dict(median_ms=round(med["B"], 5), min_ms=round(min(ms["B"]), 5), max_ms=round(max(ms["B"]), 5), calls_per_window=ks["B"]),
            a_vs_a=dict(median_ms=round(statistics.median(aa), 5), min_ms=round(min(aa), 5), max_ms=round(max(aa), 5), spread_ms=round(spread, 5)),
            b_over_a=round(med["B"] / med["A"], 4), a_minus_b_ms=round(med["A"] - med["B"], 5),
            b_faster_than_a_by_more_than_the_spread=bool(med["A"] - med["B"] > spread),
            digest_a=da, digest_b=db, digests_equal=da == db and da2 == db2 == da)
        ok = ok and da2 == db2 == da
        ctx.close()
        del ybuf, uvbuf, scratch, out_a, out_b
        torch.cuda.empty_cache()
    line = json.dumps(dict(tool="resize_surfaces_ab", device=torch.cuda.get_device_name(0), rounds=args.rounds, window_s=args.window, mixes=results))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not ok:
        raise SystemExit("the two legs' outputs differ")


if __name__ == "__main__":
    main()
