"""A/B of the blur half of one tick of a server in blur mode (`-p bgblur` without `-b`: every camera's background is a blur of its own frame) whose cameras have
different capture sizes and blur sizes and deliver BGR or raw YUYV 4:2:2, in one process on one GPU (the fleets of tools/geoms_ab.py):

  A   what such a server does with the older entry points: one bsx_yuyv_to_bgr per capture size for its YUYV streams into a BGR scratch, then one
      bsx_gaussian_blur_bgr per (capture size, format region, blur size) group of streams that lie next to each other
  B   ONE bsx_gaussian_blur_bgr_batch: one launch, the YUYV frames converted as they are staged, no BGR scratch

Mixes (--mix): M1, M2, M3 and U of tools/geoms_ab.py.  --formats all: every stream delivers YUYV; half: the first half of each class does; none: all BGR.
--ksizes: the blur sizes, dealt to contiguous runs of each class's format regions (25,7: the first half of a region blurs with 25, the second with 7).  The control
is `--mix U --formats none --ksizes 25`: one size, one blur size, all BGR — leg A is ONE launch of gauss_blur_k, and what leg B adds (descriptor reads, the in-kernel
choice of the tap count) is pure cost.

Derived traffic: a YUYV pixel costs leg A 2 + 3 bytes for the conversion and 3 + 3 for the blur, leg B 2 + 3; a BGR pixel 3 + 3 in both.  Timing as
tools/geoms_ab.py: warm-up; leg A against ITSELF, alternating, for the run-to-run spread; then A and B alternating; a window repeats its leg until at least
--window seconds lie between two device events.  Outputs are compared by digest.  Prints ONE JSON line.

    python tools/blur_batch_ab.py [--mix M1,M2,M3] [--formats all,half] [--ksizes 25,7] [--rounds 7] [--window 0.05] [--out FILE]
    python tools/blur_batch_ab.py --mix M1 --formats half --steps-only B --steps 10        # no timing: warm-up, then that many calls of one leg (for a kernel trace)
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

YUYV_IN = 64
WARMUP = 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mix", default="M1,M2,M3")
    ap.add_argument("--formats", default="all,half")
    ap.add_argument("--ksizes", default="25,7")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.05)
    ap.add_argument("--steps-only", default=None, choices=["A", "B"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("blur_batch_ab needs a GPU (torch.cuda.is_available() is False): nothing is measured on the CPU")
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
        for formats in args.formats.split(","):
            ctx = backscrub_amd.MaskGen(model_path("lite"), 640, 480, n_streams=total)       # the blur calls take their own sizes: any context of enough streams
            bgr = [torch.from_numpy(synth.frames(n, w, h, t=0, distinct=4)).cuda() for w, h, n in geoms]
            ny = [{"all": n, "half": n // 2, "none": 0}[formats] for _w, _h, n in geoms]
            raw, scratch = [], []
            for g, (w, h, n) in enumerate(geoms):                         # per class: the YUYV streams first (local index < ny), packed, as a capture thread hands them over
                packed = ctx.bgr_to_yuyv(bgr[g][:max(ny[g], 1)])[:ny[g]]                     # Y0 V Y1 U -> a camera's Y0 U Y1 V
                raw.append(packed.view(ny[g], h, w // 2, 4)[..., [0, 3, 2, 1]].contiguous().view(ny[g], h, w, 2))
                scratch.append(torch.zeros((ny[g], h, w, 3), dtype=torch.uint8, device="cuda"))
            out_a = [torch.zeros_like(f) for f in bgr]
            out_b = [torch.zeros_like(f) for f in bgr]
            conv = [(C.c_void_p(raw[g].data_ptr()), C.c_void_p(scratch[g].data_ptr()), w, h, ny[g]) for g, (w, h, _n) in enumerate(geoms) if ny[g]]
            # leg A's blur launches: per class and format region, contiguous runs of one blur size; leg B's items: stream by stream, the classes interleaved
            blurs, ksize_of = [], {}
            for g, (w, h, n) in enumerate(geoms):
                for lo, hi, src in ((0, ny[g], scratch[g]), (ny[g], n, bgr[g])):
                    cnt = hi - lo                                          # (scratch and bgr are both indexed by the stream's number in its class)
                    for j, k in enumerate(ksizes):
                        a, b = cnt * j // len(ksizes), cnt * (j + 1) // len(ksizes)
                        if b > a:
                            blurs.append((C.c_void_p(src[lo + a].data_ptr()), C.c_void_p(out_a[g][lo + a].data_ptr()), w, h, b - a, k))
                            for s in range(lo + a, lo + b):
                                ksize_of[(g, s)] = k
            order = [(g, s) for g, (_w, _h, n) in enumerate(geoms) for s in range(n)]
            order = [order[i] for i in np.random.default_rng(11).permutation(total)]
            items = (api._BlurItem * total)()
            for i, (g, s) in enumerate(order):
                w, h, _n = geoms[g]
                yin = s < ny[g]
                items[i].d_src, items[i].d_dst = (raw[g][s] if yin else bgr[g][s]).data_ptr(), out_b[g][s].data_ptr()
                items[i].w, items[i].h, items[i].ksize, items[i].flags = w, h, ksize_of[(g, s)], YUYV_IN if yin else 0
            to_bgr, blur, blur_batch = L.bsx_yuyv_to_bgr, L.bsx_gaussian_blur_bgr, L.bsx_gaussian_blur_bgr_batch

            def leg_a():
                for src, dst, w, h, n in conv:
                    if to_bgr(ctx.h, src, dst, w, h, n, stream) != 0:
                        raise SystemExit("leg A failed: %s" % (L.bsx_last_error(ctx.h) or b"").decode())
                for src, dst, w, h, n, k in blurs:
                    if blur(ctx.h, src, dst, w, h, n, k, stream) != 0:
                        raise SystemExit("leg A failed: %s" % (L.bsx_last_error(ctx.h) or b"").decode())

            def leg_b():
                if blur_batch(ctx.h, items, total, stream) != 0:
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

            for _ in range(WARMUP):                                   # warm-up: the ring, the coefficient table, code objects
                leg_a()
                leg_b()
            torch.cuda.synchronize()
            if args.steps_only:
                for _ in range(args.steps):
                    (leg_a if args.steps_only == "A" else leg_b)()
                torch.cuda.synchronize()
                results["%s/%s" % (mix, formats)] = dict(leg=args.steps_only, steps=args.steps, warmup_calls_of_each_leg=WARMUP,
                                                         launches_per_call=len(conv) + len(blurs) if args.steps_only == "A" else 1)
                ctx.close()
                continue
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
            med = {k: statistics.median(v) for k, v in ms.items()}
            ypx = sum(w * h * ny[g] for g, (w, h, _n) in enumerate(geoms))
            bpx = sum(w * h * (n - ny[g]) for g, (w, h, n) in enumerate(geoms))
            results["%s/%s" % (mix, formats)] = dict(
                classes=[list(g) for g in geoms], streams=total, yuyv_streams=sum(ny), ksizes=ksizes,
                launches_in_a=len(conv) + len(blurs), conversion_launches_in_a=len(conv), blur_launches_in_a=len(blurs), launches_in_b=1,
                bytes_in_a=11 * ypx + 6 * bpx, bytes_in_b=5 * ypx + 6 * bpx, bgr_scratch_bytes_in_a=3 * ypx,
                A=dict(median_ms=round(med["A"], 5), min_ms=round(min(ms["A"]), 5), max_ms=round(max(ms["A"]), 5), calls_per_window=ks["A"]),
                B=dict(median_ms=round(med["B"], 5), min_ms=round(min(ms["B"]), 5), max_ms=round(max(ms["B"]), 5), calls_per_window=ks["B"]),
                a_vs_a=dict(median_ms=round(statistics.median(aa), 5), min_ms=round(min(aa), 5), max_ms=round(max(aa), 5), spread_ms=round(spread, 5)),
                b_over_a=round(med["B"] / med["A"], 4), a_minus_b_ms=round(med["A"] - med["B"], 5),
                b_no_slower_than_a_plus_spread=bool(med["B"] <= med["A"] + spread),
                digest_a=da, digest_b=db, digests_equal=da == db)
            ok = ok and da == db
            ctx.close()
            del bgr, raw, scratch, out_a, out_b
            torch.cuda.empty_cache()
    line = json.dumps(dict(tool="blur_batch_ab", device=torch.cuda.get_device_name(0), rounds=args.rounds, window_s=args.window, mixes=results))
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not ok:
        raise SystemExit("the two legs' outputs differ")


if __name__ == "__main__":
    main()
