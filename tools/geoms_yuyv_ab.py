"""A/B of one tick of a server whose cameras have different capture sizes and deliver raw YUYV 4:2:2, in one process on one GPU (the fleets of tools/geoms_ab.py):

  A   what such a server had to do before BSX_STREAM_YUYV_IN: one bsx_yuyv_to_bgr per capture size into a BGR scratch, then ONE bsx_step_batch_geoms of BGR items
      reading that scratch (code this feature does not touch: prep_geoms_k, mask_tile_geoms_k, outside_roi_geoms_k)
  B   ONE bsx_step_batch_geoms whose items carry the bit: the kernels that read a frame convert as they load, no conversion launch, no BGR scratch

Mixes (--mix): M1, M2 and M3 of tools/geoms_ab.py.  --formats all: every stream delivers YUYV; half: every second stream of a class does (leg A converts those, packed
per class; leg B is a call of mixed formats).  Two contexts of the same classes, one per leg, see the same frames every tick, so their temporal states settle on the
same values; composites are compared by digest, masks and temporal state byte for byte.

Derived traffic: leg A's conversion launches move 5 B/px of every YUYV frame (2 read, 3 written) that leg B does not; leg B also reads 1 B/px less in the rows prep
touches and 1 B/px less per composited pixel.  Timing as tools/geoms_ab.py: warm-up; leg A against ITSELF, alternating, for the run-to-run spread; then A and B
alternating; a window repeats its leg until at least --window seconds lie between two device events.  Prints ONE JSON line.

    python tools/geoms_yuyv_ab.py [--mix M1,M2,M3] [--formats all,half] [--rounds 7] [--window 0.05] [--out FILE]
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

FLIP_H, YUYV_IN = 2, 64
FLAG_CYCLE = [0, 0, FLIP_H, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mix", default="M1,M2,M3")
    ap.add_argument("--formats", default="all,half")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.05)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("geoms_yuyv_ab needs a GPU (torch.cuda.is_available() is False): nothing is measured on the CPU")
    import backscrub_amd
    from backscrub_amd import api, synth
    from tools.geoms_ab import MIXES
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import model_path
    L = api.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    results = {}
    ok = True
    for mix in args.mix.split(","):
        key, geoms = MIXES[mix]
        path = model_path(key)
        for formats in args.formats.split(","):
            ctx_a = backscrub_amd.MaskGen.with_geometries(path, geoms)
            ctx_b = backscrub_amd.MaskGen.with_geometries(path, geoms)
            first = [g["first_stream"] for g in ctx_a.geometries()]
            total = sum(n for _, _, n in geoms)
            bgr = [torch.from_numpy(synth.frames(n, w, h, t=0, distinct=4)).cuda() for w, h, n in geoms]
            gallery = [torch.from_numpy(np.stack([synth.background(w, h, seed=21 + k) for k in range(2)])).cuda() for w, h, _n in geoms]
            # per class: the YUYV streams first (local index < ny), packed, as a capture thread would hand them over; the rest stay BGR
            ny = [n if formats == "all" else n // 2 for _w, _h, n in geoms]
            raw, scratch = [], []
            for g, (w, h, n) in enumerate(geoms):
                packed = ctx_a.bgr_to_yuyv(bgr[g][:ny[g]])                                  # Y0 V Y1 U -> a camera's Y0 U Y1 V
                raw.append(packed.view(ny[g], h, w // 2, 4)[..., [0, 3, 2, 1]].contiguous().view(ny[g], h, w, 2))
                scratch.append(torch.zeros((ny[g], h, w, 3), dtype=torch.uint8, device="cuda"))
            out_a = [torch.zeros_like(f) for f in bgr]
            out_b = [torch.zeros_like(f) for f in bgr]
            order = [int(i) for i in np.random.default_rng(11).permutation(total)]
            ids = (C.c_int * total)(*order)
            items_a, items_b = (api._GeomItem * total)(), (api._GeomItem * total)()
            for i, s in enumerate(order):
                g = max(j for j, f0 in enumerate(first) if f0 <= s)
                k = s - first[g]
                yin = k < ny[g]
                fl, bg = FLAG_CYCLE[s % 4], gallery[g][s % 2].data_ptr()
                items_a[i].d_frame, items_a[i].d_out = (scratch[g][k] if yin else bgr[g][k]).data_ptr(), out_a[g][k].data_ptr()
                items_b[i].d_frame, items_b[i].d_out = (raw[g][k] if yin else bgr[g][k]).data_ptr(), out_b[g][k].data_ptr()
                items_a[i].setting.d_bg, items_a[i].setting.flags = bg, fl
                items_b[i].setting.d_bg, items_b[i].setting.flags = bg, fl | (YUYV_IN if yin else 0)
            conv = [(C.c_void_p(raw[g].data_ptr()), C.c_void_p(scratch[g].data_ptr()), w, h, ny[g]) for g, (w, h, _n) in enumerate(geoms) if ny[g]]
            to_bgr, step_geoms = L.bsx_yuyv_to_bgr, L.bsx_step_batch_geoms

            def leg_a():
                for src, dst, w, h, n in conv:
                    if to_bgr(ctx_a.h, src, dst, w, h, n, stream) != 0:
                        raise SystemExit("leg A failed: %s" % (L.bsx_last_error(ctx_a.h) or b"").decode())
                if step_geoms(ctx_a.h, ids, items_a, total, stream, 0) != 0:
                    raise SystemExit("leg A failed: %s" % (L.bsx_last_error(ctx_a.h) or b"").decode())

            def leg_b():
                if step_geoms(ctx_b.h, ids, items_b, total, stream, 0) != 0:
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
            whole = sum(w * h * n for w, h, n in geoms)
            states = bool(torch.equal(ctx_a.ofinal(), ctx_b.ofinal()) and torch.equal(ctx_a._view(3, "uint8", (whole,)), ctx_b._view(3, "uint8", (whole,))))
            med = {k: statistics.median(v) for k, v in ms.items()}
            ypx = sum(w * h * ny[g] for g, (w, h, _n) in enumerate(geoms))
            results["%s/%s" % (mix, formats)] = dict(
                model=key, classes=[list(g) for g in geoms], streams=total, yuyv_streams=sum(ny), conversion_launches_in_a=len(conv),
                conversion_bytes_in_a=5 * ypx, bgr_scratch_bytes_in_a=3 * ypx,
                A=dict(median_ms=round(med["A"], 5), min_ms=round(min(ms["A"]), 5), max_ms=round(max(ms["A"]), 5), ticks_per_window=ks["A"]),
                B=dict(median_ms=round(med["B"], 5), min_ms=round(min(ms["B"]), 5), max_ms=round(max(ms["B"]), 5), ticks_per_window=ks["B"]),
                a_vs_a=dict(median_ms=round(statistics.median(aa), 5), min_ms=round(min(aa), 5), max_ms=round(max(aa), 5), spread_ms=round(spread, 5)),
                b_over_a=round(med["B"] / med["A"], 4), a_minus_b_ms=round(med["A"] - med["B"], 5),
                difference_inside_spread=bool(abs(med["B"] - med["A"]) <= spread),
                digest_a=da, digest_b=db, digests_equal=da == db, masks_and_temporal_states_equal=states)
            ok = ok and da == db and states
            for c in (ctx_a, ctx_b):
                c.close()
            del bgr, raw, scratch, out_a, out_b, gallery
            torch.cuda.empty_cache()
    line = json.dumps(dict(tool="geoms_yuyv_ab", device=torch.cuda.get_device_name(0), rounds=args.rounds, window_s=args.window, mixes=results))
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not ok:
        raise SystemExit("the two legs' outputs differ")


if __name__ == "__main__":
    main()
