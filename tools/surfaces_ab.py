"""A/B of one tick of a simulcast forwarder that receives ENCODED video — what it holds after the hardware decoder is an NV12 surface per camera — and feeds
video encoders, in one process on one GPU, same build, same fleet and layer sets as tools/vcam_nv12_ab.py:

  A   one bsx_nv12_to_bgr per class (the surfaces of a class lie one behind the other), then bsx_step_batch_vcam_geoms_outs_nv12 on the BGR frames: 1 + classes
      calls, every frame written as 3 B/px and read back by prep and by the resize pass
  B   ONE bsx_step_batch_surfaces call: prep and the resize pass read 1.5 B/px straight from the decoder's surfaces

Fleet: segm_lite, 64 x 640x480 + 64 x 1280x720 + 64 x 640x360, every stream at 640x360 + 320x180 + 160x90 (--layers and --per-class change it); a plane's pitch, in
and out, is its width rounded up to --pitch-align bytes.

Each leg has a context of its own (both made the same way), so neither advances the other's temporal state.  Both go through the raw C ABI with their arguments
prepared.  Warm-up (every table exists, the rings are allocated); then leg A against ITSELF, alternating, which gives the run-to-run spread of this machine in this
run (max - min of its windows' ms per tick); then A and B alternating.  A window repeats its leg until at least --window seconds have passed between two device
events; ms per tick = window / repetitions.  Both legs see the same surfaces every tick, so their temporal states settle on the same values and the planes are
compared by digest.  Prints ONE JSON line.  No bar is set: the figures are recorded, whichever way they fall (docs/design/05e-host-side.md has them).

    python tools/surfaces_ab.py [--layers 640x360,320x180,160x90] [--per-class 64] [--pitch-align 256] [--rounds 7] [--window 0.3] [--out FILE]
    python tools/surfaces_ab.py --steps-only B --steps 10        # no timing: warm-up, then that many ticks of one leg (for a kernel trace)
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

SIZES = [(640, 480), (1280, 720), (640, 360)]
FLIP_H = 2
FLAG_CYCLE = [0, 0, FLIP_H, 0]
WARM_UP = 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", default="640x360,320x180,160x90")
    ap.add_argument("--per-class", type=int, default=64)
    ap.add_argument("--pitch-align", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--steps-only", default=None, choices=["A", "B"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    layers = [tuple(int(v) for v in l.split("x")) for l in args.layers.split(",")]
    if not 1 <= len(layers) <= 4 or len(set(layers)) != len(layers) or any((w | h) & 1 for w, h in layers):
        raise SystemExit("--layers: one to four distinct WxH, both even")
    if args.pitch_align < 4 or args.pitch_align % 4:
        raise SystemExit("--pitch-align: a multiple of 4")
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("surfaces_ab needs a GPU (torch.cuda.is_available() is False): nothing is measured on the CPU")
    import backscrub_amd
    from backscrub_amd import api, synth
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import model_path
    L = api.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    geoms = [(w, h, args.per_class) for w, h in SIZES]
    total = sum(n for _, _, n in geoms)
    path = model_path("lite")

    def up(v):
        return (v + args.pitch_align - 1) // args.pitch_align * args.pitch_align
    ctx_a, ctx_b = (backscrub_amd.MaskGen.with_geometries(path, geoms) for _ in range(2))
    # the decoder's surfaces: per class one Y and one UV allocation, stream k of the class at index k of each
    in_pitch = [up(w) for w, _h, _n in geoms]
    surf = [ctx_a.bgr_to_nv12(torch.from_numpy(synth.frames(n, w, h, t=0, distinct=4)).cuda(), p, p) for (w, h, n), p in zip(geoms, in_pitch)]
    surf = [(y.as_strided((n, h, p), (h * p, p, 1)), uv.as_strided((n, h // 2, p), (h // 2 * p, p, 1))) for (y, uv), (_w, h, n), p in zip(surf, geoms, in_pitch)]
    bgr_in = [torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda") for w, h, n in geoms]                  # leg A's converted frames
    gallery = [torch.from_numpy(np.stack([synth.background(w, h, seed=21 + k) for k in range(2)])).cuda() for w, h, _n in geoms]
    order = [int(i) for i in np.random.default_rng(11).permutation(total)]
    first = [g["first_stream"] for g in ctx_a.geometries()]
    pitch = [up(ow) for ow, _oh in layers]

    def planes():
        """per layer (Y [total, oh, pitch], UV [total, oh / 2, pitch]): stream s's surface at index s of each"""
        return [(torch.zeros((total, oh, p), dtype=torch.uint8, device="cuda"), torch.zeros((total, oh // 2, p), dtype=torch.uint8, device="cuda"))
                for (_ow, oh), p in zip(layers, pitch)]
    out_a, out_b = planes(), planes()
    ids = (C.c_int * total)(*order)
    items_a, items_b = (api._GeomItem * total)(), (api._SurfaceItem * total)()
    m = total * len(layers)
    recs_a, recs_b = (api._VcamOutNv12 * m)(), (api._VcamOutNv12 * m)()
    for i, s in enumerate(order):
        g = max(j for j, f0 in enumerate(first) if f0 <= s)
        k = s - first[g]
        items_a[i].d_frame, items_a[i].d_out = bgr_in[g][k].data_ptr(), None
        b = items_b[i]
        b.d_y, b.d_uv, b.pitch_y, b.pitch_uv = surf[g][0][k].data_ptr(), surf[g][1][k].data_ptr(), in_pitch[g], in_pitch[g]
        for it in (items_a[i], b):
            it.setting.d_bg, it.setting.flags = gallery[g][s % 2].data_ptr(), FLAG_CYCLE[s % 4]
        for q, (ow, oh) in enumerate(layers):                      # the records as a forwarder has them: per camera, its layers
            for recs, outs in ((recs_a, out_a), (recs_b, out_b)):
                r = recs[i * len(layers) + q]
                r.item, r.out_w, r.out_h, r.pitch_y, r.pitch_uv, r.d_y, r.d_uv = i, ow, oh, pitch[q], pitch[q], outs[q][0][s].data_ptr(), outs[q][1][s].data_ptr()
    P = lambda t: C.c_void_p(t.data_ptr())                    # noqa: E731
    conv = [(P(surf[g][0]), in_pitch[g], P(surf[g][1]), in_pitch[g], w, h, n, P(bgr_in[g])) for g, (w, h, n) in enumerate(geoms)]
    to_bgr, step_nv12, step_surf = L.bsx_nv12_to_bgr, L.bsx_step_batch_vcam_geoms_outs_nv12, L.bsx_step_batch_surfaces

    def leg_a():
        rc = 0
        for c in conv:
            rc = rc or to_bgr(ctx_a.h, *c, stream)
        rc = rc or step_nv12(ctx_a.h, ids, items_a, total, recs_a, m, stream, 0)
        if rc != 0:
            raise SystemExit("leg A failed: %s" % (L.bsx_last_error(ctx_a.h) or b"").decode())

    def leg_b():
        if step_surf(ctx_b.h, ids, items_b, total, recs_b, m, stream, 0) != 0:
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
        for y, uv in outs:
            hsh.update(y.cpu().numpy().tobytes())
            hsh.update(uv.cpu().numpy().tobytes())
        return hsh.hexdigest()[:16]

    for _ in range(WARM_UP):                                     # tables, rings, code objects; the temporal states settle (the surfaces do not change)
        leg_a()
        leg_b()
    torch.cuda.synchronize()
    fleet = dict(model="lite", classes=[list(g) for g in geoms], streams=total, layers=[list(l) for l in layers], in_pitches=in_pitch, pitches=pitch, records=m)
    ok = True
    if args.steps_only:
        fn = leg_a if args.steps_only == "A" else leg_b
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        result = dict(fleet, leg=args.steps_only, ticks=args.steps, warm_up_ticks_of_each_leg=WARM_UP)
    else:
        ks = {leg: max(3, int(args.window / (timed(fn, 3) / 1e3)) + 1) for leg, fn in (("A", leg_a), ("B", leg_b))}
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
        states = bool(torch.equal(ctx_a.ofinal(), ctx_b.ofinal())) and all(bool(torch.equal(ctx_a.masks_of(s), ctx_b.masks_of(s))) for s in range(total))
        med = {k: statistics.median(v) for k, v in ms.items()}
        result = dict(
            fleet,
            A=dict(median_ms=round(med["A"], 5), min_ms=round(min(ms["A"]), 5), max_ms=round(max(ms["A"]), 5), ticks_per_window=ks["A"], calls_per_tick=1 + len(conv)),
            B=dict(median_ms=round(med["B"], 5), min_ms=round(min(ms["B"]), 5), max_ms=round(max(ms["B"]), 5), ticks_per_window=ks["B"], calls_per_tick=1),
            a_vs_a=dict(median_ms=round(statistics.median(aa), 5), min_ms=round(min(aa), 5), max_ms=round(max(aa), 5), spread_ms=round(spread, 5)),
            b_over_a=round(med["B"] / med["A"], 4), a_minus_b_ms=round(med["A"] - med["B"], 5),
            difference_inside_spread=bool(abs(med["B"] - med["A"]) <= spread),
            b_faster_beyond_spread=bool(med["A"] - med["B"] > spread),
            digest_a=da, digest_b=db, digests_equal=da == db, states_equal=states)
        ok = da == db and states
    for c in (ctx_a, ctx_b):
        c.close()
    line = json.dumps(dict(tool="surfaces_ab", device=torch.cuda.get_device_name(0), rounds=args.rounds, window_s=args.window, result=result))
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    if not ok:
        raise SystemExit("the two legs' planes or states differ")


if __name__ == "__main__":
    main()
