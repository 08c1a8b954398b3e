"""A/B of one tick of a simulcast forwarder that feeds video encoders — every camera published at several sizes at once, each layer an NV12 surface with a row
pitch — in one process on one GPU, same build, same fleet (tools/vcam_outs_ab.py's):

  A   bsx_step_batch_vcam_geoms_outs with BGR out, a layer's records laid out contiguously, then one bsx_bgr_to_nv12 per layer size: 1 + sizes calls, every layer
      written as 3 B/px and read back once
  B   ONE bsx_step_batch_vcam_geoms_outs_nv12 call: the resize pass stores Y and 2x2-subsampled chroma, 1.5 B/px, from the registers that hold the pixels

Fleet: segm_lite, 64 x 640x480 + 64 x 1280x720 + 64 x 640x360, every stream at 640x360 + 320x180 + 160x90 (--layers and --per-class change it); a plane's pitch is
its width rounded up to --pitch-align bytes (256: the 160-wide layer sits in rows of 256 bytes).

Each leg has a context of its own (both made the same way), so neither advances the other's temporal state.  Both go through the raw C ABI with their arguments
prepared.  Warm-up (every table exists, the rings are allocated); then leg A against ITSELF, alternating, which gives the run-to-run spread of this machine in this
run (max - min of its windows' ms per tick); then A and B alternating.  A window repeats its leg until at least --window seconds have passed between two device
events; ms per tick = window / repetitions.  Both legs see the same frames every tick, so their temporal states settle on the same values and the planes are
compared by digest.  Prints ONE JSON line.  No bar is set: the figures are recorded, whichever way they fall (docs/design/05e-host-side.md has them: B is 7 % faster for the three layers, 2.6 % for one).

    python tools/vcam_nv12_ab.py [--layers 640x360,320x180,160x90] [--per-class 64] [--pitch-align 256] [--rounds 7] [--window 0.3] [--out FILE]
    python tools/vcam_nv12_ab.py --steps-only B --steps 10        # no timing: warm-up, then that many ticks of one leg (for a kernel trace)
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
        raise SystemExit("vcam_nv12_ab needs a GPU (torch.cuda.is_available() is False): nothing is measured on the CPU")
    import backscrub_amd
    from backscrub_amd import api, synth
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import model_path
    L = api.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    geoms = [(w, h, args.per_class) for w, h in SIZES]
    total = sum(n for _, _, n in geoms)
    path = model_path("lite")
    frames = [torch.from_numpy(synth.frames(n, w, h, t=0, distinct=4)).cuda() for w, h, n in geoms]
    gallery = [torch.from_numpy(np.stack([synth.background(w, h, seed=21 + k) for k in range(2)])).cuda() for w, h, _n in geoms]
    order = [int(i) for i in np.random.default_rng(11).permutation(total)]
    ctx_a, ctx_b = (backscrub_amd.MaskGen.with_geometries(path, geoms) for _ in range(2))
    first = [g["first_stream"] for g in ctx_a.geometries()]
    pitch = [(ow + args.pitch_align - 1) // args.pitch_align * args.pitch_align for ow, _oh in layers]
    bgr = [torch.zeros((total, oh, ow, 3), dtype=torch.uint8, device="cuda") for ow, oh in layers]      # leg A's packed layers, stream s at index s

    def planes():
        """per layer (Y [total, oh, pitch], UV [total, oh / 2, pitch]): stream s's surface at index s of each"""
        return [(torch.zeros((total, oh, p), dtype=torch.uint8, device="cuda"), torch.zeros((total, oh // 2, p), dtype=torch.uint8, device="cuda"))
                for (_ow, oh), p in zip(layers, pitch)]
    out_a, out_b = planes(), planes()
    ids = (C.c_int * total)(*order)
    items = (api._GeomItem * total)()
    m = total * len(layers)
    recs_a, recs_b = (api._VcamOut * m)(), (api._VcamOutNv12 * m)()
    for i, s in enumerate(order):
        g = max(j for j, f0 in enumerate(first) if f0 <= s)
        k = s - first[g]
        items[i].d_frame, items[i].d_out = frames[g][k].data_ptr(), None
        items[i].setting.d_bg, items[i].setting.flags = gallery[g][s % 2].data_ptr(), FLAG_CYCLE[s % 4]
        for q, (ow, oh) in enumerate(layers):                      # the records as a forwarder has them: per camera, its layers
            a, b = recs_a[i * len(layers) + q], recs_b[i * len(layers) + q]
            a.item, a.out_w, a.out_h, a.d_out = i, ow, oh, bgr[q][s].data_ptr()
            b.item, b.out_w, b.out_h, b.pitch_y, b.pitch_uv, b.d_y, b.d_uv = i, ow, oh, pitch[q], pitch[q], out_b[q][0][s].data_ptr(), out_b[q][1][s].data_ptr()
    P = lambda t: C.c_void_p(t.data_ptr())                    # noqa: E731
    conv = [(P(bgr[q]), ow, oh, P(out_a[q][0]), pitch[q], P(out_a[q][1]), pitch[q]) for q, (ow, oh) in enumerate(layers)]
    step_outs, to_nv12, step_nv12 = L.bsx_step_batch_vcam_geoms_outs, L.bsx_bgr_to_nv12, L.bsx_step_batch_vcam_geoms_outs_nv12

    def leg_a():
        rc = step_outs(ctx_a.h, ids, items, total, recs_a, m, stream, 0)
        for src, ow, oh, y, py, uv, puv in conv:
            rc = rc or to_nv12(ctx_a.h, src, ow, oh, total, y, py, uv, puv, stream)
        if rc != 0:
            raise SystemExit("leg A failed: %s" % (L.bsx_last_error(ctx_a.h) or b"").decode())

    def leg_b():
        if step_nv12(ctx_b.h, ids, items, total, recs_b, m, stream, 0) != 0:
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

    for _ in range(WARM_UP):                                     # tables, rings, code objects; the temporal states settle (the frames do not change)
        leg_a()
        leg_b()
    torch.cuda.synchronize()
    fleet = dict(model="lite", classes=[list(g) for g in geoms], streams=total, layers=[list(l) for l in layers], pitches=pitch, records=m)
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
        states = bool(torch.equal(ctx_a.ofinal(), ctx_b.ofinal()))
        med = {k: statistics.median(v) for k, v in ms.items()}
        result = dict(
            fleet,
            A=dict(median_ms=round(med["A"], 5), min_ms=round(min(ms["A"]), 5), max_ms=round(max(ms["A"]), 5), ticks_per_window=ks["A"], calls_per_tick=1 + len(conv)),
            B=dict(median_ms=round(med["B"], 5), min_ms=round(min(ms["B"]), 5), max_ms=round(max(ms["B"]), 5), ticks_per_window=ks["B"], calls_per_tick=1),
            a_vs_a=dict(median_ms=round(statistics.median(aa), 5), min_ms=round(min(aa), 5), max_ms=round(max(aa), 5), spread_ms=round(spread, 5)),
            b_over_a=round(med["B"] / med["A"], 4), a_minus_b_ms=round(med["A"] - med["B"], 5),
            difference_inside_spread=bool(abs(med["B"] - med["A"]) <= spread),
            digest_a=da, digest_b=db, digests_equal=da == db, temporal_states_equal=states)
        ok = da == db and states
    for c in (ctx_a, ctx_b):
        c.close()
    line = json.dumps(dict(tool="vcam_nv12_ab", device=torch.cuda.get_device_name(0), rounds=args.rounds, window_s=args.window, result=result))
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not ok:
        raise SystemExit("the two legs' planes differ")


if __name__ == "__main__":
    main()
