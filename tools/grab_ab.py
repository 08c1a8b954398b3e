"""A/B of one tick's background grabs for a server whose cameras each play their own background, in one process on one GPU:

  A   the loop of n bsx_background_grab calls (n resize_bgr_k launches; code the batch call does not touch)
  B   ONE bsx_background_grab_batch call (one resize_bgr_batch_k launch behind one descriptor copy)

for n in {1, 16, 256} outputs of 640x480 from synthetic sources of mixed native sizes — up-scale, down-scale, the exact 2x area mean, the identity — half of
them stills, half two-picture animations slow enough (one picture per 10^4 s) that both legs name picture 1 for as long as the tool runs, so that their outputs
can be compared.  Both legs go through the raw C ABI with their arguments prepared, so the host side of a leg is its HIP calls plus one foreign call each.

Per n: warm-up (every table exists, the ring is allocated); then leg A against ITSELF, alternating, which gives the run-to-run spread of this machine
(max - min of its windows' ms per tick); then A and B alternating.  A window repeats its leg until at least --window seconds have passed (never a fraction of a
millisecond) between two device events; ms per tick = window / repetitions.  Prints ONE JSON line: per n both legs' median, min and max, the spread, both output
digests, and the bytes a tick must move, computed from the shapes (the same for both legs: they differ in launches, not in bytes).

usage: python tools/grab_ab.py [--n 1,16,256] [--rounds 7] [--window 0.05] [--out FILE]
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

W, H = 640, 480
SIZES = [(320, 240), (1280, 720), (1280, 960), (640, 480), (517, 333), (1920, 1080)]     # up, down, exact 2x, identity, up, down


def tick_bytes(sizes):
    """what one tick must move for these sources -> W x H: every output byte written once; of a source, the pixels its taps name — all of it when it is no larger
    than four taps per output pixel (up-scale, 2x, identity), else four pixels per output pixel; plus the tables' rows and columns and one descriptor each"""
    rd = sum(3 * min(sw * sh, 4 * W * H) for sw, sh in sizes)
    wr = len(sizes) * W * H * 3
    tab = sum(0 if (sw, sh) in ((W, H), (2 * W, 2 * H)) else (W + H) * 8 for sw, sh in set(sizes))
    return dict(read=rd, write=wr, tables=tab, descriptors=64 * len(sizes), total=rd + wr + tab + 64 * len(sizes))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="1,16,256")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.05)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("grab_ab needs a GPU (torch.cuda.is_available() is False): nothing is measured on the CPU")
    import backscrub_amd
    from backscrub_amd import api
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import model_path
    ns = [int(v) for v in args.n.split(",")]
    n_max = max(ns)
    L = api.lib()
    mg = backscrub_amd.MaskGen(model_path("lite"), W, H, n_streams=n_max)
    rng = np.random.default_rng(3)
    proto = {}
    for sw, sh in SIZES:                                              # one pair of pictures per size; every source gets its own copy on the GPU
        proto[(sw, sh)] = rng.integers(0, 256, (2, sh, sw, 3), dtype=np.uint8)
    sizes = [SIZES[i % len(SIZES)] for i in range(n_max)]
    bgs = [backscrub_amd.Background(mg, frames=proto[s][: 1 + (i // len(SIZES)) % 2], fps=1e-4) for i, s in enumerate(sizes)]
    out_a = torch.zeros((n_max, H, W, 3), dtype=torch.uint8, device="cuda")
    out_b = torch.zeros((n_max, H, W, 3), dtype=torch.uint8, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    img = W * H * 3
    handles = (C.c_void_p * n_max)(*[b.h for b in bgs])
    nos = (C.c_int * n_max)()
    dst_a = [C.c_void_p(out_a.data_ptr() + i * img) for i in range(n_max)]
    p_b = C.c_void_p(out_b.data_ptr())
    grab, grab_batch = L.bsx_background_grab, L.bsx_background_grab_batch

    def leg_a(n):
        for i in range(n):
            if grab(handles[i], W, H, dst_a[i], stream) != 1:
                raise SystemExit("leg A: source %d is not at picture 1" % i)

    def leg_b(n):
        if grab_batch(handles, n, W, H, p_b, img, -1.0, nos, stream) != 0:
            raise SystemExit("leg B failed: %s" % (L.bsx_last_error(mg.h) or b"").decode())

    def timed(fn, n, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(k):
            fn(n)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / k

    def digest(t, n):
        return hashlib.sha256(t[:n].cpu().numpy().tobytes()).hexdigest()[:16]

    results = {}
    ok = True
    for n in ns:
        for _ in range(3):                                            # warm-up: tables, ring, code objects
            leg_a(n)
            leg_b(n)
        torch.cuda.synchronize()
        if list(nos[:n]) != [1] * n:
            raise SystemExit("leg B: not every source is at picture 1: %s" % list(nos[:n]))
        ks = {name: max(3, int(args.window / (timed(fn, n, 3) / 1e3)) + 1) for name, fn in (("A", leg_a), ("B", leg_b))}
        aa = []
        for _ in range(args.rounds):                                  # A against itself: the spread
            aa.append(timed(leg_a, n, ks["A"]))
            aa.append(timed(leg_a, n, ks["A"]))
        spread = max(aa) - min(aa)
        ms = {"A": [], "B": []}
        for _ in range(args.rounds):
            ms["A"].append(timed(leg_a, n, ks["A"]))
            ms["B"].append(timed(leg_b, n, ks["B"]))
        torch.cuda.synchronize()
        da, db = digest(out_a, n), digest(out_b, n)
        med = {k: statistics.median(v) for k, v in ms.items()}
        by = tick_bytes(sizes[:n])
        results[str(n)] = dict(
            A=dict(median_ms=round(med["A"], 5), min_ms=round(min(ms["A"]), 5), max_ms=round(max(ms["A"]), 5), ticks_per_window=ks["A"], launches_per_tick=n),
            B=dict(median_ms=round(med["B"], 5), min_ms=round(min(ms["B"]), 5), max_ms=round(max(ms["B"]), 5), ticks_per_window=ks["B"], launches_per_tick=1),
            a_vs_a=dict(median_ms=round(statistics.median(aa), 5), min_ms=round(min(aa), 5), max_ms=round(max(aa), 5), spread_ms=round(spread, 5)),
            b_over_a=round(med["B"] / med["A"], 4), a_minus_b_ms=round(med["A"] - med["B"], 5), digest_a=da, digest_b=db, digests_equal=da == db,
            bytes_per_tick=by, b_gbytes_per_s=round(by["total"] / (med["B"] * 1e-3) / 1e9, 1), a_gbytes_per_s=round(by["total"] / (med["A"] * 1e-3) / 1e9, 1))
        ok = ok and da == db
    for b in bgs:
        b.close()
    mg.close()
    line = json.dumps(dict(tool="grab_ab", device=torch.cuda.get_device_name(0), output=[W, H], source_sizes=SIZES, rounds=args.rounds, window_s=args.window, n=results))
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not ok:
        raise SystemExit("the two legs' outputs differ")


if __name__ == "__main__":
    main()
