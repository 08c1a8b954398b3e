"""A/B of the step addressed by stream id (bsx_step_batch_streams) against the dense step (bsx_step_batch_ex), in one process on one GPU, at BASELINE configs[1]
(256 x 640x480, segm_lite_v681):

  dense      step_ex over streams 0 .. 255
  identity   step_streams with ids = 0 .. 255                 (the id form of the same work: target within 1 % of dense)
  permuted   step_streams with a random permutation of 0 .. 255   (target within 1 % of dense)
  dense128   step_ex over streams 0 .. 127 of a 256-stream context
  subset128  step_streams with a random 128-of-256 subset      (target within 3 % of dense128)

Each form runs on a context of its own, warmed up, then all five are timed alternately (round after round) with device events over windows of at least --window
seconds.  Afterwards the dense and identity contexts are reset and step once more: outputs, masks and temporal state must be identical bytes.  Prints ONE JSON line:
per form the median ms per step and the spread (min / max over the rounds), and the ratios to the dense forms.

usage: python tools/streams_ab.py [--rounds 7] [--window 0.25] [--n 256] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("streams_ab needs a GPU (torch.cuda.is_available() is False): nothing is measured on the CPU")
    import backscrub_amd
    from backscrub_amd import synth
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import model_path
    n, half = args.n, args.n // 2
    W, H = 640, 480
    path = model_path("lite")
    rng = np.random.default_rng(1)
    perm = rng.permutation(n)
    subset = rng.permutation(n)[:half]
    base = [synth.frame(W, H, s, 0) for s in range(16)]
    frames = torch.from_numpy(np.stack([base[i % 16] for i in range(n)])).cuda()
    bg = torch.from_numpy(synth.background(W, H)).cuda()
    outs = {k: torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda") for k in ("dense", "identity", "permuted", "dense128", "subset128")}
    ctx = {k: backscrub_amd.MaskGen(path, W, H, n_streams=n) for k in outs}
    ident = list(range(n))
    forms = {
        "dense": lambda: ctx["dense"].step_ex(frames, bg, outs["dense"]),
        "identity": lambda: ctx["identity"].step_streams(ident, frames, bg, outs["identity"]),
        "permuted": lambda: ctx["permuted"].step_streams(perm, frames, bg, outs["permuted"]),
        "dense128": lambda: ctx["dense128"].step_ex(frames[:half], bg, outs["dense128"]),
        "subset128": lambda: ctx["subset128"].step_streams(subset, frames[:half], bg, outs["subset128"]),
    }

    def timed(fn, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(k):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / k

    for fn in forms.values():                                        # warm-up: code objects, tables, the id ring
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ks = {name: max(3, int(args.window / (timed(fn, 3) / 1e3)) + 1) for name, fn in forms.items()}
    ms = {name: [] for name in forms}
    for _ in range(args.rounds):
        for name, fn in forms.items():
            ms[name].append(timed(fn, ks[name]))
    ctx["dense"].reset()
    ctx["identity"].reset()
    forms["dense"]()
    forms["identity"]()
    torch.cuda.synchronize()
    identical = bool(torch.equal(outs["dense"], outs["identity"]) and torch.equal(ctx["dense"].masks(), ctx["identity"].masks())
                     and torch.equal(ctx["dense"].ofinal(), ctx["identity"].ofinal()))
    for c in ctx.values():
        c.close()
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = {k: dict(median_ms=round(med[k], 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), rounds_ms=[round(x, 4) for x in v], steps_per_window=ks[k])
           for k, v in ms.items()}
    ratios = dict(identity_over_dense=round(med["identity"] / med["dense"], 4), permuted_over_dense=round(med["permuted"] / med["dense"], 4),
                  subset128_over_dense128=round(med["subset128"] / med["dense128"], 4))
    line = json.dumps(dict(tool="streams_ab", device=torch.cuda.get_device_name(0), model=os.path.basename(path), capture=[W, H], n=n, subset=half,
                           identical_identity_vs_dense=identical, forms=res, ratios=ratios))
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not identical:
        raise SystemExit("identity ids and the dense step differ")


if __name__ == "__main__":
    main()
