"""A/B of the mixed-settings step (bsx_step_batch_mixed) against what a server does without it, in one process on one GPU, at BASELINE configs[1]'s geometry
(256 x 640x480, segm_lite_v681):

  (a) ex_plain     step_ex over 256 streams, one shared background
      mixed_plain  step_mixed, every stream on that plain setting                    (target: within 10 % of ex_plain)
  (b) grouped4     four step_streams calls of 64 streams each: gallery background, flip_h, bgblur 25, "filter off" (no such form: stepped over a background)
      mixed4       ONE step_mixed call with the same four groups                      (target: faster than grouped4)
  (c) copies8      step_ex over a [256,H,W,3] stride buffer holding 8 gallery images copied 32 times each
      gallery8     step_mixed with 256 streams pointing at the 8 images themselves

Each form runs on a context of its own, warmed up, then the forms are timed alternately (round after round) with device events over windows of at least --window
seconds (the two sides of each comparison alternate in the same process, as in tools/streams_ab.py).  Prints ONE JSON line: per form the median ms
per step and the spread (min / max over the rounds), and the three ratios.

--trace: no timing — step (b)'s mixed call a few times at 640x480 lite and at 1280x720 MLKit (a geometry with strips outside the ROI), for a rocprofv3 kernel trace.

usage: python tools/mixed_ab.py [--rounds 7] [--window 0.25] [--n 256] [--out FILE] [--trace]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _four_groups(bs, n, gallery):
    """(b)'s settings: four contiguous groups of n / 4 streams"""
    q = n // 4
    S = bs.StreamSetting
    return [S(bg=gallery[0])] * q + [S(bg=gallery[1], flip_h=True)] * q + [S(bgblur=25)] * q + [S(filter_off=True)] * (n - 3 * q)


def trace(bs, model_path, synth, torch, np):
    for key, (W, H), n in (("lite", (640, 480), 256), ("mlkit", (1280, 720), 64)):
        mg = bs.MaskGen(model_path(key), W, H, n_streams=n)
        frames = torch.from_numpy(np.stack([synth.frame(W, H, s % 16, 0) for s in range(n)])).cuda()
        gallery = torch.from_numpy(np.stack([synth.background(W, H, seed=1 + k) for k in range(2)])).cuda()
        out = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
        sett = _four_groups(bs, n, gallery)
        for _ in range(5):
            mg.step_mixed(frames, out, sett)
        torch.cuda.synchronize()
        mg.close()
    print(json.dumps(dict(tool="mixed_ab", mode="trace", device=torch.cuda.get_device_name(0))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mixed_ab needs a GPU (torch.cuda.is_available() is False): nothing is measured on the CPU")
    import backscrub_amd as bs
    from backscrub_amd import synth
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import model_path
    if args.trace:
        return trace(bs, model_path, synth, torch, np)
    n, q = args.n, args.n // 4
    W, H = 640, 480
    path = model_path("lite")
    base = [synth.frame(W, H, s, 0) for s in range(16)]
    frames = torch.from_numpy(np.stack([base[i % 16] for i in range(n)])).cuda()
    gallery = torch.from_numpy(np.stack([synth.background(W, H, seed=1 + k) for k in range(8)])).cuda()
    bg = gallery[0]
    copies = gallery[torch.arange(n, device="cuda") % 8].contiguous()            # the workaround: every stream's background copied into a stride buffer
    names = ("ex_plain", "mixed_plain", "grouped4", "mixed4", "copies8", "gallery8")
    outs = {k: torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda") for k in names}
    ctx = {k: bs.MaskGen(path, W, H, n_streams=n) for k in names}
    plain = [bs.StreamSetting(bg=bg)] * n
    four = _four_groups(bs, n, gallery)
    gal = [bs.StreamSetting(bg=gallery[i % 8]) for i in range(n)]
    groups = [(list(range(k * q, (k + 1) * q if k < 3 else n)), kw) for k, kw in enumerate(
        [dict(bg=gallery[0]), dict(bg=gallery[1], flip_h=True), dict(bg=None, bgblur=25), dict(bg=gallery[2])])]

    def grouped():
        c, o = ctx["grouped4"], outs["grouped4"]
        for ids, kw in groups:
            a, b = ids[0], ids[-1] + 1
            kw = dict(kw)
            c.step_streams(ids, frames[a:b], kw.pop("bg"), o[a:b], **kw)

    forms = {
        "ex_plain": lambda: ctx["ex_plain"].step_ex(frames, bg, outs["ex_plain"]),
        "mixed_plain": lambda: ctx["mixed_plain"].step_mixed(frames, outs["mixed_plain"], plain),
        "grouped4": grouped,
        "mixed4": lambda: ctx["mixed4"].step_mixed(frames, outs["mixed4"], four),
        "copies8": lambda: ctx["copies8"].step_ex(frames, copies, outs["copies8"]),
        "gallery8": lambda: ctx["gallery8"].step_mixed(frames, outs["gallery8"], gal),
    }

    def timed(fn, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(k):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / k

    for fn in forms.values():                                        # warm-up: code objects, tables, the rings, the blur scratch
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ks = {name: max(3, int(args.window / (timed(fn, 3) / 1e3)) + 1) for name, fn in forms.items()}
    ms = {name: [] for name in forms}
    for _ in range(args.rounds):
        for name, fn in forms.items():
            ms[name].append(timed(fn, ks[name]))
    # the same bytes: plain mixed = step_ex, gallery = copies (fresh state on both sides)
    same = {}
    for a, b in (("ex_plain", "mixed_plain"), ("copies8", "gallery8")):
        ctx[a].reset()
        ctx[b].reset()
        forms[a]()
        forms[b]()
        torch.cuda.synchronize()
        same[b] = bool(torch.equal(outs[a], outs[b]) and torch.equal(ctx[a].masks(), ctx[b].masks()) and torch.equal(ctx[a].ofinal(), ctx[b].ofinal()))
    for c in ctx.values():
        c.close()
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = {k: dict(median_ms=round(med[k], 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), rounds_ms=[round(x, 4) for x in v], steps_per_window=ks[k])
           for k, v in ms.items()}
    ratios = dict(mixed_plain_over_ex_plain=round(med["mixed_plain"] / med["ex_plain"], 4), mixed4_over_grouped4=round(med["mixed4"] / med["grouped4"], 4),
                  gallery8_over_copies8=round(med["gallery8"] / med["copies8"], 4))
    line = json.dumps(dict(tool="mixed_ab", device=torch.cuda.get_device_name(0), model=os.path.basename(path), capture=[W, H], n=n, identical=same, forms=res,
                           ratios=ratios))
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not all(same.values()):
        raise SystemExit("a mixed form and its dense counterpart differ: %s" % same)


if __name__ == "__main__":
    main()
