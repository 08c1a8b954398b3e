"""A/B of the main loop at the virtual camera's geometry (--vg differs from the capture size, app/deepseg.cc:675-679), in one process on one GPU:

  A: bsx_step_batch_ex (full-size composite) + bsx_resize_bgr [+ bsx_bgr_to_yuyv]   — the separate calls
  B: bsx_step_batch_vcam                                                             — the resize folded into the composite

Each configuration: A and B on contexts of their own, warmed up, then timed alternately (A, B, A, B, ...) with device events over windows of at least
--window seconds.  Afterwards both contexts are reset and run the timed batch once more: the outputs must be identical bytes.  The HBM bytes per camera
pixel after the network are computed from the shapes.  Prints ONE JSON line.

usage: python tools/vcam_ab.py [--rounds 4] [--window 0.25] [--n 256] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONFIGS = [  # (model key, capture, vcam, YUYV out)
    ("mlkit", (1280, 720), (640, 360), False),
    ("mlkit", (1280, 720), (640, 360), True),
    ("lite", (640, 480), (1280, 720), True),
]


def bytes_per_camera_pixel(W, H, ow, oh, yuyv):
    """HBM traffic after the network, per camera pixel, from the shapes (every operand counted once per pass that touches it)."""
    r = ow * oh / (W * H)
    a = (3 + 3 + 1 + 3) + 3 + 3 * r + ((3 + 2) * r if yuyv else 0)     # step: frame, bg, mask out, composite out; resize: composite in, out; [pack: in, out]
    b = 1 + (3 + 3 + 1) + (2 if yuyv else 3) * r                        # mask out; frame, bg, mask in; output
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("vcam_ab needs a GPU (torch.cuda.is_available() is False): nothing is measured on the CPU")
    import backscrub_amd
    from backscrub_amd import api, synth
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import model_path
    L = api.lib()
    n = args.n
    results = []
    for key, (W, H), (ow, oh), yuyv in CONFIGS:
        path = model_path(key)
        base = [synth.frame(W, H, s, 0) for s in range(16)]
        frames = torch.from_numpy(np.stack([base[i % 16] for i in range(n)])).cuda()
        bg = torch.from_numpy(synth.background(W, H)).cuda()
        full = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
        rsz = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device="cuda")
        out_a = torch.empty((n, oh, ow, 2 if yuyv else 3), dtype=torch.uint8, device="cuda")
        out_b = torch.empty_like(out_a)
        ma = backscrub_amd.MaskGen(path, W, H, n_streams=n)
        mb = backscrub_amd.MaskGen(path, W, H, n_streams=n)
        P = lambda t: ctypes.c_void_p(t.data_ptr())                    # noqa: E731

        def run_a():
            ma.step_ex(frames, bg, full)
            s = api._stream_ptr()
            api._check(L.bsx_resize_bgr(ma.h, P(full), W, H, P(rsz if yuyv else out_a), ow, oh, n, s), ma.h, "bsx_resize_bgr")
            if yuyv:
                api._check(L.bsx_bgr_to_yuyv(ma.h, P(rsz), P(out_a), ow, oh, n, s), ma.h, "bsx_bgr_to_yuyv")

        def run_b():
            mb.step_vcam(frames, bg, out_b, yuyv=yuyv)

        def timed(fn, k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(k):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / k

        for fn in (run_a, run_b):                                       # warm-up: code objects, tables, scratch
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ks = {}
        for name, fn in (("A", run_a), ("B", run_b)):
            ks[name] = max(3, int(args.window / (timed(fn, 3) / 1e3)) + 1)
        ms = {"A": [], "B": []}
        for _ in range(args.rounds):
            for name, fn in (("A", run_a), ("B", run_b)):
                ms[name].append(timed(fn, ks[name]))
        ma.reset()
        mb.reset()
        run_a()
        run_b()
        torch.cuda.synchronize()
        identical = bool(torch.equal(out_a, out_b)) and bool(torch.equal(ma.masks(), mb.masks()))
        ma.close()
        mb.close()
        ba, bb = bytes_per_camera_pixel(W, H, ow, oh, yuyv)
        ma_ms, mb_ms = statistics.median(ms["A"]), statistics.median(ms["B"])
        results.append(dict(model=key, capture=[W, H], vcam=[ow, oh], yuyv=yuyv, n=n, identical=identical,
                            A_ms_per_step=round(ma_ms, 4), B_ms_per_step=round(mb_ms, 4),
                            A_frames_per_s=round(n / ma_ms * 1e3, 1), B_frames_per_s=round(n / mb_ms * 1e3, 1),
                            A_rounds_ms=[round(v, 4) for v in ms["A"]], B_rounds_ms=[round(v, 4) for v in ms["B"]], steps_per_window=ks,
                            A_bytes_per_camera_px=round(ba, 2), B_bytes_per_camera_px=round(bb, 2)))
        del frames, bg, full, rsz, out_a, out_b
        torch.cuda.empty_cache()
    line = json.dumps(dict(tool="vcam_ab", device=torch.cuda.get_device_name(0), configs=results))
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not all(r["identical"] for r in results):
        raise SystemExit("A and B outputs differ")


if __name__ == "__main__":
    main()
