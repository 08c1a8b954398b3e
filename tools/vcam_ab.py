"""A/B of the main loop at the virtual camera's geometry (--vg differs from the capture size, app/deepseg.cc:675-679), in one process on one GPU:

  A: bsx_step_batch_ex (full-size composite) + bsx_resize_bgr [+ bsx_bgr_to_yuyv]   — the separate calls
  B: bsx_step_batch_vcam                                                             — the resize folded into the composite
  C: bsx_step_batch_vcam_mixed, every stream on B's setting                          — the per-stream form of B: what its descriptors cost

and, for batches whose streams do NOT share one setting (MIX_CONFIGS, the KINDS table below cycled over the streams):

  A: bsx_step_batch_mixed into a capture-size scratch + bsx_resize_bgr [+ bsx_bgr_to_yuyv]   — what a caller had to run for per-stream settings
  C: bsx_step_batch_vcam_mixed                                                               — one pass

Each configuration: every leg on a context of its own, warmed up, then timed alternately (A, B, C, A, B, C, ...) with device events over windows of at least
--window seconds.  Afterwards the contexts are reset and run the timed batch once more: the outputs must be identical bytes.  The HBM bytes per camera
pixel after the network are computed from the shapes.  Prints ONE JSON line.

--trace: no timing — legs B and C (uniform settings) 43 steps each per TRACE_CONFIGS entry, for `rocprofv3 --kernel-trace --stats -- python tools/vcam_ab.py --trace`
(a run of its own: the two kernels, vcam_blend_resize_k and vg_mixed_k, side by side on the same batch; the last entry's table takes the direct-tap form).

usage: python tools/vcam_ab.py [--rounds 4] [--window 0.25] [--n 256] [--out FILE] [--trace]
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


TRACE_CONFIGS = [CONFIGS[0], CONFIGS[2], ("mlkit", (1280, 720), (160, 90), False)]
MIX_CONFIGS = [
    ("lite", (640, 480), (1280, 720), True),
    ("mlkit", (1280, 720), (854, 480), True),
]
# per stream: (background: "own" / gallery index / None, StreamSetting arguments)
KINDS = [("own", {}), (0, {}), (1, {"flip_h": True}), (2, {"flip_v": True}), ("own", {"flip_h": True, "flip_v": True}), (None, {"bgblur": 7}),
         (None, {"bgblur": 25}), (None, {"bgblur": 7, "flip_h": True}), (1, {"filter_off": True}), (None, {"filter_off": True, "flip_h": True}),
         (0, {"filter_off": True, "bgblur": 25, "flip_v": True}), (2, {})]


def mixed_bytes_per_camera_pixel(W, H, ow, oh, yuyv, kinds):
    """the same count for a heterogeneous batch, averaged over its streams: a blur stream adds the blur pass (frame in, blurred frame out) to either leg; a
    filter-off stream reads neither background nor mask in the pass that composites it"""
    r = ow * oh / (W * H)
    a = c = 0.0
    for _, kf in kinds:
        off = kf.get("filter_off", False)
        blur = 6 if (kf.get("bgblur", 0) > 1 and not off) else 0
        a += blur + (3 + 1 + 3 if off else 3 + 3 + 1 + 3) + 3 + 3 * r + ((3 + 2) * r if yuyv else 0)
        c += blur + 1 + (3 if off else 3 + 3 + 1) + (2 if yuyv else 3) * r
    return a / len(kinds), c / len(kinds)


def timed(torch, fn, k):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(k):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / k


def interleaved(torch, legs, rounds, window):
    """legs: [(name, fn)], warmed up here, then `rounds` rounds of one window per leg in turn -> ({name: [ms per step]}, {name: steps per window})"""
    for _, fn in legs:                                                  # warm-up: code objects, tables, scratch
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ks = {name: max(3, int(window / (timed(torch, fn, 3) / 1e3)) + 1) for name, fn in legs}
    ms = {name: [] for name, _ in legs}
    for _ in range(rounds):
        for name, fn in legs:
            ms[name].append(timed(torch, fn, ks[name]))
    return ms, ks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
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
    if args.trace:
        for key, (W, H), (ow, oh), yuyv in TRACE_CONFIGS:
            base = [synth.frame(W, H, s, 0) for s in range(16)]
            frames = torch.from_numpy(np.stack([base[i % 16] for i in range(n)])).cuda()
            bg = torch.from_numpy(synth.background(W, H)).cuda()
            out = torch.empty((n, oh, ow, 2 if yuyv else 3), dtype=torch.uint8, device="cuda")
            mb = backscrub_amd.MaskGen(model_path(key), W, H, n_streams=n)
            mc = backscrub_amd.MaskGen(model_path(key), W, H, n_streams=n)
            uniform = [backscrub_amd.StreamSetting(bg=bg) for _ in range(n)]
            for _ in range(43):
                mb.step_vcam(frames, bg, out, yuyv=yuyv)
            torch.cuda.synchronize()
            for _ in range(43):
                mc.step_vcam_mixed(frames, out, uniform, yuyv=yuyv)
            torch.cuda.synchronize()
            mb.close()
            mc.close()
        print(json.dumps(dict(tool="vcam_ab", trace=[list(map(str, c)) for c in TRACE_CONFIGS], steps_per_leg=43)))
        return
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
        out_c = torch.empty_like(out_a)
        ma = backscrub_amd.MaskGen(path, W, H, n_streams=n)
        mb = backscrub_amd.MaskGen(path, W, H, n_streams=n)
        mc = backscrub_amd.MaskGen(path, W, H, n_streams=n)
        uniform = [backscrub_amd.StreamSetting(bg=bg) for _ in range(n)]
        P = lambda t: ctypes.c_void_p(t.data_ptr())                    # noqa: E731

        def run_a():
            ma.step_ex(frames, bg, full)
            s = api._stream_ptr()
            api._check(L.bsx_resize_bgr(ma.h, P(full), W, H, P(rsz if yuyv else out_a), ow, oh, n, s), ma.h, "bsx_resize_bgr")
            if yuyv:
                api._check(L.bsx_bgr_to_yuyv(ma.h, P(rsz), P(out_a), ow, oh, n, s), ma.h, "bsx_bgr_to_yuyv")

        def run_b():
            mb.step_vcam(frames, bg, out_b, yuyv=yuyv)

        def run_c():
            mc.step_vcam_mixed(frames, out_c, uniform, yuyv=yuyv)

        ms, ks = interleaved(torch, [("A", run_a), ("B", run_b), ("C", run_c)], args.rounds, args.window)
        for m in (ma, mb, mc):
            m.reset()
        run_a()
        run_b()
        run_c()
        torch.cuda.synchronize()
        identical = (bool(torch.equal(out_a, out_b)) and bool(torch.equal(ma.masks(), mb.masks())) and bool(torch.equal(out_c, out_b))
                     and bool(torch.equal(mc.masks(), mb.masks())))
        for m in (ma, mb, mc):
            m.close()
        ba, bb = bytes_per_camera_pixel(W, H, ow, oh, yuyv)
        ma_ms, mb_ms, mc_ms = statistics.median(ms["A"]), statistics.median(ms["B"]), statistics.median(ms["C"])
        results.append(dict(model=key, capture=[W, H], vcam=[ow, oh], yuyv=yuyv, n=n, identical=identical,
                            A_ms_per_step=round(ma_ms, 4), B_ms_per_step=round(mb_ms, 4), C_ms_per_step=round(mc_ms, 4),
                            A_frames_per_s=round(n / ma_ms * 1e3, 1), B_frames_per_s=round(n / mb_ms * 1e3, 1), C_frames_per_s=round(n / mc_ms * 1e3, 1),
                            A_rounds_ms=[round(v, 4) for v in ms["A"]], B_rounds_ms=[round(v, 4) for v in ms["B"]], C_rounds_ms=[round(v, 4) for v in ms["C"]],
                            B_min_max_ms=[round(min(ms["B"]), 4), round(max(ms["B"]), 4)], C_median_inside_B_range=bool(min(ms["B"]) <= mc_ms <= max(ms["B"])),
                            steps_per_window=ks, A_bytes_per_camera_px=round(ba, 2), B_bytes_per_camera_px=round(bb, 2), C_bytes_per_camera_px=round(bb, 2)))
        del frames, bg, full, rsz, out_a, out_b, out_c, uniform
        torch.cuda.empty_cache()
    mixed = []
    for key, (W, H), (ow, oh), yuyv in MIX_CONFIGS:
        path = model_path(key)
        base = [synth.frame(W, H, s, 0) for s in range(16)]
        frames = torch.from_numpy(np.stack([base[i % 16] for i in range(n)])).cuda()
        gallery = torch.from_numpy(np.stack([synth.background(W, H, seed=31 + s) for s in range(3)])).cuda()
        own = torch.from_numpy(np.stack([synth.background(W, H, seed=11 + s) for s in range(len(KINDS))])).cuda()
        kinds = [KINDS[i % len(KINDS)] for i in range(n)]
        sett = [backscrub_amd.StreamSetting(bg=None if b is None else (own[i % len(KINDS)] if b == "own" else gallery[b]), **kf) for i, (b, kf) in enumerate(kinds)]
        full = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
        rsz = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device="cuda")
        out_a = torch.empty((n, oh, ow, 2 if yuyv else 3), dtype=torch.uint8, device="cuda")
        out_c = torch.empty_like(out_a)
        ma = backscrub_amd.MaskGen(path, W, H, n_streams=n)
        mc = backscrub_amd.MaskGen(path, W, H, n_streams=n)
        P = lambda t: ctypes.c_void_p(t.data_ptr())                    # noqa: E731

        def mix_a():
            ma.step_mixed(frames, full, sett)
            s = api._stream_ptr()
            api._check(L.bsx_resize_bgr(ma.h, P(full), W, H, P(rsz if yuyv else out_a), ow, oh, n, s), ma.h, "bsx_resize_bgr")
            if yuyv:
                api._check(L.bsx_bgr_to_yuyv(ma.h, P(rsz), P(out_a), ow, oh, n, s), ma.h, "bsx_bgr_to_yuyv")

        def mix_c():
            mc.step_vcam_mixed(frames, out_c, sett, yuyv=yuyv)

        ms, ks = interleaved(torch, [("A", mix_a), ("C", mix_c)], args.rounds, args.window)
        ma.reset()
        mc.reset()
        mix_a()
        mix_c()
        torch.cuda.synchronize()
        identical = bool(torch.equal(out_a, out_c)) and bool(torch.equal(ma.masks(), mc.masks()))
        ma.close()
        mc.close()
        ba, bc = mixed_bytes_per_camera_pixel(W, H, ow, oh, yuyv, kinds)
        ma_ms, mc_ms = statistics.median(ms["A"]), statistics.median(ms["C"])
        mixed.append(dict(model=key, capture=[W, H], vcam=[ow, oh], yuyv=yuyv, n=n, kinds=len(KINDS), identical=identical,
                          A_ms_per_step=round(ma_ms, 4), C_ms_per_step=round(mc_ms, 4), A_frames_per_s=round(n / ma_ms * 1e3, 1), C_frames_per_s=round(n / mc_ms * 1e3, 1),
                          A_rounds_ms=[round(v, 4) for v in ms["A"]], C_rounds_ms=[round(v, 4) for v in ms["C"]], steps_per_window=ks,
                          A_bytes_per_camera_px=round(ba, 2), C_bytes_per_camera_px=round(bc, 2)))
        del frames, gallery, own, sett, full, rsz, out_a, out_c
        torch.cuda.empty_cache()
    line = json.dumps(dict(tool="vcam_ab", device=torch.cuda.get_device_name(0), configs=results, mixed=mixed))
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not all(r["identical"] for r in results + mixed):
        raise SystemExit("the legs' outputs differ")


if __name__ == "__main__":
    main()
