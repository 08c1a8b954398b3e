#!/usr/bin/env python3
"""bench.py — composited frames/s of the backscrub hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--full]

A plain run does only what the headline figure needs: it sets up, ramps the clocks, warms up, times the K steps, writes --dump-outputs and prints
the line.  --full then measures and checks everything else, as described below: per-launch profile and roofline, parity with the CPU oracle, the
side probes, the CPU baseline, the other BASELINE configurations and opt-in modes (and at N > 1 rank 0 alone, configs[4] and the second device).

With --gpus N > 1 and no WORLD_SIZE in the environment the script re-executes itself under
`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ...` (one rank per GPU, RCCL);
launched that way by someone else it just reads RANK / LOCAL_RANK / WORLD_SIZE.

A "step" is one pass of the whole per-frame hot path over one batch of device-resident synthetic camera frames: ROI
resize + BGR2RGB + bilateral + normalise, the segmentation network, decode + temporal IIR, mask upscale + 5x5 blur, alpha
blend with the background (`bsx_step_batch`; reference: lib/libbackscrub.cc:279-376 + app/deepseg.cc:108-134).
`value` = BASELINE.json configs[1]: batch of 256 640x480 frames, segm_lite_v681 (Google Meet 160x96), on a MOVING scene:
every step reads the next batch of a ring of RING time steps per stream (the person sways, the sensor noise is redrawn),
as a camera delivers them.  Streams are independent, so N GPUs run N such batches (weak scaling, no data-path collective);
the only RCCL traffic is the all-reduce of the throughput counters.

Rank 0 prints ONE COMPACT JSON line (< 6 KB: contract keys + roofline + cpu_baseline + one short entry per BASELINE
config) and writes everything else — per-launch tables, every leg of the CPU thread sweeps, the opt-in modes, notes — to
`bench_detail.json` next to this file (and under gpurun_out/ when that directory exists).  compact_line() is the only
place the printed line is assembled; tests/test_bench_contract.py holds it to the size limit.

`roofline.frac` has ONE definition everywhere: bytes of the launch that must cross HBM (algorithmic bytes for this input
minus the reads of cache-resident data all streams share) / hipEvent duration / 8 TB/s.  SURVEY 8(d)'s dense 10 B/px
figure is carried as `dense_10Bpx_GBps` and is never a fraction.

The oracle is used only in the cpu_baseline / parity legs — never in the measured path.
"""
import argparse
import json
import math
import os
import socket
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0      # MI355X HBM3E spec (MI355X_MICROARCH.md); ~6300 GB/s is the measured copy ceiling
FP32_PEAK_TFLOPS = 157.3   # f32 vector/matrix peak
F16_PEAK_TFLOPS = 2500.0   # dense f16 MFMA peak
LINE_LIMIT = 6144          # bytes of the printed line (the driver keeps an 8 KB tail: round 4's 22 KB line was unparsable)
RING = 4                   # time steps per stream of the moving scene
METRIC = "composited frames/sec at 640×480 (batch), 1/2/4/8 MI355X + mask IoU vs CPU ref"
NAMES = {"lite": "segm_lite_v681.tflite", "full": "segm_full_v679.tflite",
         "mlkit": "selfiesegmentation_mlkit-256x256-2021_01_19-v1215.f16.tflite", "deeplab": "deeplabv3_257_mv_gpu.tflite"}
PMC_NAMES = {"frame_program": ("bsx_mid", "frame_program_k"), "blend": "blend4x4_k", "blend(standalone)": "blend4x4_k", "mask_blend": "mask_tile_k<true",
             "mask_upscale_blur": "mask_tile_k<false", "prep": "prep_fused_k", "decode_iir": "decode_k",
             # the segment kernels: specialised by hipRTC for the loaded graph (bsx_seg_*), or the ahead-of-time templates
             "seg_head": ("bsx_seg_head", "seg_head_k"), "seg_k2": ("bsx_seg_k2", "seg_k2_k"), "seg_k3": ("bsx_seg_k3", "seg_k3_k"), "seg_tail": ("bsx_seg_tail", "seg_tail_k"),
             "seg_tail+decode": ("bsx_seg_tail", "seg_tail_k"), "seg_gate": "seg_gate_k"}
IMAGE_LAUNCHES = {"prep_resize": "prep", "prep_bilateral": "prep", "prep": "prep", "decode_iir": "decode", "mask_upscale_blur": "mask", "blend": "blend", "mask_blend": "blend"}


def cpu_description():
    """CPU model string + socket / core counts of this box ("core count and CPU model stated")."""
    model, sockets, cores = "unknown", set(), os.cpu_count() or 1
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name") and model == "unknown":
                model = line.split(":", 1)[1].strip()
            elif line.startswith("physical id"):
                sockets.add(line.split(":", 1)[1].strip())
    except OSError:
        pass
    return {"model": model, "sockets": max(len(sockets), 1), "logical_cpus": cores}


def csrc_digest():
    """Content hash of the kernel sources (backscrub_amd/csrc): what ties the committed PMC passes to the kernels that are timed.  A content hash, not a git
    tree id — the GPU box receives a snapshot without .git.  tools/merge_pmc.py stamps profiles/pmc_latest.json with the same function."""
    import hashlib
    d = os.path.join(ROOT, "backscrub_amd", "csrc")
    h = hashlib.sha256()
    for fn in sorted(os.listdir(d)):
        if fn.endswith((".hip", ".cpp", ".hpp")):
            h.update(fn.encode() + b"\0")
            h.update(open(os.path.join(d, fn), "rb").read())
    return h.hexdigest()[:16]


def pipe_of(model_name, launch_name):
    """(pipe label, peak TFLOP/s of USEFUL flops) of the arithmetic pipe a launch issues on — the denominator a flops fraction may be quoted against.
    DeepLab's 1x1 convolutions (GEMM launches `conv#N`, and the expand half of the fused `conv#N+dw#M` launches) run on v_mfma_f32_16x16x32_f16 with the
    3-term split product (f32-grade): the f16 pipe does 3 MFMAs per useful MAC → 2500 / 3; BSX_F16_GEMM=fast/fast16: 1 term; =off: the f32 pipe.
    Meet / MLKit kernels use v_mfma_f32_16x16x4_f32 (157.3 TFLOP/s); depthwise / resize / argmax work is f32 VALU (157.3)."""
    if "deeplab" in model_name and launch_name.startswith("conv#") and not launch_name.startswith("conv#0+"):     # conv#0+dw#1+conv#2 = dl_head0_k: 3x3 stem on the f32 MFMA
        mode = os.environ.get("BSX_F16_GEMM", "")
        if mode == "off":
            return "f32 MFMA (v_mfma_f32_16x16x4_f32)", FP32_PEAK_TFLOPS
        if mode in ("fast", "fast16"):
            return "f16 MFMA (v_mfma_f32_16x16x32_f16), 1 term", F16_PEAK_TFLOPS
        return "f16 MFMA (v_mfma_f32_16x16x32_f16), 3-term split product: useful peak = dense f16 peak / 3", round(F16_PEAK_TFLOPS / 3.0, 1)
    return "f32 MFMA / VALU", FP32_PEAK_TFLOPS


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--ramp-seconds", type=float, default=2.0, help="untimed clock ramp before the warmup steps: the step is repeated for this long so that "
                    "the GPU has left its idle power state (a step is ~0.4 ms: W = 20 of them do not; a cold box measured 380 k instead of 455 k frames/s)")
    ap.add_argument("--batch", type=int, default=256, help="streams per GPU")
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--model", default="lite", help="lite|full|mlkit|deeplab or a .tflite path")
    ap.add_argument("--static-scene", action="store_true", help="time the SAME batch of frames every step (rounds 1-4's protocol) instead of the moving scene")
    ap.add_argument("--per-stream-bg", action="store_true", help="every stream composites over its own background frame instead of one shared image")
    ap.add_argument("--bg-ring", action="store_true", help="animated background: every step uploads the next frame of a pinned 36-frame 480x360 ring (H2D) and resizes it on the GPU (grab_background), inside the timed region")
    ap.add_argument("--host-io", action="store_true", help="(kept for old command lines: the with-H2D/D2H leg now always runs max(20, min(steps, 100)) steps; reported as host_io, never as value)")
    ap.add_argument("--no-host-io", action="store_true", help="skip the host_io leg")
    ap.add_argument("--second-device-check", action="store_true", help="(internal, run by `--gpus N` as a subprocess of rank 0) one context on a device other than 0, checked against device 0")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extra-configs", action="store_true", help="skip the other BASELINE configurations, the opt-in modes and the single-stream legs (N = 1 only)")
    ap.add_argument("--no-side-probes", action="store_true", help="skip everything that follows the timed region of the main configuration except its per-launch profile (profiling runs: other launches would mix into the per-kernel averages)")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="target wall time of the CPU baseline sample of the main configuration (the other configurations get a third of it each)")
    ap.add_argument("--profile-iters", type=int, default=8, help="per-launch hipEvent passes (each over the next batch of the scene ring)")
    ap.add_argument("--dump-launches", default="", help="write the per-launch hipEvent table to this file")
    ap.add_argument("--detail", default="", help="where the full record goes (default: bench_detail.json next to bench.py, and gpurun_out/ when it exists)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR", help="after the timed steps of the main configuration, write what its last step handed the caller "
                    "(rank 0's composites and masks) to DIR/composite.npy and DIR/mask.npy as float32, at most 60 MB in all (a fixed, seeded sample of the streams "
                    "when the batch is larger) — with the same arguments the inputs are the same bytes every run, so two builds compare output for output")
    ap.add_argument("--selftest-dist", action="store_true", help="CPU plumbing test of the multi-process path (gloo): launch, rendezvous, counter all-reduce, JSON line — no GPU work")
    ap.add_argument("--full", action="store_true", help="after the headline figure, measure and check everything else: per-launch profile and roofline, twin-stream and "
                    "oracle parity checks, the side probes, the CPU baseline, the other BASELINE configurations and opt-in modes, single-stream latency; at N > 1 "
                    "also rank 0 alone, the configs[4] slice and the second-device check.  Without it a run sets up, warms up, times the steps, writes "
                    "--dump-outputs and prints the line; the --no-* switches, --cpu-seconds and --profile-iters then have nothing to act on")
    a = ap.parse_args()
    if a.dump_launches and not a.full:
        ap.error("--dump-launches writes the per-launch profile, which only a --full run takes")
    return a


def resolve_model(key):
    if key in NAMES:
        real = os.path.join(ROOT, "models", NAMES[key])    # model DATA the user supplies; tools/stage_models.py copies the reference's files here
        if os.path.exists(real):
            return real, NAMES[key], "reference weights"
        from tools import make_synthetic_model
        return make_synthetic_model.ensure(key), NAMES[key], "random-init weights, reference architecture"
    return key, os.path.basename(key), "user model"


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def self_launch(args):
    """--gpus N without a launcher: become `torch.distributed.run` with N ranks on this node."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.execv(sys.executable, cmd)


# ------------------------------------------------------------------------------------------------------------------------------
# CPU legs (test infrastructure: the oracle is the checker / the baseline, never the measured path)
# ------------------------------------------------------------------------------------------------------------------------------
def parity_sequence(model_path, width, height, seq):
    """The metric's "mask IoU vs CPU ref" on a small sample.  `seq` (measure(): parity_run) holds, for the first k streams of the measured job, the frames of S
    consecutive steps FROM A RESET CONTEXT and what the GPU produced at every one of them; the oracle runs the same sequence from its own zero state
    (lib/libbackscrub.cc:330,339,355: the IIR carries three frames of history), so outline pixels are compared while they still hold 0xE0 / 0xFC transients."""
    import numpy as np
    from oracle import oracle_py
    frames, masks, outs, bgs = seq["frames"], seq["masks"], seq["out"], seq["bg"]
    S, k = len(frames), len(frames[0])
    # animated background through the product's source: the oracle resizes the same decoded picture itself (grab_background, app/background.cc:186) and composites over
    # THAT; the picture the GPU handed out must be the same bytes
    bg_steps, bg_source_identical = None, None
    if seq.get("bg_steps") is not None:
        bg_steps = [oracle_py.resize_linear(seq["bg_decoded"][c], width, height) for c in seq["bg_pictures"]]
        bg_source_identical = all(np.array_equal(a_, b_) for a_, b_ in zip(bg_steps, seq["bg_steps"]))

    def one_stream(i):
        ious, max_abs, differing, fg, transient = [], 0, 0, 0.0, 0
        ctx = oracle_py.Ctx(model_path, width, height)
        bg = bgs[i] if bgs.ndim == 4 else bgs
        for t in range(S):
            if bg_steps is not None:
                bg = bg_steps[t]
            want = ctx.process(frames[t][i])
            fa, fb = masks[t][i] < 128, want < 128
            union = np.logical_or(fa, fb).sum()
            ious.append(1.0 if union == 0 else float(np.logical_and(fa, fb).sum() / union))
            comp = oracle_py.alpha_blend(bg, frames[t][i], want)
            d = np.abs(comp.astype(np.int16) - outs[t][i].astype(np.int16))
            max_abs = max(max_abs, int(d.max()))
            differing += int((d > 1).any(axis=-1).sum())
            if t == S - 1:
                fg = float(fb.mean())
                transient = int(((want > 0) & (want < 255)).sum())
        ctx.close()
        return ious, max_abs, differing, fg, transient

    from concurrent.futures import ThreadPoolExecutor          # one oracle context per stream, the C calls release the GIL (DeepLab: ~1.5 s per frame)
    with ThreadPoolExecutor(max_workers=k) as ex:
        per = list(ex.map(one_stream, range(k)))
    ious = [v for p_ in per for v in p_[0]]
    max_abs, differing = max(p_[1] for p_ in per), sum(p_[2] for p_ in per)
    fg, transient = [p_[3] for p_ in per], sum(p_[4] for p_ in per)
    out = {"streams": k, "steps": S, "mask_iou_min": round(min(ious), 6), "composite_max_abs_diff": max_abs,
           "composite_pixels_off_by_more_than_1": differing, "pixels": k * S * width * height,
           "oracle_person_fraction": [round(v, 4) for v in fg], "oracle_mask_pixels_between_0_and_255_last_step": transient}
    if seq.get("need_person") and max(fg) < 0.05:
        out["warning"] = "oracle masks contain no person: IoU is vacuous"
    if bg_source_identical is not None:
        out["background_pictures"] = [int(c) for c in seq["bg_pictures"]]
        out["background_identical_to_oracle_resize_of_the_same_decoded_picture"] = bool(bg_source_identical)
    return out


def usable_cpus():
    """How many CPUs this process can really run on: the scheduler affinity mask AND the cgroup CPU quota (cpu.max / cfs_quota_us) — a container on a
    256-thread host is often given a fraction of it, while os.cpu_count() still says 256 (round 3's all-core leg: 7.6x of one thread on "256 threads")."""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except (AttributeError, OSError):
        pass
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = float(q) / float(per)
    except (OSError, ValueError):
        try:
            q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                quota = q / per
        except (OSError, ValueError):
            pass
    return n, quota


def cpu_baseline(model_path, width, height, target_s, short=False):
    """Time the CPU oracle port on a bounded sample: a thread sweep 1, 2 (the reference's default `threads`, app/deepseg.cc:362), then doubling up to the CPUs
    this process can use (usable_cpus: affinity and cgroup quota, not os.cpu_count()); `value` = the best leg, `cores` = its thread count.  short=True (the
    configurations other than the headline): only 1, 2 and the quota.  The port parallelises with OpenMP ACROSS streams (one stream — one context, created and
    first-touched by the thread that runs it — per thread); the reference's threads are TFLite intra-op threads of ONE stream — a scalar port has no intra-op
    parallelism, so the t-thread leg is the throughput of t cores running t streams."""
    from backscrub_amd import synth
    from oracle import oracle_py
    logical = os.cpu_count() or 1
    affinity, quota = usable_cpus()
    top = affinity if quota is None else max(1, min(affinity, int(quota + 0.5)))
    bg = synth.background(width, height)
    scenes = synth.frames(4, width, height)

    def leg(threads, budget_s):
        frames = scenes[[i % 4 for i in range(threads)]]
        sec, _, _ = oracle_py.baseline_run(model_path, frames, bg, 1, threads)     # warm-up (page faults, thread pool) = calibration
        iters = int(max(2, min(200, budget_s / max(sec, 1e-3))))
        sec, stages, _ = oracle_py.baseline_run(model_path, frames, bg, iters, threads)
        return threads * iters / sec, iters, sec, stages

    counts = sorted({1, min(2, top), top} | (set() if short else {t for t in (4, 8, 16, 32, 64, 128, 256) if t < top}))
    if affinity > top and not short:
        counts.append(affinity)              # one leg beyond the quota, to show that it is the quota (not the port) that caps the scaling
    legs, best = [], None
    share = target_s / (len(counts) + 1.0)
    for t in counts:
        fps, iters, sec, stages = leg(t, max(0.5, share * (2.0 if t == top else 1.0)))
        legs.append({"threads": t, "value": round(fps, 2), "unit": "frames/s", "fps_per_thread": round(fps / t, 2),
                     "sample": "%d stream(s) x %d frames, %.1f s" % (t, iters, sec)})
        if best is None or fps > best[0]:
            best = (fps, t, iters, sec, stages)
    fps, t, iters, sec, stages = best
    tot = sum(stages) or 1.0
    return {"value": round(fps, 2), "unit": "frames/s", "cores": t, "kind": "port",
            "sample": "%d streams x %d frames of %dx%d through oracle/libbs_oracle_fast.so (-O3 -mavx2 -mfma, OpenMP over streams, one context per thread), %.1f s; "
                      "best of the thread sweep in `legs`" % (t, iters, width, height, sec),
            "host": {**cpu_description(), "affinity_cpus": affinity, "cgroup_cpu_quota": quota, "logical_cpus": logical},
            "legs": legs,
            "stage_share": {k: round(v / tot, 3) for k, v in zip(("prep", "infer", "mask", "blend"), stages)}}


# ------------------------------------------------------------------------------------------------------------------------------
# roofline accounting
# ------------------------------------------------------------------------------------------------------------------------------
def load_pmc(B, W, H, model_name):
    """HBM-traffic counters of this workload from the COMMITTED rocprofv3 passes (profiles/pmc_latest.json: one entry per workload,
    tools/profile_config.sh) — not measured in this run; the detail record says so in `traffic_source`."""
    try:
        pj = json.load(open(os.path.join(ROOT, "profiles", "pmc_latest.json")))
        for e in pj.get("workloads", [pj]):
            wl = e.get("workload", {})
            if (wl.get("batch"), wl.get("width"), wl.get("height"), wl.get("model")) == (B, W, H, model_name):
                e = dict(e)
                e["csrc_digest"] = pj.get("csrc_digest")          # the kernel sources the passes were collected on (tools/merge_pmc.py)
                return e
    except Exception:
        pass
    return {}


def traffic_of(pmc, launch_index, n_launches, name):
    """(2 * FETCH_SIZE + WRITE_SIZE) KiB of one launch: by position in the step when the profiled step has the same number of launches
    (layers that share a kernel instantiation — DeepLab's GEMMs — keep their own figure), else by kernel name."""
    seq = []
    for e in pmc.get("step_launches") or []:              # the fused mask + blend launch is two dispatches when the ROI does not cover the frame
        last = seq[-1]["kernel"].split(" + ")[-1] if seq else ""
        # ... and the tile classifier in front of it, and (last tile row partial) two instantiations of the tile kernel: all ONE launch of the step (launch_mask_blend)
        if seq and (last.startswith("outside_roi") or last.endswith("tile_class_k") or (last.startswith("mask_tile_k") and e["kernel"].startswith("mask_tile_k"))):
            seq[-1] = {"kernel": seq[-1]["kernel"] + " + " + e["kernel"], "FETCH_SIZE_KiB": seq[-1]["FETCH_SIZE_KiB"] + e["FETCH_SIZE_KiB"],
                       "WRITE_SIZE_KiB": seq[-1]["WRITE_SIZE_KiB"] + e["WRITE_SIZE_KiB"]}
        else:
            seq.append(dict(e))
    k = None
    if len(seq) == n_launches and 0 <= launch_index < n_launches:
        k = seq[launch_index]
    else:
        wants = PMC_NAMES.get(name, ())
        wants = (wants,) if isinstance(wants, str) else wants          # the specialised (hipRTC) and the interpreted program are different kernels
        kern = pmc.get("kernels", {})
        for want in wants:                                    # every instantiation of the kernel the launch dispatches (the mask tiles of a frame whose last tile row is partial
            hit = [(n_, v) for n_, v in kern.items() if n_ == want or n_.startswith(want)]      # run as two instantiations, each once per step): their sum
            if hit:
                k = {"kernel": " + ".join(n_ for n_, _ in hit), "FETCH_SIZE_KiB": sum(v.get("FETCH_SIZE_KiB", 0.0) for _, v in hit),
                     "WRITE_SIZE_KiB": sum(v.get("WRITE_SIZE_KiB", 0.0) for _, v in hit)}
                break
    if k and "FETCH_SIZE_KiB" in k and "WRITE_SIZE_KiB" in k:
        return int((2 * k["FETCH_SIZE_KiB"] + k["WRITE_SIZE_KiB"]) * 1024), k.get("kernel")
    return None, None


GENERAL_TILE_BPP = 10.0    # fused mask + blend, general tile: background 3 + frame 3 read, composite 3 + mask 1 written
UNIFORM_TILE_BPP = 7.0     # tile whose model-resolution block is uniformly 0 / 255: ONE operand 3 read, composite 3 + mask 1 written


def apply_event_overhead(stats, extra, ms_per_step):
    """hipEvent figures of the instrumented pass → durations inside the un-instrumented step: the excess of their sum over the measured step is the cost of
    the L events, removed from every launch in equal parts (an event costs the same behind a 6 us and behind a 100 us launch).  Never adds time; a launch keeps
    at least half of its event figure.  Returns what was done, for the detail record."""
    L = len(stats)
    total = sum(s["avg_ms"] for s in stats)
    per = max(0.0, total - ms_per_step) / L if L else 0.0
    for s in stats + extra:
        s["avg_ms_events"] = s["avg_ms"]
        s["avg_ms"] = max(s["avg_ms"] - per, 0.5 * s["avg_ms"])
    return {"launches": L, "sum_of_event_ms": round(total, 4), "ms_per_step": round(ms_per_step, 4), "removed_per_launch_us": round(per * 1e3, 3),
            "sum_after_ms": round(sum(s["avg_ms"] for s in stats), 4)}


def hbm_bytes_of(s):
    """bytes of one launch that must cross HBM: its algorithmic bytes for this input minus the reads of cache-resident data every stream shares
    (ONE background image for all B streams: 0.9 MB at VGA — L2 / MALL hits by construction)"""
    return float(s["bytes"]) - float(s.get("shared_bytes") or 0.0)


def roofline_of(s, pmc, model_name, launch_index=-1, n_launches=0):
    """One definition for every launch: achieved = HBM-side bytes (hbm_bytes_of) — or useful flops — of the launch / its mean hipEvent duration; frac =
    achieved / peak.  traffic = HBM bytes per launch from the committed rocprofv3 PMC passes: (2*FETCH_SIZE + WRITE_SIZE) KiB — FETCH_SIZE doubled per
    MI355X_MICROARCH.md §HBM (gfx950 counts 128-B reads at 64 B); `frac_counted_traffic` = those bytes over the same duration.  The wall is chosen against the
    pipe the kernel ISSUES on (pipe_of): a launch is "mfma"-bound only if its arithmetic intensity exceeds that pipe's ridge.  Figures that are NOT bandwidths —
    the same launch priced with the cache-resident reads included, or at SURVEY 8(d)'s dense 10 B/px — carry their own names and never a `frac`."""
    traffic, kern = traffic_of(pmc, launch_index, n_launches, s["name"]) if pmc else (None, None)
    src = {}
    if traffic is not None:
        stale = pmc.get("csrc_digest") != csrc_digest()
        src = {"traffic_source": "committed rocprofv3 --pmc passes (profiles/pmc_latest.json, round %s), not measured in this run" % pmc.get("round", "?"),
               "traffic_stale": bool(stale)}
        if stale:
            src["traffic_stale_note"] = "backscrub_amd/csrc changed since the passes were collected (digest %s then, %s now)" % (pmc.get("csrc_digest"), csrc_digest())
    if kern:
        src["traffic_kernel"] = kern
    sec = s["avg_ms"] * 1e-3
    pipe, peak_tf = pipe_of(model_name, s["name"])
    hbm = hbm_bytes_of(s)
    counted = {"frac_counted_traffic": round(traffic / sec / 1e9 / HBM_PEAK_GBS, 4)} if traffic and sec > 0 else {}
    if s["flops"] > 0 and s["flops"] / max(hbm, 1) > peak_tf * 1e12 / (HBM_PEAK_GBS * 1e9):
        a = s["flops"] / sec / 1e12
        return {"kernel": s["name"], "bound": "mfma", "pipe": pipe, "achieved": round(a, 3), "peak": peak_tf, "unit": "TFLOP/s", "frac": round(a / peak_tf, 4),
                "traffic": traffic, **src, **counted, "avg_ms": round(s["avg_ms"], 4), "algorithmic_flops_per_launch": int(s["flops"]),
                "hbm_bytes_per_launch": int(hbm)}
    a = hbm / sec / 1e9 if sec > 0 else 0.0
    out = {"kernel": s["name"], "bound": "hbm", "achieved": round(a, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(a / HBM_PEAK_GBS, 4),
           "traffic": traffic, **src, **counted, "avg_ms": round(s["avg_ms"], 4), "hbm_bytes_per_launch": int(hbm)}
    if s.get("shared_bytes"):
        out.update({"cache_resident_bytes_per_launch": int(s["shared_bytes"]), "incl_cache_resident_GBps": round(s["bytes"] / sec / 1e9, 1)})
    if "bytes_dense" in s:           # the data-dependent fused mask + blend (measure()): SURVEY §8(d)'s dense figure beside what the launch had to move for this input
        out.update({"tiles": s["tiles"], "dense_10Bpx_bytes_per_launch": int(s["bytes_dense"]), "dense_10Bpx_GBps": round(s["bytes_dense"] / sec / 1e9, 1)})
    if s["flops"] > 0:
        fl = s["flops"] / sec / 1e12
        out.update({"algorithmic_flops_per_launch": int(s["flops"]), "flops_pipe": pipe, "flops_frac_of_pipe": round(fl / peak_tf, 4),
                    "intensity_flop_per_byte": round(s["flops"] / max(hbm, 1), 1), "ridge_flop_per_byte": round(peak_tf * 1e12 / (HBM_PEAK_GBS * 1e9), 1)})
    return out


def finish_counters(coll, frames, elapsed, checksum):
    """The job's one reduction, shared by measure() and the CPU self-test: {frames Σ, elapsed max, checksum Σ} + every rank's own rate.  coll=None = THIS RANK ALONE
    (N = 1, or rank 0's solo reference run while the other ranks wait at a barrier): nothing collective may be touched then — an all-reduce entered by one rank
    only would pair up with the waiting ranks' barrier (round 4, found by `bench.py --gpus 2` on one GPU: it hung)."""
    if coll is None:
        return float(frames), float(elapsed), int(checksum) % (1 << 40), [frames / elapsed]
    total, max_elapsed, checksum_all = coll.reduce(frames, elapsed, checksum)
    return total, max_elapsed, checksum_all, coll.gather(frames / elapsed)


def solo_reference(coll, rank, fn):
    """rank 0 runs fn() ALONE — fn must not touch the collective (coll=None inside) — while the other ranks wait; → fn()'s value on rank 0, None elsewhere"""
    v = fn() if rank == 0 else None
    coll.barrier()
    return v


DUMP_BYTES = 60_000_000    # --dump-outputs: bytes of array data in all (under 64 MB with the .npy headers)


def dump_step_outputs(out_dir, d_out, d_masks):
    """--dump-outputs: the composites [B,H,W,3] and masks [B,H,W] of one step as float32 DIR/composite.npy, DIR/mask.npy.  A batch larger than DUMP_BYTES is
    cut to whole streams picked by a fixed seed (sorted), or — when one stream alone is too large — to pixels picked the same way: the same sample every run."""
    import numpy as np
    import torch
    B, H, W = d_masks.shape
    cap = DUMP_BYTES // (4 * (3 + 1))                            # pixels whose composite (3 x f32) and mask (f32) fit
    rng = np.random.default_rng(0xD5)
    comp, mask = d_out[:B], d_masks
    if B * H * W > cap and H * W <= cap:
        sel = torch.from_numpy(np.sort(rng.choice(B, cap // (H * W), replace=False))).to(d_out.device)
        comp, mask = comp.index_select(0, sel), mask.index_select(0, sel)
    elif B * H * W > cap:
        sel = torch.from_numpy(np.sort(rng.choice(B * H * W, cap, replace=False))).to(d_out.device)
        comp, mask = comp.reshape(-1, 3).index_select(0, sel), mask.reshape(-1).index_select(0, sel)
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "composite.npy"), comp.cpu().numpy().astype(np.float32))
    np.save(os.path.join(out_dir, "mask.npy"), mask.cpu().numpy().astype(np.float32))


# ------------------------------------------------------------------------------------------------------------------------------
# one measured configuration
# ------------------------------------------------------------------------------------------------------------------------------
def scene_ring(base, B, T, W, seed):
    """[T][B,H,W,3] device-resident camera batches from `base` [D,H,W,3] (D noise-free scenes): time step t shifts the scene sideways by the sway of
    synth.frame (1 % of the width x sin 0.7 t, whole pixels) and redraws +-6 uniform sensor noise — so outline pixels change class from step to step and the
    temporal filter carries 0xE0 / 0xFC transients, as with a camera.  Stream i carries scene i mod D (its twins share every byte: the full-batch check relies on it).
    Made on the GPU (an HD scene takes 0.4 s to render on the host); the parity leg downloads the very bytes it checks."""
    import torch
    D = base.shape[0]
    g = torch.Generator(device="cuda")
    g.manual_seed(0xB5C0 + seed)
    ring = []
    for t in range(T):
        dx = int(round(0.01 * W * math.sin(0.7 * t)))
        fr = torch.roll(base, shifts=dx, dims=2).to(torch.int16)
        fr += torch.randint(-6, 7, fr.shape, generator=g, device="cuda", dtype=torch.int16)
        fr = fr.clamp_(0, 255).to(torch.uint8)
        ring.append(fr.repeat((B + D - 1) // D, 1, 1, 1)[:B].contiguous())
    return ring


def measure(model_key, W, H, B, steps, warmup, rank, world, local_rank, per_stream_bg=False, bg_ring=False, bg_source="", profile_iters=8, dump_launches="", ramp_s=0.0, coll=None,
            profile=True, moving=True, static_leg=False, parity_streams=2, parity_steps=0, dump_outputs=""):
    """Run one configuration on this rank's GPU.  Returns a dict with the timed result and (rank 0) the per-launch profile and
    the samples the parity leg needs.  `coll` (backscrub_amd.dist.Collective) carries the barriers around the timed region and the one
    reduction of the job; None = this rank alone (N = 1, and rank 0's solo reference run at N > 1)."""
    import numpy as np
    import torch

    import backscrub_amd
    from backscrub_amd import synth

    model_path, model_name, weights = resolve_model(model_key)
    mg = backscrub_amd.MaskGen(model_path, W, H, n_streams=B, device=local_rank)
    # synthetic, device-resident inputs: each GPU owns its own B streams (scenes seeded by rank); at 640x480 the first two
    # streams carry the two REAL webcam frames of tests/golden/photo_2x640x480.png so that the parity sample has a real person
    distinct = 16
    host = np.stack([synth.frame(W, H, s + 16 * rank, 0, noise=0) for s in range(distinct)])
    photo = False
    if (W, H) == (640, 480):
        try:
            from tools import make_photo_fixture
            host[:2] = make_photo_fixture.load_frames()
            photo = True
        except Exception:
            pass
    T = RING if moving else 1
    ring = scene_ring(torch.from_numpy(host).cuda(), B, T, W, seed=rank)
    bg_host = synth.background(W, H, seed=1 + rank)
    d_bg = torch.from_numpy(bg_host).cuda()
    if per_stream_bg:      # [B,H,W,3]: one background frame per stream, no two streams share a byte (random bytes: nothing of it can come out of a cache)
        g = torch.Generator(device="cuda")
        g.manual_seed(77 + rank)
        d_bg = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8, device="cuda")
    d_out = torch.empty_like(ring[0])
    bring = None
    if bg_ring:
        # animated background (configs[3]): the reference decodes the video on a host thread (app/background.cc:29-104) and
        # grab_background() resizes the current frame to the camera size EVERY frame (:186).  webm cannot be decoded in this image:
        # the decode is emulated by a ring of 36 pre-decoded 480x360 frames (the size of backgrounds/animated.gif) in PINNED host
        # memory; per step: H2D of the next frame + bsx_resize_bgr on the GPU, both inside the timed region.
        bring = torch.from_numpy(np.stack([synth.background(480, 360, seed=100 + i) for i in range(36)])).pin_memory()
        d_small = torch.empty((1, 360, 480, 3), dtype=torch.uint8, device="cuda")

    bgsrc = d_anim = None
    if bg_source:
        # the product's OWN background source (csrc/media.cpp + live.cpp = app/background.cc:29-104,126-194): the file is decoded when it is loaded (in-tree GIF / PNG /
        # JPEG decoders), its pictures live on the GPU, and bsx_background_grab() — grab_background() — hands out the picture the playback clock points at, resized to
        # the camera size, every step.  Timed inside the step like the reference's per-frame cv::resize (:186).
        bgsrc = backscrub_amd.Background(mg, path=bg_source)
        d_anim = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")

    def one_step(t, frames=None):
        fr = ring[t % T] if frames is None else frames
        if bgsrc is not None:
            bgsrc.grab(W, H, out=d_anim)
            mg.step(fr, d_anim, d_out)
        elif bring is not None:
            d_small[0].copy_(bring[t % 36], non_blocking=True)
            bg = mg.resize_bgr(d_small, W, H)[0]
            mg.step(fr, bg, d_out)
        else:
            mg.step(fr, d_bg, d_out)

    def barrier():
        torch.cuda.synchronize()
        if coll is not None:
            coll.barrier()

    if ramp_s > 0:                        # clock ramp (untimed, before the W warmup steps): sustained work until the GPU is out of its idle state
        t_r = time.perf_counter()
        while time.perf_counter() - t_r < ramp_s:
            for t in range(8):
                one_step(t)
            torch.cuda.synchronize()
    for t in range(warmup):
        one_step(t)
    barrier()
    t0 = time.perf_counter()
    for t in range(steps):
        one_step(warmup + t)
    barrier()
    elapsed = time.perf_counter() - t0

    checksum = int(d_out[:, ::16, ::16].to(torch.int64).sum().item())
    total_frames, max_elapsed, checksum_all, rank_fps = finish_counters(coll, B * steps, elapsed, checksum)     # the only collective of the job
    if dump_outputs and rank == 0:        # the last timed step's results, before anything below steps the context again
        dump_step_outputs(dump_outputs, d_out, mg.masks()[:B])
    res = {"model_path": model_path, "model_name": model_name, "weights": weights, "B": B, "W": W, "H": H, "photo": photo, "ring": T,
           "fps": total_frames / max_elapsed, "ms_per_step": 1e3 * max_elapsed / steps, "checksum": checksum_all, "mg": mg, "rank_fps": rank_fps,
           "frames_ring": ring, "d_bg": d_bg, "d_out": d_out, "bg_host": bg_host, "steps": steps, "warmup": warmup}
    if bgsrc is not None:
        res["background_source"] = {"file": os.path.basename(bg_source), "pictures": bgsrc.n_frames, "size": "%dx%d" % (bgsrc.width, bgsrc.height), "fps": bgsrc.fps,
                                    "animated": bgsrc.video, "what": "bsx_background_load + bsx_background_grab per step (decoded once at load, pictures resident on the GPU, "
                                                                     "clock-indexed playback + GPU resize to the camera size inside the timed step)"}
    if bgsrc is not None:
        res["bgsrc"] = bgsrc
    if rank == 0 and profile:
        last_t = warmup + steps - 1
        # EVERY stream of the batch, on the GPU: streams i and i + 16 carry the same scene (and, shared background, the same temporal history), so their
        # masks and composites must be identical bytes whatever tile / workgroup / XCD they ran on; the first streams are then held to the oracle (parity_sequence)
        if per_stream_bg:
            res["full_batch"] = None
        else:
            if bring is not None or bgsrc is not None:                # twins need ONE known background: one more step over the still image
                mg.step(ring[(last_t + 1) % T], d_bg, d_out)
                last_t += 1
                torch.cuda.synchronize()
            groups_ok = 0
            n_groups = B // distinct
            masks_all = mg.masks()[:B]
            for gi in range(1, n_groups):
                if torch.equal(d_out[gi * distinct:(gi + 1) * distinct], d_out[:distinct]) and torch.equal(masks_all[gi * distinct:(gi + 1) * distinct], masks_all[:distinct]):
                    groups_ok += 1
            res["full_batch"] = {"streams": B, "distinct_scenes": distinct, "groups_compared_with_group_0": max(n_groups - 1, 0), "groups_identical": groups_ok,
                                 "all_identical": groups_ok == max(n_groups - 1, 0)}
        # per-launch hipEvent times (bsx_profile_batch, one pass per call) over the NEXT batches of the ring, so that the data-dependent launch is timed on the
        # moving scene's tile mix; its tile classification is read after every pass
        acc, tiles_acc, P = None, {}, max(profile_iters, T)
        for p in range(P):
            st = mg.profile(ring[(last_t + 1 + p) % T], d_bg, d_out, iters=1)
            if acc is None:
                acc = st
            else:
                for a_, b_ in zip(acc, st):
                    a_["avg_ms"] += b_["avg_ms"]
            try:
                ts = mg.mask_tile_stats(B)
                for k_ in ("tiles", "uniform_255", "uniform_0", "general"):
                    tiles_acc[k_] = tiles_acc.get(k_, 0) + ts[k_]
            except Exception:  # noqa: BLE001 — accounting only
                tiles_acc = None
        stats = acc
        for s in stats:
            s["avg_ms"] /= P
        last_t += P
        # The fused mask + blend launch is data dependent since round 4: a tile whose whole model-resolution source block is 0xFF / 0x00 (the temporal filter's steady
        # state away from the person's outline) skips the mask phases and reads only the operand its composite is a copy of.  Its algorithmic bytes are therefore
        # stated for THIS input: per ROI pixel 10 B on a general tile (background 3 + frame 3 read, composite 3 + mask 1 written; the model-resolution source block is
        # the separate in_roi_px term), 7 B on a uniform one (one operand is not read); 6 B outside the ROI (background copied).  `bytes_dense` keeps SURVEY §8(d)'s
        # 10 B/px figure.  (Rounds 4-5 charged a general tile 11 B: VERDICT r5 weak #2.)
        ts = None
        if tiles_acc:
            ts = {k_: v / P for k_, v in tiles_acc.items()}
            ts["tile"] = "128x32"
            i_ = mg.info
            roi_px, in_roi_px = i_["roi"][2] * i_["roi"][3], i_["in_roi"][2] * i_["in_roi"][3]
            f_uni = (ts["uniform_255"] + ts["uniform_0"]) / max(ts["tiles"], 1)
            aware = B * (in_roi_px + 6.0 * (W * H - roi_px) + roi_px * (GENERAL_TILE_BPP * (1.0 - f_uni) + UNIFORM_TILE_BPP * f_uni))
            res["mask_tiles"] = {**{k_: round(ts[k_], 1) for k_ in ("tiles", "uniform_255", "uniform_0", "general")}, "tile": "128x32", "uniform_fraction": round(f_uni, 4)}
            for s in stats:
                if s["name"] == "mask_blend":
                    s["bytes_dense"] = s["bytes"]
                    s["bytes"] = aware
                    s["tiles"] = res["mask_tiles"]
        # ONE background image shared by all B streams (0.9 MB at VGA) is cache-resident by construction: its reads are algorithmic bytes (10 B/px)
        # but cannot be HBM traffic — hbm_bytes_of() leaves them out of every bandwidth.
        if not per_stream_bg:
            i_ = mg.info
            roi_px = i_["roi"][2] * i_["roi"][3]
            f_bg = (ts["general"] + ts["uniform_255"]) / max(ts["tiles"], 1) if ts else 1.0      # tiles that read the background at all
            for s in stats:
                if s["name"] == "mask_blend":
                    s["shared_bytes"] = B * 3.0 * ((W * H - roi_px) + roi_px * f_bg)
                elif s["name"].startswith("blend"):
                    s["shared_bytes"] = B * 3.0 * W * H
        extra = [s for s in stats if s["name"].endswith("(standalone)")]   # measured for its roofline line, not part of the step
        stats = [s for s in stats if not s["name"].endswith("(standalone)") and "(inside the launch before)" not in s["name"]]   # fused-away steps launch nothing
        # The instrumented pass carries one hipEvent per launch; the un-instrumented step was just timed (ms_per_step).  What the events add is taken off every
        # launch in equal parts, so that sum(launches) == ms_per_step and every `frac` below is priced on the duration the launch has INSIDE the step
        # (round 5's bracketing pairs summed to 0.3908 ms against a 0.3506 ms step).  The raw event figure stays in `avg_ms_events`.
        res["event_overhead"] = apply_event_overhead(stats, extra, res["ms_per_step"])
        for s in stats + extra:
            s["GBps"] = hbm_bytes_of(s) / (s["avg_ms"] * 1e-3) / 1e9 if s["avg_ms"] > 0 else 0.0
        if dump_launches:
            with open(dump_launches, "w") as f:
                f.write(mg.plan())
                for i, s in enumerate(stats):
                    f.write("%3d %-22s %8.2f us %9.1f GB/s %8.2f GFLOP/s\n" % (i, s["name"], s["avg_ms"] * 1e3, s["GBps"], s["flops"] / max(s["avg_ms"], 1e-9) / 1e6))
        groups = {"prep": 0.0, "network": 0.0, "decode": 0.0, "mask": 0.0, "blend": 0.0}
        for s in stats:
            groups[IMAGE_LAUNCHES.get(s["name"], "network")] += s["avg_ms"]
        net = [s for s in stats if s["name"] not in IMAGE_LAUNCHES]
        res.update(stats=stats, extra=extra, groups=groups, net=net, net_ms=sum(s["avg_ms"] for s in net), net_flops=sum(s["flops"] for s in net),
                   net_launches=len(net))
        # the SAME batch every step (rounds 1-4's protocol), in the same context, beside the moving scene: the temporal filter then settles on pure 0x00 / 0xFF
        # and the uniform-tile shortcut takes its best case
        if static_leg and moving and coll is None:
            n_st = max(20, min(steps, 100))
            for t in range(4):
                one_step(t, ring[0])
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for t in range(n_st):
                one_step(t, ring[0])
            torch.cuda.synchronize()
            dt = time.perf_counter() - t1
            st = {"value": round(B * n_st / dt, 1), "unit": "frames/s", "ms_per_step": round(1e3 * dt / n_st, 4), "steps": n_st}
            try:
                ts_ = mg.mask_tile_stats(B)
                st["uniform_fraction"] = round((ts_["uniform_255"] + ts_["uniform_0"]) / max(ts_["tiles"], 1), 4)
            except Exception:  # noqa: BLE001
                pass
            res["static_scene"] = st
        # parity sample: reset, then RING + 3 consecutive steps of the first streams, every step's mask and composite kept for the oracle (parity_sequence)
        k = min(parity_streams, B)
        S = parity_steps or ((T + 3) if moving else 4)
        mg.reset()
        seq = {"frames": [], "masks": [], "out": [], "need_person": photo,
               "bg": (d_bg[:k] if per_stream_bg else d_bg).cpu().numpy()}
        if bgsrc is not None:
            # with the background source: every parity step composites over the picture the source handed out at that step; the oracle gets THE SAME DECODED picture
            # (the product's host decoder, byte-equal to Pillow in tests/test_media.py) and does its own cv::resize of it (oracle resize_linear = background.cc:186)
            seq["bg_steps"], seq["bg_pictures"] = [], []
            decoded, _fps = backscrub_amd.media_decode(bg_source)
            seq["bg_decoded"] = decoded
        for t in range(S):
            if bgsrc is not None:
                frm, _ = bgsrc.grab(W, H, out=d_anim)
                mg.step(ring[t % T], d_anim, d_out)
                torch.cuda.synchronize()
                seq["bg_steps"].append(d_anim.cpu().numpy())
                seq["bg_pictures"].append(frm - 1)
            else:
                mg.step(ring[t % T], d_bg, d_out)
            torch.cuda.synchronize()
            seq["frames"].append(ring[t % T][:k].cpu().numpy())
            seq["masks"].append(mg.masks()[:k].cpu().numpy())
            seq["out"].append(d_out[:k].cpu().numpy())
        res["parity_in"] = seq
    return res


def summarize(res, pmc):
    """→ the full JSON fragment of one measured configuration (rank 0); compact_config() cuts it down for the printed line."""
    stats, extra = res["stats"], res["extra"]
    dom = max(stats, key=lambda s: s["avg_ms"])
    blend = dict((extra or [s for s in stats if s["name"] in ("blend", "mask_blend")])[0], name="blend")
    n_l = len(stats)
    out = {"value": round(res["fps"], 1), "unit": "frames/s", "ms_per_step": round(res["ms_per_step"], 4), "steps": res["steps"], "warmup": res["warmup"],
           "scene": "moving (ring of %d batches)" % res["ring"] if res["ring"] > 1 else "static (the same batch every step)",
           "roofline": roofline_of(dom, pmc, res["model_name"], stats.index(dom), n_l), "roofline_blend": roofline_of(blend, pmc, res["model_name"])}
    if extra:
        out["roofline_blend"]["note"] = "bsx_composite_batch kernel timed stand-alone; inside the step the blend is fused with mask upscale+blur (mask_blend)"
    if res["net_launches"] > 1:              # the network launches together, against BOTH walls: useful flops over the pipe they issue on, and bytes over HBM
        ms = res["net_ms"] * 1e-3
        net_traffic = [traffic_of(pmc, i, n_l, s_["name"])[0] for i, s_ in enumerate(stats) if s_ in res["net"]] if pmc and len(pmc.get("step_launches") or []) else []
        traffic = int(sum(net_traffic)) if net_traffic and all(t is not None for t in net_traffic) else None
        # pipe time: every launch's flops at the peak of ITS pipe (DeepLab: GEMM launches on the split-f16 pipe, the rest f32)
        pipe_s = sum(s_["flops"] / (pipe_of(res["model_name"], s_["name"])[1] * 1e12) for s_ in res["net"])
        alg_bytes = sum(s_["bytes"] for s_ in res["net"])
        f_pipe = pipe_s / ms
        f_alg = alg_bytes / ms / 1e9 / HBM_PEAK_GBS
        f_cnt = traffic / ms / 1e9 / HBM_PEAK_GBS if traffic else None
        hbm_side = max(f_alg, f_cnt or 0.0)
        out["roofline_network"] = {"kernel": "network (%d launches)" % res["net_launches"], "bound": "hbm" if hbm_side >= f_pipe else "mfma",
                                   "frac": round(max(hbm_side, f_pipe), 4),
                                   "flops_TFLOPs": round(res["net_flops"] / ms / 1e12, 3), "frac_of_issuing_pipes": round(f_pipe, 4),
                                   "algorithmic_GBps": round(alg_bytes / ms / 1e9, 1), "frac_hbm_algorithmic": round(f_alg, 4),
                                   "counted_GBps": round(traffic / ms / 1e9, 1) if traffic else None, "frac_hbm_counted_traffic": round(f_cnt, 4) if f_cnt else None,
                                   "peak_hbm_GBps": HBM_PEAK_GBS, "traffic": traffic, "avg_ms": round(res["net_ms"], 4),
                                   "note": "frac_of_issuing_pipes = sum over launches of useful flops / the peak of the pipe that launch issues on (pipe_of), over the measured time"}
    for k_ in ("mask_tiles", "static_scene", "event_overhead", "background_source"):
        if res.get(k_) is not None:
            out[k_] = res[k_]
    if res.get("full_batch") is not None:
        out["full_batch_twin_streams"] = res["full_batch"]
    out["stage_ms"] = {k: round(v, 4) for k, v in res["groups"].items()}
    out["stage_ms"]["sum_of_launches"] = round(sum(s["avg_ms"] for s in stats), 4)
    out["top_launches"] = [{"name": s["name"], "ms": round(s["avg_ms"], 4), "GBps": round(s["GBps"], 1)} for s in sorted(stats, key=lambda s: -s["avg_ms"])[:8]]
    return out


def release(res):
    import torch
    if res.get("bgsrc") is not None:
        res["bgsrc"].close()
    res["mg"].close()
    for k in ("mg", "frames_ring", "d_bg", "d_out", "parity_in", "bgsrc"):
        res.pop(k, None)
    torch.cuda.empty_cache()


def single_stream_latency(model_key, W, H, calls):
    """The drop-in path an unchanged deepseg.cc would take: bs_maskgen_process → bsx_process_host (H2D of one frame, the whole
    mask pipeline for one stream, D2H of the mask, synchronous).  Context: the reference's README quotes ~10 FPS for DeepLab on two
    CPU cores (README.md:177) and the Meet model card ~120 FPS inference on a laptop CPU — neither measured here."""
    import numpy as np

    import backscrub_amd
    from backscrub_amd import synth
    path, name, _ = resolve_model(model_key)
    mg = backscrub_amd.MaskGen(path, W, H, n_streams=1)
    f = synth.frame(W, H, 0)
    mask = np.empty((H, W), np.uint8)
    for _ in range(5):
        mg.process_host(f, 0, mask)
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        mg.process_host(f, 0, mask)
        ts.append(1e3 * (time.perf_counter() - t0))
    mg.close()
    ts.sort()
    return {"network": name, "frame": "%dx%d" % (W, H), "calls": calls, "p50_ms": round(ts[len(ts) // 2], 3), "p99_ms": round(ts[min(len(ts) - 1, int(len(ts) * 0.99))], 3),
            "fps_at_p50": round(1e3 / ts[len(ts) // 2], 1)}


def multi_gpu_sections(coll, main, c4, solo1, solo4, world):
    """The N > 1 part of the record (rank 0): what RCCL really connected, the per-rank rates behind `value`, the north-star job's per-GPU slice
    (BASELINE configs[4]: 8192 x 1280x720 segm_full streams over 8 GPUs = 1024 per GPU, weak-scaled to N) and both against rank 0 running the
    same work ALONE on this box a moment earlier (the other ranks waiting at a barrier) — the driver computes its own efficiency from separate runs;
    this one is same-box, same-minute.  `main` / `c4`: {"fps", "ms_per_step", "rank_fps"}; solo*: frames/s or None."""
    def leg(r, solo, what):
        fps = r["rank_fps"]
        d = {"workload": what, "value": round(r["fps"], 1), "unit": "frames/s", "ms_per_step": round(r["ms_per_step"], 4),
             "per_rank_fps": [round(v, 1) for v in fps], "per_rank_fps_min": round(min(fps), 1), "per_rank_fps_max": round(max(fps), 1)}
        if solo:
            d["rank0_alone_fps"] = round(solo, 1)
            d["efficiency_vs_rank0_alone"] = round(r["fps"] / (world * solo), 4)
        return d
    out = {"collective": coll.describe(), "ranks_seen": coll.ranks_seen,
           "configs1": leg(main, solo1, "BASELINE configs[1] per GPU: %d x %dx%d, %s" % (main["B"], main["W"], main["H"], main["model_name"]))}
    if c4 is not None:
        out["configs4"] = leg(c4, solo4, "BASELINE configs[4]: %d x %dx%d %s streams sharded as contiguous blocks of %d per GPU over %d GPU(s), no data-path collective"
                              % (c4["B"] * world, c4["W"], c4["H"], c4["model_name"], c4["B"], world))
        out["configs4"]["streams_total"] = c4["B"] * world
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# the printed line
# ------------------------------------------------------------------------------------------------------------------------------
def _pick(d, keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d and d[k] is not None}


def _short_model(name):
    return {v: k for k, v in NAMES.items()}.get(name, name)


def compact_roofline(r):
    """the task statement's roofline object {bound, achieved, peak, unit, frac, traffic} + the launch it is about, its hipEvent duration, the counted-traffic
    fraction and (the data-dependent fused launch) the dense 10 B/px figure and the share of uniform tiles"""
    if not isinstance(r, dict) or "frac" not in r:
        return None
    out = _pick(r, ("kernel", "bound", "achieved", "peak", "unit", "frac"))
    out["traffic"] = r.get("traffic")
    out.update(_pick(r, ("avg_ms", "frac_counted_traffic", "traffic_stale", "dense_10Bpx_GBps")))
    if isinstance(r.get("tiles"), dict) and "uniform_fraction" in r["tiles"]:
        out["uniform_tiles"] = r["tiles"]["uniform_fraction"]
    return out


def compact_parity(p):
    if not isinstance(p, dict) or "mask_iou_min" not in p:
        return None
    out = {"iou_min": p["mask_iou_min"], "max_abs": p["composite_max_abs_diff"], "px_off_gt1": p["composite_pixels_off_by_more_than_1"], "streams": p["streams"], "steps": p.get("steps")}
    if "warning" in p:
        out["vacuous"] = True
    return out


def compact_cpu(c, full=False):
    """{value, cores} (+ the 1- and 2-thread legs; the headline also kind / unit / sample / host)"""
    if not isinstance(c, dict) or c.get("value") is None:
        return _pick(c, ("value", "cores", "kind", "unit", "sample")) if isinstance(c, dict) else None
    out = {"value": c["value"], "cores": c["cores"]}
    for leg in c.get("legs", []):
        if leg["threads"] in (1, 2):
            out["t%d" % leg["threads"]] = leg["value"]
    if full:
        h = c.get("host", {})
        out.update({"unit": c["unit"], "kind": c["kind"],
                    "sample": "oracle -O3 port, OpenMP over streams: %s; best of 1/2/.../quota threads" % c["sample"].split(" through ")[0],
                    "host": "%s, %s logical CPUs, cgroup quota %s" % (h.get("model"), h.get("logical_cpus"), h.get("cgroup_cpu_quota")),
                    "stage_share": c.get("stage_share")})
    return out


def compact_config(tag, frag):
    """one BASELINE configuration in the printed line: {baseline_config, value, ms_per_step, steps, frac (+ its kernel), iou_min, max_abs, cpu {value, cores}}"""
    if "error" in frag:
        return {"baseline_config": tag, "error": str(frag["error"])[:160]}
    out = {"baseline_config": tag}
    out.update(_pick(frag, ("net", "batch", "frame", "value", "ms_per_step", "steps")))
    r = frag.get("roofline")
    if isinstance(r, dict):
        out.update({"kernel": r.get("kernel"), "bound": r.get("bound"), "frac": r.get("frac"), "kernel_ms": r.get("avg_ms")})
        if r.get("frac_counted_traffic") is not None:
            out["frac_counted"] = r["frac_counted_traffic"]
    rn = frag.get("roofline_network")
    if isinstance(rn, dict):
        out["network"] = _pick(rn, ("bound", "frac", "avg_ms"))
    if isinstance(frag.get("static_scene"), dict):
        out["static_value"] = frag["static_scene"]["value"]
    if isinstance(frag.get("mask_tiles"), dict):
        out["uniform_tiles"] = frag["mask_tiles"].get("uniform_fraction")
    p = compact_parity(frag.get("parity_sample"))
    if p:
        out.update({"iou_min": p["iou_min"], "max_abs": p["max_abs"]})
    fb = frag.get("full_batch_twin_streams")
    if isinstance(fb, dict):
        out["twins_identical"] = fb["all_identical"]
    if isinstance(frag.get("background_source"), dict):
        out["bg"] = "%s via bsx_background_grab" % frag["background_source"]["file"]
        if isinstance(frag.get("parity_sample"), dict) and "background_identical_to_oracle_resize_of_the_same_decoded_picture" in frag["parity_sample"]:
            out["bg_identical"] = frag["parity_sample"]["background_identical_to_oracle_resize_of_the_same_decoded_picture"]
        if isinstance(frag.get("decode_elsewhere_h2d_ring"), dict) and "value" in frag["decode_elsewhere_h2d_ring"]:
            out["h2d_ring_value"] = frag["decode_elsewhere_h2d_ring"]["value"]
    c = compact_cpu(frag.get("cpu_baseline"))
    if c:
        out["cpu"] = c
    return out


def compact_line(d):
    """The ONE line the driver parses, cut from the full record `d` (which goes to bench_detail.json): contract keys, `roofline`, `cpu_baseline`, and a short
    entry per BASELINE configuration / opt-in mode.  No prose beyond `config.workload` and `cpu_baseline.sample`."""
    out = {k: d.get(k) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data")}
    out["config"] = d.get("config")
    out["env_set"] = d.get("env_set") or {}
    out["roofline"] = compact_roofline(d.get("roofline"))
    for k in ("roofline_blend", "roofline_blend_per_stream_bg"):
        r = compact_roofline(d.get(k))
        if r:
            out[k] = _pick(r, ("achieved", "frac", "avg_ms", "frac_counted_traffic"))
    rn = d.get("roofline_network")
    if isinstance(rn, dict):
        out["roofline_network"] = _pick(rn, ("bound", "frac", "avg_ms", "flops_TFLOPs", "frac_of_issuing_pipes", "frac_hbm_counted_traffic"))
    if d.get("stage_ms"):
        out["stage_ms"] = d["stage_ms"]
    if d.get("top_launches"):
        out["top_launches"] = [[t["name"], t["ms"], t["GBps"]] for t in d["top_launches"][:4]]
    c = d.get("cpu_baseline")
    if isinstance(c, dict):
        cc = compact_cpu(c, full=True) or {}
        p = compact_parity(c.get("parity_sample"))
        if p:
            cc["parity_sample"] = p
        out["cpu_baseline"] = cc
    fb = d.get("full_batch_twin_streams")
    if isinstance(fb, dict):
        out["twins_identical"] = fb["all_identical"]
    if isinstance(d.get("static_scene"), dict):
        out["static_scene"] = _pick(d["static_scene"], ("value", "ms_per_step", "steps", "uniform_fraction"))
    w = d.get("worst_case")
    if isinstance(w, dict):
        out["worst_case"] = w if "error" in w else {**_pick(w, ("value", "ms_per_step", "steps")), **_pick(w.get("roofline") or {}, ("frac", "avg_ms")),
                                                    **({"iou_min": w["parity_sample"]["mask_iou_min"], "max_abs": w["parity_sample"]["composite_max_abs_diff"]}
                                                       if isinstance(w.get("parity_sample"), dict) else {})}
    if d.get("configs"):
        out["configs"] = [compact_config(f.get("baseline_config"), f) for f in d["configs"]]
    modes = []
    for m in (d.get("gemm_modes") or []) + (d.get("act_modes") or []):
        e = _pick(m, ("env", "cfg", "value", "ms_per_step", "steps"))
        p = compact_parity(m.get("parity_sample"))
        if p:
            e.update({"iou_min": p["iou_min"], "max_abs": p["max_abs"], "within_1lsb": p["max_abs"] <= 1 and p["iou_min"] >= 0.999})
        if "error" in m:
            e["error"] = str(m["error"])[:100]
        modes.append(e)
    if modes:
        out["opt_in_modes"] = modes
    for k, keys in (("host_io", ("value", "ms_per_step", "steps")), ("host_io_yuyv", ("value", "ms_per_step", "steps")), ("yuyv_out", ("value", "bit_identical_to_step_then_bgr_to_yuyv")),
                    ("yuyv_in_out", ("value", "ms_per_step", "bit_identical_to_yuyv_to_bgr_then_step_yuyv")), ("bgblur_step", ("value", "speedup"))):
        if isinstance(d.get(k), dict):
            out[k] = _pick(d[k], keys)
    if isinstance(d.get("single_stream"), dict) and d["single_stream"].get("runs"):
        out["single_stream_p50_ms"] = {_short_model(r["network"]) + "/" + r["frame"]: r["p50_ms"] for r in d["single_stream"]["runs"]}
    # N > 1
    if d.get("collective"):
        out["collective"] = d["collective"]
        for k in ("configs1", "configs4"):
            if isinstance(d.get(k), dict):
                e = _pick(d[k], ("value", "ms_per_step", "per_rank_fps_min", "per_rank_fps_max", "rank0_alone_fps", "efficiency_vs_rank0_alone", "streams_total"))
                r = d[k].get("roofline")
                if isinstance(r, dict):
                    e["frac"] = r.get("frac")
                p = compact_parity(d[k].get("parity_sample"))
                if p:
                    e.update({"iou_min": p["iou_min"], "max_abs": p["max_abs"]})
                out[k] = e
        if d.get("gpu_sharing"):
            out["gpu_sharing"] = True
        s2 = d.get("second_device_check")
        if isinstance(s2, dict):
            out["second_device_check"] = _pick(s2, ("ran", "ok", "why"))
    out["detail"] = d.get("detail_file", "bench_detail.json")
    return out


def emit(detail, path=""):
    """write the full record, print the compact line (shrunk further, least important parts first, should it ever exceed LINE_LIMIT)"""
    targets = [path] if path else [os.path.join(ROOT, "bench_detail.json")]
    if not path and os.path.isdir(os.path.join(ROOT, "gpurun_out")):
        targets.append(os.path.join(ROOT, "gpurun_out", "bench_detail.json"))
    for t in targets:
        try:
            with open(t, "w") as f:
                json.dump(detail, f, indent=1)
        except OSError:
            pass
    line = compact_line(detail)
    s = json.dumps(line, separators=(",", ":"))
    for k in ("single_stream_p50_ms", "bgblur_step", "yuyv_out", "top_launches", "opt_in_modes", "roofline_blend", "stage_ms", "yuyv_in_out", "host_io_yuyv", "host_io", "roofline_network"):
        if len(s.encode()) <= LINE_LIMIT:
            break
        line.pop(k, None)
        s = json.dumps(line, separators=(",", ":"))
    print(s, flush=True)
    return s


# ------------------------------------------------------------------------------------------------------------------------------
def selftest_dist(args):
    """CPU plumbing check of the multi-process path (tests/test_dist_gloo.py): the same launch, rendezvous, Collective (gloo instead of RCCL),
    barriers, counter reduction, per-rank gather and JSON assembly (multi_gpu_sections) as the GPU run — the GPU work replaced by made-up timings."""
    from backscrub_amd.dist import Collective, bind_to_gpu_numa, shard_streams
    coll = Collective(gpu=False)
    world, rank = coll.world, coll.rank
    numa = bind_to_gpu_numa(None, dry_run=True)

    def fake(B, W, H, name, steps, ms, c):                # what measure() does around its timed region, with a rank-dependent made-up duration
        if c is not None:
            c.barrier()
        elapsed = steps * ms * 1e-3 * (1.0 + 0.25 * rank)
        if c is not None:
            c.barrier()
        frames, max_elapsed, checksum, rank_fps = finish_counters(c, B * steps, elapsed, 1000 + rank)
        return {"B": B, "W": W, "H": H, "model_name": name, "fps": frames / max_elapsed, "ms_per_step": 1e3 * max_elapsed / steps,
                "rank_fps": rank_fps, "frames": frames, "elapsed_max": max_elapsed, "checksum": checksum}
    a, b = shard_streams(args.batch * world, world, rank)
    n4 = max(3, args.steps // 4)
    # the same order of solo runs, barriers and collectives as main(): a plain run has the main leg alone
    solo1 = solo_reference(coll, rank, lambda: fake(b - a, args.width, args.height, NAMES["lite"], args.steps, 1.0, None)["fps"]) if world > 1 and args.full else None
    main = fake(b - a, args.width, args.height, NAMES["lite"], args.steps, 1.0, coll)
    solo4 = solo_reference(coll, rank, lambda: fake(1024, 1280, 720, NAMES["full"], n4, 4.0, None)["fps"]) if world > 1 and args.full else None
    c4 = fake(1024, 1280, 720, NAMES["full"], n4, 4.0, coll) if args.full else None
    line = None
    if rank == 0:
        line = {"metric": METRIC, "selftest": "dist", "value": main["fps"], "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                "ms_per_step": main["ms_per_step"], "higher_is_better": True, "scaling": "weak", "frames": main["frames"], "elapsed_max": main["elapsed_max"],
                "checksum": main["checksum"], "host": cpu_description(), "numa": numa}
        line.update(multi_gpu_sections(coll, main, c4, solo1, solo4, world))
    coll.close()
    if rank == 0:
        if args.full and not args.no_cpu_baseline:        # kept at world > 1 (rank 0, after the other ranks have left)
            try:
                path, _, _ = resolve_model(args.model)
                line["cpu_baseline"] = cpu_baseline(path, args.width, args.height, args.cpu_seconds, short=True)
            except Exception as e:  # noqa: BLE001
                line["cpu_baseline"] = {"value": None, "unit": "frames/s", "cores": os.cpu_count(), "kind": "port", "sample": "failed: %r" % (e,)}
        print(json.dumps(line), flush=True)


def second_device_check():
    """`bench.py --second-device-check` (a subprocess of rank 0 at N > 1, so that a fault cannot take the measurement down): the code path with device != 0 —
    per-device kernel attributes, hipRTC module load, hipGraph capture of the host path, every entry point's device guard — executed on real hardware the first
    time two devices are visible.  One context on the LAST visible device and one on device 0, same frames: masks, composites and the single-frame host path
    must be byte-identical, and the caller's current device must be untouched."""
    import numpy as np
    import torch

    import backscrub_amd
    from backscrub_amd import synth
    ndev = backscrub_amd.lib().bsx_device_count()
    if ndev < 2:
        print(json.dumps({"ran": False, "why": "%d visible device(s)" % ndev}))
        return
    out = {"ran": True, "devices": [0, ndev - 1], "models": {}}
    ok_all = True
    W, H, n = 640, 480, 4
    frames = np.stack([synth.frame(W, H, s, 0) for s in range(n)])
    bg = synth.background(W, H)
    torch.cuda.set_device(0)
    for key in ("lite", "deeplab"):
        path, name, _ = resolve_model(key)
        got = {}
        for dev in (0, ndev - 1):
            mg = backscrub_amd.MaskGen(path, W, H, n_streams=n, device=dev)
            with torch.cuda.device(dev):
                d = torch.from_numpy(frames).cuda()
                d_bg = torch.from_numpy(bg).cuda()
                o = torch.empty_like(d)
                for _ in range(3):
                    mg.step(d, d_bg, o)
                torch.cuda.synchronize()
                masks, comp = mg.masks().cpu().numpy(), o.cpu().numpy()
            restored = torch.cuda.current_device() == 0
            hm = np.empty((H, W), np.uint8)
            mg.reset()
            torch.cuda.synchronize(dev)
            for _ in range(3):
                mg.process_host(frames[1], 1, hm)          # the drop-in path (hipGraph capture + replay) on that device
            got[dev] = (masks, comp, hm.copy(), restored and torch.cuda.current_device() == 0)
            mg.close()
        a_, b_ = got[0], got[ndev - 1]
        res = {"masks_identical": bool(np.array_equal(a_[0], b_[0])), "composites_identical": bool(np.array_equal(a_[1], b_[1])),
               "host_path_identical": bool(np.array_equal(a_[2], b_[2])), "host_path_equals_batch_path": bool(np.array_equal(b_[2], b_[0][1])),
               "callers_device_restored": bool(a_[3] and b_[3]), "person_fraction": round(float((b_[0] < 128).mean()), 4)}
        ok_all = ok_all and all(v for k, v in res.items() if k != "person_fraction")
        out["models"][name] = res
    out["ok"] = ok_all
    print(json.dumps(out))


def run_second_device_check():
    import subprocess
    try:
        env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "LOCAL_WORLD_SIZE", "GROUP_RANK",
                                                                "TORCHELASTIC_RUN_ID", "ROLE_RANK", "ROLE_WORLD_SIZE")}
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--second-device-check"], env=env, capture_output=True, text=True, timeout=240)
        lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
        if p.returncode == 0 and lines:
            return json.loads(lines[-1])
        return {"ran": True, "ok": False, "returncode": p.returncode, "stderr_tail": p.stderr[-600:]}
    except Exception as e:  # noqa: BLE001
        return {"ran": True, "ok": False, "error": repr(e)}


def main():
    args = parse()
    if args.second_device_check:
        return second_device_check()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args)                                     # does not return
    if args.selftest_dist:
        return selftest_dist(args)
    import torch

    from backscrub_amd.dist import Collective, bind_to_gpu_numa

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        sys.exit("--gpus %d disagrees with WORLD_SIZE=%d" % (args.gpus, world))
    if not torch.cuda.is_available():
        sys.exit("bench.py needs a GPU (no CPU fallback exists)")
    n_dev = torch.cuda.device_count()
    shared = world > n_dev                                     # more ranks than GPUs (e.g. `--gpus 2` on a 1-GPU box): ranks share devices round-robin — a plumbing run,
    local_rank = local_rank % n_dev                            # labelled `gpu_sharing` in the line; RCCL needs one GPU per rank, so the counters then travel over gloo
    torch.cuda.set_device(local_rank)
    affinity_at_start = sorted(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else None
    numa = bind_to_gpu_numa(local_rank) if world > 1 else None  # each rank's host threads (launch loop, pinned staging buffers of the host_io leg) next to its GPU
    coll = Collective(gpu=not shared) if world > 1 else None   # RCCL over xGMI, probed; labelled gloo fall-back if RCCL cannot be brought up
    if coll is not None and shared:
        coll.backend, coll.note = "gloo (ranks share GPUs)", "%d ranks on %d visible GPU(s): RCCL requires one GPU per rank" % (world, n_dev)

    W, H, B = args.width, args.height, args.batch
    moving = not args.static_scene
    default_job = (args.model, W, H, B) == ("lite", 640, 480, 256) and not args.per_stream_bg and not args.bg_ring
    side = args.full and not args.no_side_probes
    solo1 = solo4 = None
    if coll is not None and args.full:
        # rank 0 ALONE first (the others wait at the barrier): the N = 1 reference of this box, minutes — not runs — apart from the N-rank number
        def solo_main():
            r1 = measure(args.model, W, H, B, args.steps, args.warmup, 0, 1, local_rank, ramp_s=args.ramp_seconds, per_stream_bg=args.per_stream_bg, bg_ring=args.bg_ring,
                         profile=False, moving=moving)
            fps = r1["fps"]
            release(r1)
            return fps
        solo1 = solo_reference(coll, rank, solo_main)
    res = measure(args.model, W, H, B, args.steps, args.warmup, rank, world, local_rank, ramp_s=args.ramp_seconds, per_stream_bg=args.per_stream_bg, bg_ring=args.bg_ring,
                  profile_iters=args.profile_iters, dump_launches=args.dump_launches, coll=coll, profile=args.full, moving=moving, static_leg=side, parity_streams=4,
                  dump_outputs=args.dump_outputs)
    multi = None
    c4_frag = c4_parity_in = None
    if coll is not None:
        main_leg = {k: res[k] for k in ("B", "W", "H", "model_name", "fps", "ms_per_step", "rank_fps")}
        c4 = None
        if args.full and default_job and not args.no_extra_configs:
            # the north-star job's per-GPU slice on EVERY rank: BASELINE configs[4] = 8192 x HD segm_full streams / 8 GPUs = 1024 per GPU
            n4 = max(20, args.steps // 4)
            kw4 = dict(model_key="full", W=1280, H=720, B=1024, moving=moving)
            try:
                def solo_c4():
                    r4s = measure(steps=n4, warmup=3, rank=0, world=1, local_rank=local_rank, profile=False, **kw4)
                    fps = r4s["fps"]
                    release(r4s)
                    return fps
                solo4 = solo_reference(coll, rank, solo_c4)
                r4 = measure(steps=n4, warmup=3, rank=rank, world=world, local_rank=local_rank, profile_iters=4, coll=coll, **kw4)
                c4 = {k: r4[k] for k in ("B", "W", "H", "model_name", "fps", "ms_per_step", "rank_fps")}
                if rank == 0:
                    c4_frag = summarize(r4, load_pmc(1024, 1280, 720, r4["model_name"]))
                    c4_parity_in = (r4["model_path"], r4["parity_in"])
                release(r4)
            except Exception as e:  # noqa: BLE001 — every rank takes the same path: the exception classes here are allocation / model errors, identical on all ranks
                c4 = None
                if rank == 0:
                    c4_frag = {"error": repr(e)}
        if rank == 0:
            multi = multi_gpu_sections(coll, main_leg, c4, solo1, solo4, world)
            if c4_frag is not None and "configs4" in multi:
                multi["configs4"].update({k: v for k, v in c4_frag.items() if k in ("roofline", "stage_ms", "top_launches", "full_batch_twin_streams", "error")})
        coll.close()                                          # ranks > 0 are done; rank 0 goes on alone (parity, CPU baseline, the device check)
    if rank != 0:
        release(res)
        return
    import backscrub_amd
    mode = backscrub_amd.bs_tensorflow_version()
    scene = ("moving scene: ring of %d batches, a new one every step" % RING) if moving else "static scene: the same batch every step"
    result = {
        "metric": METRIC, "value": round(res["fps"], 1), "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(res["ms_per_step"], 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32 (network) / u8 (image kernels)", "data": "synthetic (%s)" % res["weights"],
        "config": {"workload": "BASELINE configs[1]: batch=%d %dx%d frames, %s; %s; 1 step = prep+network+decode+mask+blend, inputs resident in HBM"
                               % (B, W, H, res["model_name"], scene),
                   "streams_per_gpu": B, "sharding": "streams/%d GPUs, no data-path collective" % world, "library": mode},
        "checksum": res["checksum"], "host": cpu_description(), "numa_binding": numa,
        "env_set": {k_: v_ for k_, v_ in sorted(os.environ.items()) if k_.startswith("BSX_")},      # every library switch the process started with (none = the default build's defaults)
        "definitions": {"roofline.frac": "bytes of the launch that must cross HBM (algorithmic bytes for this input minus reads of the one background image all streams share) "
                                         "/ the launch's duration inside the step (hipEvent figure minus the per-launch event cost: event_overhead; sum of launches == ms_per_step) / 8000 GB/s "
                                         "— for every launch of every configuration; a general mask tile moves 10 B/px, a uniform one 7, outside the ROI 6",
                        "dense_10Bpx_GBps": "SURVEY 8(d)'s 10 B/px over the same duration: not a bandwidth (uniform tiles and the shared background move fewer bytes)",
                        "static_scene": "the same batch every step (rounds 1-4's headline protocol): the uniform-tile shortcut's best case",
                        "worst_case": "BSX_NO_UNIFORM_TILES=1 and one random background image per stream, moving scene: every byte from HBM, every tile on the general path"},
    }
    if multi is not None:
        result.update(multi)
        if shared:
            result["gpu_sharing"] = "%d ranks on %d GPU(s): throughput numbers of this line are a plumbing run, not a scaling measurement" % (world, n_dev)
    result["detail_file"] = os.path.basename(args.detail) if args.detail else "bench_detail.json"
    if not args.full:                                   # a plain run: the headline figure is all it measures
        release(res)
        emit(result, args.detail)
        return
    result.update({k: v for k, v in summarize(res, load_pmc(B, W, H, res["model_name"])).items() if k not in ("value", "unit", "ms_per_step", "steps", "warmup")})
    mg, ring, d_bg, d_out = res["mg"], res["frames_ring"], res["d_bg"], res["d_out"]
    d_frames = ring[0]

    # PCIe-inclusive variant: every step uploads its frames and downloads its composites through pinned buffers.
    # Copies run on their own HIP streams with double-buffered device frames / composites, so the upload of step t+1 and the
    # download of step t-1 overlap the compute of step t (the per-stream mask state keeps the compute steps in order).
    if world == 1 and not args.no_host_io and side:
        h_in = ring[0].cpu().pin_memory()
        h_out = torch.empty_like(h_in).pin_memory()
        s_in, s_out, s_cmp = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.current_stream()
        bufs = [(torch.empty_like(d_frames), torch.empty_like(d_out)) for _ in range(2)]
        ev_in = [torch.cuda.Event() for _ in range(2)]
        ev_cmp = [torch.cuda.Event() for _ in range(2)]
        ev_out = [torch.cuda.Event() for _ in range(2)]

        def run(steps):
            for t in range(steps):
                fr, out = bufs[t & 1]
                with torch.cuda.stream(s_in):
                    s_in.wait_event(ev_cmp[t & 1])            # the step that last read this frame buffer has finished
                    fr.copy_(h_in, non_blocking=True)
                    ev_in[t & 1].record(s_in)
                s_cmp.wait_event(ev_in[t & 1])
                s_cmp.wait_event(ev_out[t & 1])               # the composite buffer has been downloaded
                mg.step(fr, d_bg, out)
                ev_cmp[t & 1].record(s_cmp)
                with torch.cuda.stream(s_out):
                    s_out.wait_event(ev_cmp[t & 1])
                    h_out.copy_(out, non_blocking=True)
                    ev_out[t & 1].record(s_out)
            torch.cuda.synchronize()

        run(2)
        io_steps = max(20, min(args.steps, 100))                      # >= 20 steps (round 5's 4-step leg read 31-44 k where 100 steps read 51.7 k: VERDICT r5 weak #7)
        t1 = time.perf_counter()
        run(io_steps)
        dt = time.perf_counter() - t1
        result["host_io"] = {"value": round(B * io_steps / dt, 1), "unit": "frames/s", "ms_per_step": round(1e3 * dt / io_steps, 3), "steps": io_steps,
                             "note": "same step + H2D of %d frames and D2H of %d composites per step (pinned buffers, copy streams overlapped with "
                                     "compute, double-buffered); %.1f GB/s each way" % (B, B, B * W * H * 3 / (dt / io_steps) / 1e9)}
        del bufs, h_in, h_out

    # the same step with the composite leaving as YUYV 4:2:2 (convert_rgb_to_yuyv fused into the blend epilogue): reported
    # next to `value`, never as `value`; checked bit for bit against the two-call form
    if world == 1 and W % 2 == 0 and not args.no_extra_configs and side:
        d_yuyv = torch.empty((B, H, W, 2), dtype=torch.uint8, device="cuda")
        mg.reset(); mg.step(d_frames, d_bg, d_out); a = mg.bgr_to_yuyv(d_out)          # both forms from the same (fresh) temporal state
        mg.reset(); mg.step_yuyv(d_frames, d_bg, d_yuyv)
        same = bool(torch.equal(a, d_yuyv))
        n_y = max(20, min(args.steps, 100))
        for t in range(5):
            mg.step_yuyv(ring[t % len(ring)], d_bg, d_yuyv)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for t in range(n_y):
            mg.step_yuyv(ring[t % len(ring)], d_bg, d_yuyv)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t1
        result["yuyv_out"] = {"value": round(B * n_y / dt, 1), "unit": "frames/s", "ms_per_step": round(1e3 * dt / n_y, 4), "steps": n_y,
                              "bit_identical_to_step_then_bgr_to_yuyv": same,
                              "note": "bsx_step_batch_yuyv: composite written as YUYV (2 B/px instead of 3), no separate packing pass"}
        del d_yuyv, a

    # YUYV in -> YUYV out as ONE step (BSX_STEP_YUYV_IN | BSX_STEP_YUYV, SURVEY §8 f3 + f1): the camera's raw 4:2:2 frames in, the loop-back device's wire format out —
    # 7 B/px of device traffic instead of 9, 4 B/px over PCIe instead of 6.  Device-resident leg + the PCIe-inclusive leg next to `host_io`; both beside `value`.
    if world == 1 and W % 4 == 0 and not args.no_extra_configs and side:
        def to_camera_yuyv(bgr):                                           # BT.601 limited range, Y0 U Y1 V: what a YUYV webcam would deliver for this scene
            f = bgr.to(torch.float32)
            b_, g_, r_ = f[..., 0], f[..., 1], f[..., 2]
            y = 16 + 0.257 * r_ + 0.504 * g_ + 0.098 * b_
            u = 128 - 0.148 * r_ - 0.291 * g_ + 0.439 * b_
            v = 128 + 0.439 * r_ - 0.368 * g_ - 0.071 * b_
            o = torch.empty(bgr.shape[:-1] + (2,), dtype=torch.uint8, device=bgr.device)
            o[..., 0] = y.round().clamp(0, 255).to(torch.uint8)
            o[:, :, 0::2, 1] = ((u[:, :, 0::2] + u[:, :, 1::2]) / 2).round().clamp(0, 255).to(torch.uint8)
            o[:, :, 1::2, 1] = ((v[:, :, 0::2] + v[:, :, 1::2]) / 2).round().clamp(0, 255).to(torch.uint8)
            return o
        raw_ring = [to_camera_yuyv(fr) for fr in ring]
        d_y = torch.empty((B, H, W, 2), dtype=torch.uint8, device="cuda")
        mg.reset(); bgr0 = mg.yuyv_to_bgr(raw_ring[0]); mg.step_yuyv(bgr0, d_bg, d_y); a = d_y.clone()       # convert + BGR step with YUYV out, from a fresh temporal state
        mg.reset(); mg.step_ex(raw_ring[0], d_bg, d_y, yuyv=True, yuyv_in=True)
        same = bool(torch.equal(a, d_y))
        del a, bgr0
        n_y = max(20, min(args.steps, 100))
        for t in range(5):
            mg.step_ex(raw_ring[t % len(ring)], d_bg, d_y, yuyv=True, yuyv_in=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for t in range(n_y):
            mg.step_ex(raw_ring[t % len(ring)], d_bg, d_y, yuyv=True, yuyv_in=True)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t1
        result["yuyv_in_out"] = {"value": round(B * n_y / dt, 1), "unit": "frames/s", "ms_per_step": round(1e3 * dt / n_y, 4), "steps": n_y,
                                 "bit_identical_to_yuyv_to_bgr_then_step_yuyv": same,
                                 "note": "bsx_step_batch_ex(BSX_STEP_YUYV_IN | BSX_STEP_YUYV): raw camera frames in (2 B/px), composite out as YUYV (2 B/px); no BGR frame in between"}
        if not args.no_host_io:
            h_in = raw_ring[0].cpu().pin_memory()
            h_out = torch.empty_like(h_in).pin_memory()
            s_in, s_out, s_cmp = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.current_stream()
            bufs = [(torch.empty_like(raw_ring[0]), torch.empty_like(d_y)) for _ in range(2)]
            ev_in, ev_cmp, ev_out = ([torch.cuda.Event() for _ in range(2)] for _ in range(3))

            def run_y(steps):
                for t in range(steps):
                    fr, out = bufs[t & 1]
                    with torch.cuda.stream(s_in):
                        s_in.wait_event(ev_cmp[t & 1])
                        fr.copy_(h_in, non_blocking=True)
                        ev_in[t & 1].record(s_in)
                    s_cmp.wait_event(ev_in[t & 1])
                    s_cmp.wait_event(ev_out[t & 1])
                    mg.step_ex(fr, d_bg, out, yuyv=True, yuyv_in=True)
                    ev_cmp[t & 1].record(s_cmp)
                    with torch.cuda.stream(s_out):
                        s_out.wait_event(ev_cmp[t & 1])
                        h_out.copy_(out, non_blocking=True)
                        ev_out[t & 1].record(s_out)
                torch.cuda.synchronize()
            run_y(2)
            io_steps = max(20, min(args.steps, 100))
            t1 = time.perf_counter()
            run_y(io_steps)
            dt = time.perf_counter() - t1
            result["host_io_yuyv"] = {"value": round(B * io_steps / dt, 1), "unit": "frames/s", "ms_per_step": round(1e3 * dt / io_steps, 3), "steps": io_steps,
                                      "note": "the YUYV in -> YUYV out step + H2D of %d raw frames and D2H of %d YUYV composites per step (2 B/px each way, pinned, "
                                              "copy streams overlapped with compute); %.1f GB/s each way" % (B, B, B * W * H * 2 / (dt / io_steps) / 1e9)}
            del bufs, h_in, h_out
        del raw_ring, d_y

    # `-p bgblur:25` without `-b` (deepseg.cc:652-661): background = GaussianBlur of the stream's own frame.  One pass (BSX_STEP_BGBLUR: blur tile → blend out of LDS)
    # against the two-call form (bsx_gaussian_blur_bgr into a per-stream background, then bsx_step_batch)
    if world == 1 and not args.no_extra_configs and W % 4 == 0 and side:
        d_two = torch.empty_like(d_out)
        d_blur = torch.empty_like(d_frames)

        def two_call(t):
            mg.gaussian_blur(ring[t % len(ring)], 25, out=d_blur)
            mg.step(ring[t % len(ring)], d_blur, d_two)

        def one_pass(t):
            mg.step_ex(ring[t % len(ring)], None, d_out, bgblur=25)

        def timed(fn, iters=max(20, args.steps // 4)):
            for t in range(3):
                fn(t)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for t in range(iters):
                fn(t)
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t1) / iters
        ms_two, ms_one = timed(two_call), timed(one_pass)
        result["bgblur_step"] = {"ksize": 25, "ms_per_step": round(ms_one, 4), "value": round(B / (ms_one * 1e-3), 1), "unit": "frames/s",
                                 "two_call_ms_per_step": round(ms_two, 4), "speedup": round(ms_two / ms_one, 3),
                                 "note": "bsx_step_batch_ex(BSX_STEP_BGBLUR(25)): blur + blend in one pass over the frames vs bsx_gaussian_blur_bgr + bsx_step_batch"}
        del d_two, d_blur

    # the blend kernel with ONE BACKGROUND PER STREAM (animated backgrounds): every byte of its 10 B/px is HBM traffic, unlike the shared 0.9 MB picture of the
    # default job — the north star's "HBM roofline of the blend kernel" figure
    if world == 1 and not args.per_stream_bg and side:
        d_bg_ps = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device="cuda")
        for _ in range(3):
            mg.composite(d_bg_ps, d_frames, None, d_out)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        iters = 20
        e0.record()
        for _ in range(iters):
            mg.composite(d_bg_ps, d_frames, None, d_out)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / iters
        by = 10.0 * W * H * B
        result["roofline_blend_per_stream_bg"] = {"kernel": "blend", "bound": "hbm", "achieved": round(by / (ms * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS,
                                                  "unit": "GB/s", "frac": round(by / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "traffic": None, "avg_ms": round(ms, 4),
                                                  "hbm_bytes_per_launch": int(by),
                                                  "note": "bsx_composite_batch with a separate background image per stream: every byte of the 10 B/px is HBM traffic"}
        del d_bg_ps

    main_parity_in = (res["model_path"], res["parity_in"])
    del mg, ring, d_bg, d_out, d_frames
    release(res)

    if world > 1:
        # the GPU legs are over and the other ranks have left: rank 0 takes back the affinity mask it started with, so that the CPU baseline below runs on the box's
        # host cores and not on one NUMA node's share of them (the N > 1 line otherwise under-reports the CPU by the number of nodes)
        if affinity_at_start and numa and numa.get("bound"):
            try:
                os.sched_setaffinity(0, affinity_at_start)
                numa["restored_for_cpu_baseline"] = len(affinity_at_start)
            except OSError as e:
                numa["restored_for_cpu_baseline"] = "failed: %s" % e
        result["second_device_check"] = run_second_device_check()
        if c4_parity_in is not None and not args.no_cpu_baseline and "configs4" in result:
            result["configs4"]["parity_sample"] = parity_sequence(c4_parity_in[0], 1280, 720, c4_parity_in[1])
    if not args.no_cpu_baseline:                        # kept at N > 1: rank 0, after the other ranks have left (their GPUs idle, the host cores free)
        try:
            result["cpu_baseline"] = cpu_baseline(main_parity_in[0], W, H, args.cpu_seconds)
            result["cpu_baseline"]["parity_sample"] = parity_sequence(main_parity_in[0], W, H, main_parity_in[1])
        except Exception as e:  # the baseline must never take the GPU number down with it
            result["cpu_baseline"] = {"value": None, "unit": "frames/s", "cores": os.cpu_count(), "kind": "port", "sample": "failed: %r" % (e,)}

    def extra_steps(ms_guess):
        """≥ 20 timed steps everywhere; more where a step is short"""
        return int(max(20, min(args.steps, 200, 400.0 / ms_guess)))

    def run_config(tag, kw, steps, env=None, cpu=True, **mkw):
        """one more configuration through measure() → its summarized fragment (+ parity sample and its own CPU baseline)"""
        saved = {k_: os.environ.get(k_) for k_ in (env or {})}
        os.environ.update(env or {})
        try:
            r = measure(steps=steps, warmup=3, rank=0, world=1, local_rank=local_rank, profile_iters=4, ramp_s=0.5, static_leg=True, **kw, **mkw)
            frag = summarize(r, load_pmc(kw["B"], kw["W"], kw["H"], r["model_name"]))
            frag = {"baseline_config": tag, "net": _short_model(r["model_name"]), "batch": kw["B"], "frame": "%dx%d" % (kw["W"], kw["H"]), **frag}
            mp_, seq = r["model_path"], r["parity_in"]
            release(r)
            if not args.no_cpu_baseline:
                frag["parity_sample"] = parity_sequence(mp_, kw["W"], kw["H"], seq)
                if cpu:
                    frag["cpu_baseline"] = cpu_baseline(mp_, kw["W"], kw["H"], args.cpu_seconds / 3.0, short=True)
            return frag
        finally:
            for k_, v_ in saved.items():
                if v_ is None:
                    os.environ.pop(k_, None)
                else:
                    os.environ[k_] = v_

    if world == 1 and side and not args.per_stream_bg:
        # the worst case beside `value`: every mask tile on the general path, one random background image per stream (nothing cache-resident)
        try:
            w = run_config("worst_case", dict(model_key=args.model, W=W, H=H, B=B), extra_steps(0.5), env={"BSX_NO_UNIFORM_TILES": "1"}, cpu=False, per_stream_bg=True)
            result["worst_case"] = w
        except Exception as e:  # noqa: BLE001
            result["worst_case"] = {"error": repr(e)}

    if world == 1 and default_job and not args.no_extra_configs:
        result["configs"] = []
        # configs[0]: one VGA frame, MLKit, the reference's CPU path (plumbing) — the CPU oracle on one stream, next to the drop-in single-frame GPU path
        try:
            mp0, name0, _ = resolve_model("mlkit")
            f0 = {"baseline_config": "configs[0]", "net": "mlkit", "batch": 1, "frame": "640x480"}
            if not args.no_cpu_baseline:
                f0["cpu_baseline"] = cpu_baseline(mp0, 640, 480, args.cpu_seconds / 3.0, short=True)
            ss = single_stream_latency("mlkit", 640, 480, 100)
            f0.update({"value": ss["fps_at_p50"], "ms_per_step": ss["p50_ms"], "steps": ss["calls"], "single_stream": ss,
                       "what": "one stream through bsx_process_host (= bs_maskgen_process): H2D frame, mask pipeline, D2H mask, synchronous; cpu_baseline = the oracle on the same frame size"})
            result["configs"].append(f0)
        except Exception as e:  # noqa: BLE001
            result["configs"].append({"baseline_config": "configs[0]", "error": repr(e)})
        # the other single-GPU BASELINE configurations, same protocol
        extra_cfgs = [
            ("configs[2]", dict(model_key="mlkit", W=1280, H=720, B=256), 1.4, {}),
            ("configs[3]", dict(model_key="deeplab", W=640, H=480, B=1024), 17.0, dict(bg_ring=True, parity_steps=5)),       # animated background: per-step H2D of a 480x360 frame + GPU resize, timed
            ("configs[4]/8", dict(model_key="full", W=1280, H=720, B=1024), 3.2, {}),                          # the 8192-stream job's per-GPU slice
        ]
        gif = os.path.join(ROOT, "models", "backgrounds", "animated.gif")       # the reference's backgrounds/animated.gif, staged as data by tools/stage_models.py
        for tag, kw, ms_guess, mkw in extra_cfgs:
            try:
                if tag == "configs[3]" and os.path.exists(gif):
                    # the animated background through the product's OWN background source (bsx_background_load / _grab = load_background / grab_background,
                    # app/background.cc:126-194) is the figure; the pinned-ring H2D emulation of rounds 1-5 ("the decode happens elsewhere") stays beside it
                    frag = run_config(tag, kw, extra_steps(ms_guess), bg_source=gif, parity_steps=5)
                    try:
                        r2 = measure(steps=extra_steps(ms_guess), warmup=3, rank=0, world=1, local_rank=local_rank, profile=False, ramp_s=0.5, bg_ring=True, **kw)
                        frag["decode_elsewhere_h2d_ring"] = {"value": round(r2["fps"], 1), "ms_per_step": round(r2["ms_per_step"], 4),
                                                             "what": "36 pre-decoded 480x360 frames in pinned host memory: per step H2D of one frame + bsx_resize_bgr"}
                        release(r2)
                    except Exception as e2:  # noqa: BLE001
                        frag["decode_elsewhere_h2d_ring"] = {"error": repr(e2)}
                    result["configs"].append(frag)
                    continue
                result["configs"].append(run_config(tag, kw, extra_steps(ms_guess), **mkw))
            except Exception as e:  # noqa: BLE001
                result["configs"].append({"baseline_config": tag, "error": repr(e)})
        # opt-in reduced-precision modes, each with its own parity sample (they FAIL the north star's <= 1 LSB bar and are never defaults):
        # BSX_F16_GEMM (DeepLab's per-launch path: fast = plain f16 MFMA operands, fast16 = + f16 storage of the fused blocks' depthwise outputs, off = f32 MFMA)
        # BSX_ACT16 (Meet / MLKit: activation tensors in HBM stored as f16, f32 arithmetic)
        result["gemm_modes"], result["act_modes"] = [], []
        for mode in ("fast16", "fast", "off"):
            try:
                f = run_config("configs[3]", dict(model_key="deeplab", W=640, H=480, B=1024), 20, env={"BSX_F16_GEMM": mode}, cpu=False, bg_ring=True, parity_steps=4)
                result["gemm_modes"].append({"env": "BSX_F16_GEMM=" + mode, "cfg": 3, **{k_: f[k_] for k_ in ("value", "ms_per_step", "steps", "parity_sample", "top_launches") if k_ in f}})
            except Exception as e:  # noqa: BLE001
                result["gemm_modes"].append({"env": "BSX_F16_GEMM=" + mode, "cfg": 3, "error": repr(e)})
        for cfg, kw, ms_guess in ((1, dict(model_key="lite", W=640, H=480, B=256), 0.4), (2, dict(model_key="mlkit", W=1280, H=720, B=256), 1.4)):
            try:
                f = run_config("configs[%d]" % cfg, kw, extra_steps(ms_guess), env={"BSX_ACT16": "1"}, cpu=False)
                result["act_modes"].append({"env": "BSX_ACT16=1", "cfg": cfg, **{k_: f[k_] for k_ in ("value", "ms_per_step", "steps", "parity_sample", "top_launches") if k_ in f}})
            except Exception as e:  # noqa: BLE001
                result["act_modes"].append({"env": "BSX_ACT16=1", "cfg": cfg, "error": repr(e)})
        try:
            result["single_stream"] = {"what": "bsx_process_host per call (= bs_maskgen_process through the C++ shim): H2D frame, whole mask pipeline, D2H mask, synchronous",
                                       "runs": [single_stream_latency("lite", 640, 480, 200), single_stream_latency("deeplab", 640, 480, 60)],
                                       "published_context_not_measured_here": "reference README.md:177 ~10 FPS DeepLab on two i5 cores; Meet model card ~120 FPS inference on a laptop CPU"}
        except Exception as e:  # noqa: BLE001
            result["single_stream"] = {"error": repr(e)}
    emit(result, args.detail)


if __name__ == "__main__":
    main()
