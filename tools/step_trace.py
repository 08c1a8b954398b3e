"""Launch traces of the batch step, on a box without a GPU: compare what two builds of libbsx.so enqueue.

Every HIP call of the library goes through tests/hip_stub/libhipstub.so (LD_PRELOAD; "device memory" is host memory and kernels do not run).  For each
configuration (model x frame geometry x debug switch) a child process creates one context on the library named by BSX_LIBRARY (default: the in-tree
libbsx.so) and drives a fixed matrix of calls through it: process / step / step_yuyv / step_ex / step_streams with every flag route, step_vcam, the two-deep
pipeline, the profile, the host path, the stage-debug entry and the refusals.  Each call's trace is the list of HIP calls it made — API, kernel, grid, block,
dynamic LDS, stream and event (numbered by first use), copy / set / allocation sizes — with its return code.

    python tools/step_trace.py --out a.json [--debug]         # one library (BSX_LIBRARY selects it), every configuration
    python tools/step_trace.py --diff a.json b.json            # calls whose return code or trace differ

trace_all(sizes=[(model, W, H[, n_streams])], brief=True) is the geometry audit's form (tests/test_geometry_host.py): one context per listed size, the short call
list of drive(brief=True) — the plain step, one call per flag route that picks another image kernel, the mixed step, stages 0 / 3 / 4 — and the context's own
roi / in_roi under "_info".  roi_sweep() (child, --roi-sweep) creates one context per size of a list and returns the rectangles bsx_get_info reports.
"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB_DIR = os.path.join(ROOT, "tests", "hip_stub")
STUB = os.path.join(STUB_DIR, "libhipstub.so")
REF_MODELS = os.path.join(ROOT, "tests", "golden", "reference_models")
MODELS = {"lite": os.path.join(REF_MODELS, "segm_lite_v681.tflite"), "full": os.path.join(REF_MODELS, "segm_full_v679.tflite"),
          "mlkit": os.path.join(REF_MODELS, "selfiesegmentation_mlkit-256x256-2021_01_19-v1215.f16.tflite"), "deeplab": None}    # None: the synthetic DeepLab
GEOMETRIES = [(640, 480), (1280, 720), (642, 480)]          # the last one: width % 4 != 0, the fused tile kernel does not apply
SWITCHES = ["BSX_NO_MASK_BLEND_FUSION", "BSX_NO_BGBLUR_FUSION", "BSX_NO_MASK_TILE", "BSX_LANES=2", "BSX_LANES=4", "BSX_KEEP_LOGITS", "BSX_NO_RTC",
            "BSX_NO_SEGMENTS", "BSX_NO_FRAME_PROGRAM", "BSX_VCAM_DIRECT", "BSX_NO_SEG_RTC"]

YUYV, FH, FV, NOMASK, YIN = 1, 2, 4, 8, 16


def blur(k):
    return (k & 255) << 8


def build_stub():
    src = os.path.join(STUB_DIR, "hip_stub.cpp")
    if not os.path.exists(STUB) or os.path.getmtime(STUB) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", STUB, src])
    return STUB


def model_file(key):
    if MODELS[key]:
        return MODELS[key]
    sys.path.insert(0, ROOT)
    from tools import make_synthetic_model
    return make_synthetic_model.ensure(key)


# ---- child: runs under the stub -------------------------------------------------------------------------------------------------------------------------------
def drive(model, W, H, n, brief=False):
    """every call of the matrix on one context → {key: {"rc", "error", "log": [first, last)}}; brief: the geometry audit's short list (the plain step, one call
    per flag route that picks another image kernel, the stage entries) and the context's own geometry under "_info" """
    sys.path.insert(0, ROOT)
    import numpy as np
    from backscrub_amd import api
    L = C.CDLL(api.lib_path())
    for name, res, args in api.SYMBOLS:
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    ctx = L.bsx_new(model.encode(), 2, W, H, n, 0, api.DEBUG_FN(), api.STAGE_FN(), api.STAGE_FN(), api.STAGE_FN(), None)
    if not ctx:
        return {"error": (L.bsx_last_error(None) or b"").decode(errors="replace")}
    info = api._Info()
    L.bsx_get_info(ctx, C.byref(info))
    fb = H * W * 3
    # one arena for all "device" buffers, so that offsets (overlaps) are plain arithmetic; every buffer starts 256-byte aligned
    sizes = {"frames": 2 * n * fb, "yuyv": n * H * W * 2, "bg": fb, "bgs": n * fb, "out": n * fb, "out2": n * H * W * 2, "vout": n * 2 * fb, "mask": H * W}
    mem = np.zeros(sum(s + 256 for s in sizes.values()) + 256, np.uint8)
    base = (mem.ctypes.data + 255) // 256 * 256
    at = {}
    for k, s in sizes.items():
        at[k] = base
        base += (s + 255) // 256 * 256
    P = lambda a: C.c_void_p(a) if a else None          # noqa: E731
    fr, yu, bg, out, out2, vout = at["frames"], at["yuyv"], at["bg"], at["out"], at["out2"], at["vout"]
    log = os.environ["BSX_STUB_LOG"]
    lines = lambda: sum(1 for _ in open(log)) if os.path.exists(log) else 0     # noqa: E731
    calls = {}

    def run(key, fn):
        a = lines()
        rc = fn()
        calls[key] = {"rc": rc, "error": (L.bsx_last_error(ctx) or b"").decode(errors="replace").strip(), "log": [a, lines()]}

    def ex(key, flags=0, frames=fr, b=bg, o=out, stride=0, nn=n):
        run("ex_" + key, lambda: L.bsx_step_batch_ex(ctx, P(frames), P(b), stride, P(o), nn, None, flags))

    def streams(key, ids, flags=0, frames=fr, b=bg, o=out, stride=0, nn=None):
        arr = (C.c_int * max(len(ids), 1))(*ids)
        run("streams_" + key, lambda: L.bsx_step_batch_streams(ctx, arr if ids else None, P(frames), P(b), stride, P(o), len(ids) if nn is None else nn, None, flags))

    def vcam(key, ow, oh, flags=0, frames=fr, b=bg, o=vout, stride=0, nn=n):
        run("vcam_" + key, lambda: L.bsx_step_batch_vcam(ctx, P(frames), P(b), stride, P(o), ow, oh, nn, None, flags))

    def pipe(key, flags=0, frames=fr, b=bg, o=out, nn=n):
        run("pipe_" + key, lambda: L.bsx_step_batch_pipelined(ctx, P(frames), P(b), 0, P(o), nn, None, flags))

    if brief:
        run("step", lambda: L.bsx_step_batch(ctx, P(fr), P(bg), 0, P(out), n, None))
        for key, flags, frames, o in [("flip_h", FH, fr, out), ("yuyv", YUYV, fr, out2), ("yuyv_flip", YUYV | FH, fr, out2), ("no_mask_flip_v", NOMASK | FV, fr, out),
                                      ("yuyv_in", YIN, yu, out), ("in_place", 0, fr, fr)]:
            ex(key, flags, frames, bg, o)
        st = (api._StreamSetting * n)()
        for i in range(n):
            st[i].d_bg, st[i].flags = at["bgs"] + i * fb, (FH, FV, 0)[i % 3]
        run("mixed", lambda: L.bsx_step_batch_mixed(ctx, None, P(fr), st, P(out), n, None, 0))
        for st_ in (0, 3, 4):
            run("stage_%d" % st_, lambda: L.bsx_debug_run_stage(ctx, st_, P(yu if st_ == 4 else fr), n, None))
        run("delete", lambda: L.bsx_delete(ctx) or 0)
        calls["_info"] = {k: (list(getattr(info, k)) if k in ("roi", "in_roi") else getattr(info, k)) for k, _ in api._Info._fields_}
        return calls
    run("process_batch", lambda: L.bsx_process_batch(ctx, P(fr), n, None, None))
    run("process_batch_masks", lambda: L.bsx_process_batch(ctx, P(fr), n, P(out), None))
    run("step", lambda: L.bsx_step_batch(ctx, P(fr), P(bg), 0, P(out), n, None))
    run("step_bgs", lambda: L.bsx_step_batch(ctx, P(fr), P(at["bgs"]), fb, P(out), n, None))
    run("step_yuyv", lambda: L.bsx_step_batch_yuyv(ctx, P(fr), P(bg), 0, P(out2), n, None))
    perm = list(range(n))[::-1]
    routes = [("plain", 0, fr, out), ("flip_h", FH, fr, out), ("flip_v", FV, fr, out), ("flip_hv", FH | FV, fr, out), ("yuyv", YUYV, fr, out2),
              ("yuyv_flip", YUYV | FH, fr, out2), ("no_mask", NOMASK, fr, out), ("yuyv_in", YIN, yu, out), ("yuyv_in_out", YIN | YUYV, yu, out2),
              ("yuyv_in_flip", YIN | FV, yu, out), ("bgblur25", blur(25), fr, out), ("bgblur25_flip", blur(25) | FH, fr, out), ("bgblur25_yuyv", blur(25) | YUYV, fr, out2),
              ("bgblur1", blur(1), fr, out), ("bgblur25_yuyv_in", blur(25) | YIN, yu, out), ("in_place", 0, fr, fr), ("in_place_flip", FH, fr, fr),
              ("in_place_yuyv", YUYV, fr, fr), ("in_place_no_mask", NOMASK, fr, fr), ("in_place_yuyv_in", YIN, yu, yu),
              ("unaligned_out", 0, fr, out + 2), ("unaligned_yuyv", YUYV, fr, out2 + 2)]
    for key, flags, frames, o in routes:
        b = None if flags & 0xFF00 else bg
        ex(key, flags, frames, b, o)
        streams(key, perm, flags, frames, b, o)
    streams("subset", [n - 1, 0])
    # the virtual camera: up, down, 2x area, a strong down-scale (per-tap table), YUYV out / in, blur, flips, the capture size
    for key, ow, oh, flags in [("up", W * 3 // 2, H * 3 // 2, 0), ("down", W * 2 // 3 // 2 * 2, H * 2 // 3, 0), ("area", W // 2, H // 2, 0),
                               ("per_tap", W // 6 // 2 * 2, H // 6, 0), ("yuyv_out", W // 2, H // 2, YUYV), ("yuyv_in", W * 2 // 3 // 2 * 2, H * 2 // 3, YIN),
                               ("yuyv_in_out", W // 2, H // 2, YIN | YUYV), ("blur", W // 2, H // 2, blur(25)), ("blur_yuyv_in", W // 2, H // 2, blur(25) | YIN),
                               ("flip_hv", W * 2 // 3 // 2 * 2, H * 2 // 3, FH | FV), ("capture", W, H, 0), ("capture_flip", W, H, FH)]:
        vcam(key, ow, oh, flags, yu if flags & YIN else fr, None if flags & 0xFF00 else bg)
    # the two-deep pipeline: the first call only enqueues, the next ones fork the previous composite; then the flush
    for i in range(3):
        pipe("%d" % i, YUYV if i == 2 else 0, o=out2 if i == 2 else out)
    # every entry point refuses while a composite is pending
    run("pending_process", lambda: L.bsx_process_batch(ctx, P(fr), n, None, None))
    run("pending_step", lambda: L.bsx_step_batch(ctx, P(fr), P(bg), 0, P(out), n, None))
    ex("pending", FH)
    streams("pending", [0])
    vcam("pending", W // 2, H // 2)
    stats = (api.LaunchStat * (info.n_steps + 8))()
    run("pending_profile", lambda: L.bsx_profile_batch(ctx, P(fr), P(bg), 0, P(out), n, 1, stats, info.n_steps + 8, None))
    run("pipe_flush", lambda: L.bsx_step_batch_pipelined(ctx, None, None, 0, None, 0, None, 0))
    run("pipe_flush_again", lambda: L.bsx_step_batch_pipelined(ctx, None, None, 0, None, 0, None, 0))
    pipe("yuyv_in", YIN)
    run("pipe_flush_yuyv_in", lambda: L.bsx_step_batch_pipelined(ctx, None, None, 0, None, 0, None, 0))
    run("profile", lambda: L.bsx_profile_batch(ctx, P(fr), P(bg), 0, P(out), n, 2, stats, info.n_steps + 8, None))
    small = (api.LaunchStat * 2)()
    run("profile_cap", lambda: L.bsx_profile_batch(ctx, P(fr), P(bg), 0, P(out), n, 1, small, 2, None))
    for i in range(2):
        run("process_host_%d" % i, lambda: L.bsx_process_host(ctx, 1, P(fr), W * 3, P(at["mask"]), W))
    for st in range(5):
        run("stage_%d" % st, lambda: L.bsx_debug_run_stage(ctx, st, P(yu if st == 4 else fr), n, None))
    # refusals
    ex("null_frames", frames=0)
    ex("null_out", o=0)
    ex("null_bg", b=0)
    ex("n0", nn=0)
    ex("n_too_big", nn=n + 1)
    ex("unknown_flag", 32)
    ex("bgblur_even", blur(24), b=0)
    ex("bgblur_33", blur(33), b=0)
    ex("bgblur_in_place", blur(25), b=0, o=fr)
    ex("partial_overlap", 0, o=fr + 4096)
    ex("partial_overlap_bgblur_fused", blur(25), b=0, o=fr + 4096)
    ex("partial_overlap_bgblur_two_pass", blur(1), b=0, o=fr + 4096)
    ex("partial_overlap_no_mask", NOMASK, o=fr + 4096)
    streams("dup", [0, 1, 0])
    ex("unknown_flag_after_dup", 32)                    # a refusal right after another entry point's refusal reports its own reason
    pipe("bgblur_after_dup", blur(25))
    streams("out_of_range", [0, n])
    streams("negative_id", [1, -2])
    streams("n_too_big", list(range(n)) + [0])
    streams("negative_n", [0], nn=-1)
    streams("null_ids", [], nn=1)
    streams("unknown_flag", perm, 32)
    streams("null_bg", perm, b=0)
    streams("partial_overlap", perm, o=fr + 4096)
    streams("partial_overlap_bgblur", perm, blur(25), b=0, o=fr + 4096)
    streams("empty", [])
    vcam("null_frames", W // 2, H // 2, frames=0)
    vcam("no_mask", W // 2, H // 2, NOMASK)
    vcam("unknown_flag", W // 2, H // 2, 32)
    vcam("bgblur_even", W // 2, H // 2, blur(4), b=0)
    vcam("zero_size", 0, H // 2)
    vcam("odd_yuyv", W // 2 | 1, H // 2, YUYV)
    vcam("overlaps_frames", W // 2, H // 2, o=fr + 4096)
    vcam("overlaps_bg", W // 2, H // 2, o=bg)
    pipe("bgblur", blur(25))
    pipe("in_place", o=fr)
    pipe("partial_overlap", o=fr + 4096)
    pipe("n_too_big", nn=n + 1)
    pipe("null_bg", b=0)
    pipe("unknown_flag", 32)
    pipe("unaligned", o=out + 2)
    run("process_n0", lambda: L.bsx_process_batch(ctx, P(fr), 0, None, None))
    run("stage_bad", lambda: L.bsx_debug_run_stage(ctx, 7, P(fr), n, None))
    run("step_after_refusals", lambda: L.bsx_step_batch(ctx, P(fr), P(bg), 0, P(out), n, None))
    run("delete", lambda: L.bsx_delete(ctx) or 0)
    return calls


# ---- parent ---------------------------------------------------------------------------------------------------------------------------------------------------
def normalise(lines):
    """HIP log lines → trace entries: device-affine calls only, handles numbered by first use (null stream = s0)"""
    ids = {}

    def num(m):
        kind, v = m.group(1), m.group(2)
        if v in ("(nil)", "0x0", "0"):
            return "%s=0" % kind
        key = (kind, v)
        if key not in ids:
            ids[key] = sum(1 for k in ids if k[0] == kind) + 1
        return "%s=%d" % (kind, ids[key])
    out = []
    for l in lines:
        f = l.split(None, 3)
        if not f or f[0] == "neutral":
            continue
        note = re.sub(r"\b([se])=(\S+)", num, f[3]) if len(f) > 3 else ""
        out.append((f[0] + " " + f[1] + " " + note).strip())
    return out


def roi_sweep(model, sizes):
    """child, under the stub: one context per (W, H) of `sizes` → [[W, H, roi or None, in_roi or None]] (None: bsx_new refused the size)"""
    sys.path.insert(0, ROOT)
    from backscrub_amd import api
    L = C.CDLL(api.lib_path())
    for name, res, args in api.SYMBOLS:
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    out = []
    info = api._Info()
    for W, H in sizes:
        ctx = L.bsx_new(model.encode(), 2, W, H, 1, 0, api.DEBUG_FN(), api.STAGE_FN(), api.STAGE_FN(), api.STAGE_FN(), None)
        if not ctx:
            out.append([W, H, None, None])
            continue
        L.bsx_get_info(ctx, C.byref(info))
        out.append([W, H, list(info.roi), list(info.in_roi)])
        L.bsx_delete(ctx)
    return out


def configs(debug, sizes=None):
    if sizes is not None:                                       # the geometry audit: [(model, W, H)] or [(model, W, H, n_streams)]
        return [tuple(s[:3]) + ("",) + tuple(s[3:4]) for s in sizes]
    geo = [(m, W, H, "") for m in MODELS for W, H in GEOMETRIES]
    if debug:
        geo += [(m, 640, 480, sw) for sw in SWITCHES for m in MODELS]
    return geo


def trace_all(debug, n, only=None, sizes=None, brief=False):
    stub = build_stub()
    sys.path.insert(0, ROOT)
    from backscrub_amd import build as _b
    lib = os.environ.get("BSX_LIBRARY") or (_b.LIB_DBG if debug else _b.LIB)
    result = {}
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        for model, W, H, sw, *own_n in configs(debug, sizes):
            name = "%s %dx%d %s" % (model, W, H, sw or "-")
            if only and not re.search(only, name):
                continue
            log = os.path.join(tmp, "hip_%d.log" % len(result))
            env = dict(os.environ, LD_PRELOAD=stub, BSX_STUB_LOG=log, BSX_STUB_NDEV="1", BSX_LIBRARY=lib)
            nn = own_n[0] if own_n else n
            if sw:
                k, _, v = sw.partition("=")
                env[k] = v or "1"
                if k == "BSX_LANES":
                    nn = 16 * int(v)                 # lanes are taken from 16 streams per lane on
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", model_file(model), str(W), str(H), str(nn)] + (["--brief"] if brief else []), env=env,
                               capture_output=True, text=True, timeout=1800)
            if r.returncode != 0:
                raise RuntimeError("%s: child failed\n%s" % (name, r.stderr[-3000:]))
            d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
            if "error" in d:
                raise RuntimeError("%s: %s" % (name, d["error"]))
            logl = open(log).read().splitlines() if os.path.exists(log) else []
            info = d.pop("_info", None)
            result[name] = {k: {"rc": c["rc"], "error": c["error"], "trace": normalise(logl[c["log"][0]:c["log"][1]])} for k, c in d.items()}
            print("%-40s %3d calls, %6d HIP calls" % (name, len(d), sum(len(c["trace"]) for c in result[name].values())), file=sys.stderr)
            if info is not None:
                result[name]["_info"] = info
    return result


def diff(a, b):
    """(number of calls compared, [(config, call, what)] of the differences)"""
    out, count = [], 0
    for cfg in sorted(set(a) | set(b)):
        ca, cb = a.get(cfg), b.get(cfg)
        if ca is None or cb is None:
            out.append((cfg, "*", "configuration missing on one side"))
            continue
        for k in sorted(set(ca) | set(cb)):
            if k.startswith("_"):                                # "_info": the context's geometry, not a call
                continue
            count += 1
            x, y = ca.get(k), cb.get(k)
            if x is None or y is None:
                out.append((cfg, k, "call missing on one side"))
            elif x["rc"] != y["rc"]:
                out.append((cfg, k, "rc %d -> %d" % (x["rc"], y["rc"])))
            elif x["trace"] != y["trace"]:
                out.append((cfg, k, "trace: %d -> %d HIP calls" % (len(x["trace"]), len(y["trace"]))))
    return count, out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--child", nargs=4, metavar=("MODEL", "W", "H", "N"), help=argparse.SUPPRESS)
    ap.add_argument("--brief", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--roi-sweep", nargs=2, metavar=("MODEL", "SIZES_JSON"), help=argparse.SUPPRESS)
    ap.add_argument("--out", help="write the traces of the library BSX_LIBRARY names (default: the in-tree build) here")
    ap.add_argument("--debug", action="store_true", help="the debug library (libbsx_dbg.so by default), with every debug switch configuration")
    ap.add_argument("--only", help="regular expression: only the configurations whose name matches")
    ap.add_argument("--streams", type=int, default=4, help="streams per context (lanes configurations use 16 per lane)")
    ap.add_argument("--diff", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if a.child:
        print(json.dumps(drive(a.child[0], int(a.child[1]), int(a.child[2]), int(a.child[3]), a.brief)))
    elif a.roi_sweep:
        print(json.dumps(roi_sweep(a.roi_sweep[0], json.load(open(a.roi_sweep[1])))))
    elif a.diff:
        count, d = diff(json.load(open(a.diff[0])), json.load(open(a.diff[1])))
        for cfg, k, what in d:
            print("%-40s %-40s %s" % (cfg, k, what))
        print("%d calls compared, %d differ" % (count, len(d)))
    elif a.out:
        json.dump(trace_all(a.debug, a.streams, a.only), open(a.out, "w"), indent=0)
    else:
        ap.print_help()


if __name__ == "__main__":
    main()
