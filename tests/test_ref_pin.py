"""Pins the oracle to the REFERENCE'S OWN OBJECT CODE wherever the reference's arithmetic is in its tree.

oracle/_ref/libbs_ref.so = /root/reference/lib/libbackscrub.cc + lib/transpose_conv_bias.cc + app/deepseg.cc:87-134,
compiled unmodified (oracle/Makefile `ref-lib`) against API shims whose OpenCV / TFLite-builtin operations are served by
the oracle's restatement.  So every comparison below isolates reference code: bs_maskgen_* glue and geometry, the decode
loops + IIR, Convolution2DTransposeBias Prepare/Eval, alpha_blend, the YUYV packing loop.  Rows pinned: SURVEY §8 a1, a2,
a10-a14, a17, a19, a20, f1 (packing).  NOT pinned by this (third-party, absent from the checkout): cv::resize, cvtColor,
bilateralFilter, blur, convertTo and the TFLite builtin kernels (rows a3-a9, a15, a16, a18).

Where the reference's object code cannot be had (no oracle/_ref/libbs_ref.so and no reference checkout to build it from),
the reference side of every comparison is its recording: SHA-256 digests of the reference's results on the very same
inputs, in tests/golden/ref_pin_digests.json (tools/make_ref_pin.py, run where the library exists).  Where it can be had,
the reference runs live and is held to the recording as well.  The cases that run a network are recorded under the name of
the model file they ran (conftest.model_path: the reference's model where the repository has it, else the synthetic one)."""
import hashlib
import json
import os
import shutil
import tempfile

import numpy as np
import pytest

from conftest import ROOT, model_path
from oracle import oracle_py, ref_py

RECORDED = os.path.join(ROOT, "tests", "golden", "ref_pin_digests.json")
_RECORDING = None          # tools/make_ref_pin.py: a dict that collects the live reference results instead of checking them

GEOMS = [("mlkit", 640, 480), ("lite", 640, 480), ("mlkit", 1280, 720), ("full", 1280, 720), ("lite", 1280, 720), ("full", 640, 480),
         ("lite", 322, 242), ("lite", 160, 96)]
DECODE_KEYS = ["lite", "mlkit", "deeplab"]
TCONV = [(48, 80, 16, 2, 2, 2, 1), (16, 16, 16, 1, 2, 2, 1), (5, 7, 4, 3, 3, 2, 1), (5, 7, 4, 3, 3, 2, 2),
         (6, 5, 8, 2, 4, 2, 1), (4, 4, 3, 5, 3, 1, 1), (3, 9, 2, 2, 2, 3, 2), (7, 3, 5, 1, 5, 3, 1)]
YUYV = [(640, 480), (2, 2), (322, 242), (6, 1)]


def _frames(w, h, n, seed):
    from backscrub_amd import synth
    return [synth.frame(w, h, seed, t) for t in range(n)]


def _digest(*arrays):
    d = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        d.update(("%s%s;" % (a.dtype.str, a.shape)).encode())
        d.update(a.tobytes())
    return d.hexdigest()[:32]


def reference(case, live):
    """→ the digests of the reference object code's results for `case`: live() through oracle/_ref/libbs_ref.so where it can be had (and then held to the
    recording too), else the recording."""
    if _RECORDING is not None:
        _RECORDING[case] = live()
        return _RECORDING[case]
    with open(RECORDED) as f:
        rec = json.load(f).get(case)
    if not ref_py.available():
        assert rec is not None, "%s: no recording in tests/golden/ref_pin_digests.json (tools/make_ref_pin.py)" % case
        return rec
    got = live()
    assert rec is None or got == rec, "%s: the reference's object code no longer gives the recorded results (re-run tools/make_ref_pin.py if the inputs changed)" % case
    return got


def _ref_process(path, w, h, frames, forced=None):
    """bs_maskgen_new + one bs_maskgen_process per frame (forced: logits handed to the decode in place of the network's) → digest of (mask, ofinal) per call"""
    ref = ref_py.RefMaskGen(path, w, h)
    assert ref.ok()
    out = []
    for i, f in enumerate(frames):
        with np.errstate(all="ignore"):
            mask = ref.process(f, forced_output=None if forced is None else forced[i])
        assert mask is not None
        out.append(_digest(mask, ref.last_ofinal()))
    ref.close()
    return out


@pytest.mark.parametrize("key,w,h", GEOMS)
def test_whole_process_matches_reference_object_code(key, w, h):
    """bs_maskgen_new + 3 x bs_maskgen_process of the reference vs the oracle's Ctx: identical masks (geometry, state,
    decode+IIR, tconv inside the network, call order) on the SURVEY §8 frame x model pairs and two odd sizes."""
    path = model_path(key)
    frames = _frames(w, h, 3, seed=7)
    want = reference("whole_process/%s/%dx%d" % (os.path.basename(path), w, h), lambda: _ref_process(path, w, h, frames))
    oc = oracle_py.Ctx(path, w, h)
    q = oc.in_roidim
    got = []
    for f in frames:
        m = oc.process(f)
        got.append(_digest(m, oc.ofinal()[q[1]:q[1] + q[3], q[0]:q[0] + q[2]]))
    oc.close()
    assert got == want


def test_whole_process_deeplab_one_frame():
    path = model_path("deeplab")
    f = _frames(640, 480, 1, seed=3)[0]

    def live():
        ref = ref_py.RefMaskGen(path, 640, 480)
        m = ref.process(f)
        ref.close()
        return [_digest(m)]
    want = reference("whole_process/%s/640x480/1" % os.path.basename(path), live)
    oc = oracle_py.Ctx(path, 640, 480)
    assert [_digest(oc.process(f))] == want
    oc.close()


def _adversarial_logits(modeltype, shape, rng):
    n = int(np.prod(shape[:2]))
    if modeltype == 3:        # Meet: softmax-2 through expf — ties, 1-ulp gaps, overflow (inf/inf = NaN → 255), NaN, ±inf
        l0 = rng.normal(0, 4, n).astype(np.float32)
        l1 = l0.copy()
        k = n // 8
        l1[:k] = np.nextafter(l0[:k], np.float32(np.inf)); l1[k:2 * k] = np.nextafter(l0[k:2 * k], np.float32(-np.inf))
        l1[2 * k:3 * k] = l0[2 * k:3 * k] + rng.normal(0, 1e-4, k).astype(np.float32)
        l0[3 * k:4 * k] = rng.uniform(80, 100, k); l1[3 * k:4 * k] = rng.uniform(80, 100, k)      # expf overflow
        l0[4 * k:5 * k] = rng.uniform(-110, -90, k); l1[4 * k:5 * k] = rng.uniform(-110, -90, k)  # both underflow → 0/0
        l1[5 * k:6 * k] = rng.normal(0, 4, k)
        sp = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, 88.72284, 88.72283], np.float32)
        l0[6 * k:7 * k] = rng.choice(sp, k); l1[6 * k:7 * k] = rng.choice(sp, k)
        l1[7 * k:] = rng.normal(0, 4, n - 7 * k)
        return np.stack([l0, l1], -1).reshape(shape)
    if modeltype == 2:        # MLKit: p > 0.65 as a DOUBLE compare — floats around (float)0.65 and 0.65 itself
        p = rng.uniform(0, 1, n).astype(np.float32)
        f65 = np.float32(0.65)
        near = np.array([f65, np.nextafter(f65, np.float32(1)), np.nextafter(f65, np.float32(0)), np.nan, np.inf, -np.inf, 0.6500001, 0.6499999], np.float32)
        p[: n // 4] = rng.choice(near, n // 4)
        return p.reshape(shape)
    x = rng.normal(0, 3, (n, shape[2])).astype(np.float32)   # DeepLab: argmax, first max wins, init -10000
    k = n // 6
    x[:k, 15] = x[:k].max(1)                                  # person ties with an EARLIER or LATER class
    x[k:2 * k] = -20000.0                                     # everything below the -10000 initial value → maxpos stays 0
    x[2 * k:3 * k, 15] = np.nan
    x[3 * k:4 * k, 15] = 1e9
    x[4 * k:5 * k, 14] = x[4 * k:5 * k, 15] = 50.0            # tie 14 vs 15: 14 wins
    return x.reshape(shape)


@pytest.mark.parametrize("key", DECODE_KEYS)
def test_decode_and_iir_match_reference_loops(key):
    """lib/libbackscrub.cc:317-357 through the reference's object code on adversarial logits, 5 frames deep (the IIR state
    walks 0x00 → 0xE0 → 0xFC → 0xFF and back), vs oracle decode_iir; and the mask the reference builds from that state
    (ROI placement, persistent 255 border) vs the oracle's post stage."""
    path = model_path(key)
    w, h = 640, 480
    oc = oracle_py.Ctx(path, w, h)
    rng = np.random.default_rng(11)
    frame = _frames(w, h, 1, seed=1)[0]
    logits = [_adversarial_logits(oc.modeltype, (oc.outH, oc.outW, oc.outC), rng) for _ in range(5)]
    want = reference("decode_iir/%s" % os.path.basename(path), lambda: _ref_process(path, w, h, [frame] * 5, forced=logits))
    state = np.zeros((oc.outH, oc.outW), np.uint8)
    q = oc.in_roidim
    got = []
    for t in range(5):
        state = oracle_py.decode_iir(oc.modeltype, logits[t], state)
        oc.set_output(logits[t])
        got.append(_digest(oc.post(), state[q[1]:q[1] + q[3], q[0]:q[0] + q[2]]))
        assert np.array_equal(oc.ofinal(), state)
    oc.close()
    for t in range(5):
        assert got[t] == want[t], "frame %d" % t


@pytest.mark.parametrize("H,W,Ci,Co,k,s,padding", TCONV)
def test_transpose_conv_bias_matches_reference_op(H, W, Ci, Co, k, s, padding):
    """Convolution2DTransposeBias: the reference's registered Prepare (output shape, :118-186) + Eval (padding arithmetic and
    scatter loops, :188-256 → :37-114) vs the oracle restatement — shipped shapes (k = s = 2, SAME) and overlapping /
    padded / VALID geometries the shipped models never exercise.  Bit-exact: same loop order, same f32 accumulation."""
    rng = np.random.default_rng(H * 131 + W * 17 + k)
    x = rng.normal(0, 1, (1, H, W, Ci)).astype(np.float32)
    w = rng.normal(0, 0.5, (Co, k, k, Ci)).astype(np.float32)
    b = rng.normal(0, 1, Co).astype(np.float32)
    want = reference("tconv_bias/%d,%d,%d,%d,%d,%d,%d" % (H, W, Ci, Co, k, s, padding), lambda: [_digest(ref_py.tconv_bias(x, w, b, padding, (s, s)))])
    assert [_digest(oracle_py.tconv_bias(x, w, b, padding, (s, s)))] == want


def test_alpha_blend_all_byte_triples_match_reference():
    """app/deepseg.cc:108-134 on all 2^24 (bg, frame, mask) byte triples: reference object code == oracle."""
    a, b, m = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    m2 = m.reshape(4096, 4096)
    # channel 0 enumerates every (bg=a, frame=b, m); the other channels carry other pairings of the same mask byte
    bg = np.stack([a.reshape(4096, 4096), b.reshape(4096, 4096), (a ^ b).reshape(4096, 4096)], -1)
    fr = np.stack([b.reshape(4096, 4096), a.reshape(4096, 4096), (255 - a).reshape(4096, 4096)], -1)
    want = reference("alpha_blend/all_byte_triples", lambda: [_digest(ref_py.alpha_blend(bg, fr, m2))])
    assert [_digest(oracle_py.alpha_blend(bg, fr, m2))] == want


@pytest.mark.parametrize("w,h", YUYV)
def test_yuyv_packing_matches_reference(w, h):
    """convert_rgb_to_yuyv (app/deepseg.cc:87-106): split + 4:2:2 packing (Y0 V Y1 U, truncating chroma mean) are the
    reference's; the RGB2YUV colour matrix underneath is the oracle's OpenCV restatement on both sides."""
    rng = np.random.default_rng(w * 7 + h)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    edge = np.array([[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255], [254, 1, 128]], np.uint8)
    img[0, : min(w, 6)] = edge[: min(w, 6)]
    want = reference("yuyv/%dx%d" % (w, h), lambda: [_digest(ref_py.convert_rgb_to_yuyv(img))])
    assert [_digest(oracle_py.bgr_to_yuyv(img))] == want


@pytest.mark.skipif(not ref_py.available(), reason="the reference's own behaviour: needs oracle/_ref/libbs_ref.so or a reference checkout to build it from")
def test_reference_interface_behaviour():
    """Error / callback / aliasing behaviour of the reference itself, which tests/test_shim.py and test_cabi.py assert for
    the product: NULL on a missing file and on an unknown model name, false on a NULL context, callbacks in the order
    prep → infer → mask once per call, mask header aliasing one lib-owned buffer."""
    msgs = []
    assert not ref_py.RefMaskGen("/nonexistent/segm_x.tflite", 640, 480, ondebug=lambda c, m: msgs.append(m)).ok()
    assert msgs and b"unable to load model" in msgs[0]
    d = tempfile.mkdtemp()
    odd = os.path.join(d, "mystery.tflite")
    shutil.copy(model_path("lite"), odd)
    msgs.clear()
    assert not ref_py.RefMaskGen(odd, 640, 480, ondebug=lambda c, m: msgs.append(m)).ok()
    assert any(b"unknown model type" in m for m in msgs)
    shutil.rmtree(d)
    order = []
    ref = ref_py.RefMaskGen(model_path("lite"), 640, 480, onprep=lambda c: order.append("prep"), oninfer=lambda c: order.append("infer"),
                            onmask=lambda c: order.append("mask"))
    f = _frames(640, 480, 1, seed=2)[0]
    ref.process(f); p1 = ref.last_mask_ptr
    ref.process(f); p2 = ref.last_mask_ptr
    assert order == ["prep", "infer", "mask"] * 2
    assert p1 == p2 and p1
    ref.close()
    out = np.empty((480, 640), np.uint8)
    assert ref_py.lib().ref_maskgen_process(None, f.ctypes.data_as(ref_py._u8p), 640, 480, out.ctypes.data_as(ref_py._u8p), None) == 0
    assert b"2.8.0" in ref_py.lib().ref_tensorflow_version()
