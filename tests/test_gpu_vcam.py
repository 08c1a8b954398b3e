"""bsx_step_batch_vcam on the GPU: the main loop at the virtual camera's geometry (blend → flip → resize → YUYV pack, app/deepseg.cc:634-681) in one pass.

Every case runs two contexts over the same moving frame sequence: context A the separate calls (bsx_step_batch_ex → bsx_resize_bgr [→ bsx_bgr_to_yuyv]),
context B MaskGen.step_vcam.  B's output must equal A's byte for byte and the CPU oracle's resize_linear(flip(C)) [→ bgr_to_yuyv] of A's composite C, and the
persistent masks of the two contexts must be equal after every step.
"""
import ctypes

import numpy as np
import pytest

from conftest import model_path

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

VGA, HD = (640, 480), (1280, 720)
T = 3                                                   # steps: the temporal state is exercised


@pytest.fixture(scope="module")
def bs():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    import backscrub_amd
    backscrub_amd.lib()
    return backscrub_amd


def _frames(W, H, n, t, distinct=None):
    from backscrub_amd import synth
    base = [synth.frame(W, H, s, t) for s in range(min(n, distinct or n))]
    return np.stack([base[s % len(base)] for s in range(n)])


def _flip_code(fh, fv):
    return -1 if fh and fv else (1 if fh else 0)


def _run(bs, oracle, key, res, vg, n=2, fh=False, fv=False, yuyv=False, yuyv_in=False, bgblur=0, distinct=None):
    from backscrub_amd import synth
    W, H = res
    ow, oh = vg
    path = model_path(key)
    a = bs.MaskGen(path, W, H, n_streams=n)
    b = bs.MaskGen(path, W, H, n_streams=n)
    bg_h = synth.background(W, H)
    d_bg = None if bgblur else torch.from_numpy(bg_h).cuda()
    full = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
    out = torch.empty((n, oh, ow, 2 if yuyv else 3), dtype=torch.uint8, device="cuda")
    outs = []
    try:
        for t in range(T):
            host = _frames(W, H, n, t, distinct)
            if yuyv_in:
                host = np.stack([oracle.bgr_to_yuyv(f) for f in host])        # any 4:2:2 bytes will do: both contexts read the same ones
            d_fr = torch.from_numpy(host).cuda()
            a_in = a.yuyv_to_bgr(d_fr) if yuyv_in else d_fr                    # A: the BGR call on the converted frames
            a.step_ex(a_in, d_bg, full, flip_h=fh, flip_v=fv, bgblur=bgblur)
            ra = a.resize_bgr(full, ow, oh) if (ow, oh) != (W, H) else full.clone()
            want = a.bgr_to_yuyv(ra) if yuyv else ra
            out.fill_(0x5a)
            b.step_vcam(d_fr, d_bg, out, flip_h=fh, flip_v=fv, yuyv=yuyv, yuyv_in=yuyv_in, bgblur=bgblur)
            torch.cuda.synchronize()
            assert torch.equal(out, want), "step %d: vcam output differs from the separate calls in %d bytes" % (t, int((out != want).sum()))
            assert torch.equal(a.masks(), b.masks()), "step %d: persistent masks differ" % t
            fa = full.cpu().numpy()
            got = out.cpu().numpy()
            for i in range(min(n, 2)):
                C = oracle.flip_bgr(fa[i], _flip_code(fh, fv)) if (fh or fv) else fa[i]      # A's composite, unflipped
                ref = oracle.resize_linear(oracle.flip_bgr(C, _flip_code(fh, fv)) if (fh or fv) else C, ow, oh)
                if yuyv:
                    ref = oracle.bgr_to_yuyv(ref)
                assert np.array_equal(got[i], ref), "step %d stream %d: differs from the oracle in %d bytes" % (t, i, int((got[i] != ref).sum()))
            outs.append(got)
    finally:
        a.close()
        b.close()
    return outs


@pytest.mark.parametrize("key,res,vg", [("lite", VGA, (1280, 720)), ("lite", VGA, (320, 240)), ("lite", VGA, (426, 240)), ("lite", VGA, (160, 120)),
                                        ("mlkit", HD, (640, 360)), ("mlkit", HD, (854, 480)), ("mlkit", HD, (1920, 1080)), ("mlkit", HD, (160, 90)),
                                        ("lite", (322, 242), (640, 480))])
def test_vcam_step_equals_the_separate_calls_and_the_oracle(bs, oracle, key, res, vg):
    _run(bs, oracle, key, res, vg)


@pytest.mark.parametrize("key,res,vg", [("lite", VGA, (426, 240)), ("mlkit", HD, (854, 480))])
@pytest.mark.parametrize("fh,fv", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("yuyv", [False, True])
def test_vcam_step_flips_before_it_resizes(bs, oracle, key, res, vg, fh, fv, yuyv):
    _run(bs, oracle, key, res, vg, fh=fh, fv=fv, yuyv=yuyv)


@pytest.mark.parametrize("yuyv", [False, True])
@pytest.mark.parametrize("fh", [False, True])
def test_vcam_step_at_the_capture_size_is_step_ex(bs, oracle, fh, yuyv):
    _run(bs, oracle, "lite", VGA, VGA, fh=fh, yuyv=yuyv)


@pytest.mark.parametrize("key,res,vg", [("lite", VGA, (1280, 720)), ("mlkit", HD, (854, 480))])
def test_vcam_step_takes_yuyv_frames(bs, oracle, key, res, vg):
    _run(bs, oracle, key, res, vg, yuyv_in=True, fh=True, yuyv=True)


def test_vcam_step_with_a_blurred_background(bs, oracle):
    _run(bs, oracle, "lite", VGA, (426, 240), bgblur=25, fh=True)


def test_vcam_step_of_64_streams_matches_every_scene_twin(bs, oracle):
    outs = _run(bs, oracle, "lite", VGA, (854, 480), n=64, fv=True, yuyv=True, distinct=4)
    for got in outs:
        for i in range(4, 64):
            assert np.array_equal(got[i], got[i % 4]), "stream %d differs from its scene twin %d" % (i, i % 4)


def test_vcam_direct_tap_path_equals_the_lds_path(bs, debug_switches, monkeypatch):
    """BSX_VCAM_DIRECT (debug library) forces the per-tap form on a table whose footprints fit LDS: same bytes as the staged form."""
    from backscrub_amd import synth
    W, H = VGA
    path = model_path("lite")
    fr = torch.from_numpy(_frames(W, H, 2, 0)).cuda()
    bg = torch.from_numpy(synth.background(W, H)).cuda()
    res = []
    for env in (None, "1"):
        if env:
            monkeypatch.setenv("BSX_VCAM_DIRECT", env)
        mg = debug_switches.MaskGen(path, W, H, n_streams=2)
        try:
            out = torch.empty((2, 240, 426, 2), dtype=torch.uint8, device="cuda")
            mg.step_vcam(fr, bg, out, flip_h=True, yuyv=True)
            torch.cuda.synchronize()
            res.append(out.cpu())
        finally:
            mg.close()
    assert torch.equal(res[0], res[1])


def test_vcam_step_argument_errors_leave_the_state_alone(bs):
    from backscrub_amd import api, synth
    W, H = VGA
    path = model_path("lite")
    mg = bs.MaskGen(path, W, H, n_streams=2)
    twin = bs.MaskGen(path, W, H, n_streams=2)
    L = api.lib()
    fr = torch.from_numpy(_frames(W, H, 2, 0)).cuda()
    bg = torch.from_numpy(synth.background(W, H)).cuda()
    out = torch.empty((2, 240, 426, 3), dtype=torch.uint8, device="cuda")
    try:
        mg.step_vcam(fr, bg, out)
        twin.step_vcam(fr, bg, out)
        torch.cuda.synchronize()
        masks0 = mg.masks().clone()
        s = api._stream_ptr()
        P = lambda t: ctypes.c_void_p(t.data_ptr())                                   # noqa: E731
        calls = [(P(fr), P(bg), 0, P(out), 426, 240, 2, 8),                           # BSX_STEP_NO_MASK
                 (P(fr), P(bg), 0, P(out), 0, 240, 2, 0), (P(fr), P(bg), 0, P(out), 426, -1, 2, 0),
                 (P(fr), P(bg), 0, P(out), 425, 240, 2, 1),                           # odd YUYV width
                 (P(fr), P(bg), 0, P(fr), 320, 240, 2, 0),                            # out overlaps the frames
                 (P(fr), P(bg), 0, ctypes.c_void_p(fr.data_ptr() + 1000), 320, 240, 2, 0),
                 (P(fr), P(bg), 0, P(bg), 320, 240, 2, 0),                            # out overlaps the background
                 (P(fr), P(bg), 0, ctypes.c_void_p(bg.data_ptr() + 3000), 160, 120, 2, 0)]
        for fp, bp, stride, op, ow, oh, n, flags in calls:
            rc = L.bsx_step_batch_vcam(mg.h, fp, bp, stride, op, ow, oh, n, s, flags)
            assert rc != 0, (ow, oh, flags)
        with pytest.raises(api.BsxError):
            mg.step_vcam(fr, bg, torch.empty((2, 240, 425, 2), dtype=torch.uint8, device="cuda"), yuyv=True)
        torch.cuda.synchronize()
        assert torch.equal(mg.masks(), masks0)
        # the temporal state did not move either: the next valid step matches the twin that saw no failed calls
        fr1 = torch.from_numpy(_frames(W, H, 2, 1)).cuda()
        o1, o2 = torch.empty_like(out), torch.empty_like(out)
        mg.step_vcam(fr1, bg, o1)
        twin.step_vcam(fr1, bg, o2)
        torch.cuda.synchronize()
        assert torch.equal(o1, o2) and torch.equal(mg.masks(), twin.masks())
    finally:
        mg.close()
        twin.close()


def test_vcam_step_refuses_odd_yuyv_capture_and_a_pending_composite(bs):
    from backscrub_amd import api, synth
    path = model_path("lite")
    odd = bs.MaskGen(path, 321, 240, n_streams=1)
    try:
        fr = torch.zeros((1, 240, 321, 3), dtype=torch.uint8, device="cuda")
        out = torch.empty((1, 120, 160, 3), dtype=torch.uint8, device="cuda")
        bg = torch.zeros((240, 321, 3), dtype=torch.uint8, device="cuda")
        rc = api.lib().bsx_step_batch_vcam(odd.h, ctypes.c_void_p(fr.data_ptr()), ctypes.c_void_p(bg.data_ptr()), 0, ctypes.c_void_p(out.data_ptr()),
                                           160, 120, 1, api._stream_ptr(), 16)
        assert rc != 0
    finally:
        odd.close()
    W, H = VGA
    mg = bs.MaskGen(path, W, H, n_streams=2)
    try:
        fr = torch.from_numpy(_frames(W, H, 2, 0)).cuda()
        bg = torch.from_numpy(synth.background(W, H)).cuda()
        full = torch.empty((2, H, W, 3), dtype=torch.uint8, device="cuda")
        mg.step_pipelined(fr, bg, full)
        with pytest.raises(api.BsxError, match="pending"):
            mg.step_vcam(fr, bg, torch.empty((2, 240, 320, 3), dtype=torch.uint8, device="cuda"))
        mg.flush_pipelined()
        torch.cuda.synchronize()
    finally:
        mg.close()
