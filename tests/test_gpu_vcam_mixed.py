"""bsx_step_batch_vcam_mixed on the GPU: a chosen subset of the streams, each with its own background, flip, blur and filter switch, written at the virtual
camera's geometry in one pass.  Every comparison between library calls is byte for byte (torch.equal): the operands are integer arithmetic the project already pins
— the new call against the dense vcam step, against step_mixed / step_streams followed by resize_bgr [and bgr_to_yuyv], and against itself through the other
kernel form; one case checks it against the CPU oracle with the bars of tests/test_gpu_mixed.py::test_one_stream_per_mode_matches_the_oracle."""
import ctypes

import numpy as np
import pytest

from conftest import model_path

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

VGA, HD = (640, 480), (1280, 720)
BATCH = ("yuyv", "yuyv_in")


@pytest.fixture(scope="module")
def bs():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    import backscrub_amd
    backscrub_amd.lib()
    return backscrub_amd


def _model(key):
    return model_path("deeplab", prefer_real=False) if key == "deeplab_synthetic" else model_path(key)


def _frames(W, H, streams, t):
    from backscrub_amd import synth
    out = []
    for s in streams:
        if (W, H) == VGA and s < 2:
            from tools import make_photo_fixture
            out.append(make_photo_fixture.load_frames()[s])
        else:
            out.append(synth.frame(W, H, s, t))
    return np.stack(out)


def _images(W, H, n, seed0=1):
    from backscrub_amd import synth
    return torch.from_numpy(np.stack([synth.background(W, H, seed=seed0 + s) for s in range(n)])).cuda()


def _out(n, W, H, yuyv):
    return torch.full((n, H, W, 2 if yuyv else 3), 0x5a, dtype=torch.uint8, device="cuda")


def _flip_code(fh, fv):
    return -1 if (fh and fv) else (1 if fh else 0)


# ---- 1. every stream on the same setting = the dense vcam step ----------------------------------------------------------------------------------------------
FLAGS = [{}, {"flip_h": True, "yuyv": True}, {"yuyv_in": True, "yuyv": True}, {"bgblur": 25}, {"bgblur": 25, "flip_v": True}]


@pytest.mark.parametrize("flags", FLAGS, ids=["plain", "flip_h_yuyv", "yuyv_in", "bgblur", "bgblur_flip_v"])
@pytest.mark.parametrize("key,res,vg,n", [("lite", VGA, (1280, 720), 6), ("lite", VGA, (426, 240), 6), ("lite", VGA, (320, 240), 6), ("mlkit", HD, (854, 480), 4),
                                          ("deeplab_synthetic", VGA, (320, 240), 4)])
def test_uniform_settings_equal_the_dense_vcam_step(bs, key, res, vg, n, flags):
    """ticks 0-2: every stream points at ONE image; ticks 3-5: each stream at its own image (the twin steps with the per-stream stride form)"""
    W, H = res
    ow, oh = vg
    path = _model(key)
    twin, mg = bs.MaskGen(path, W, H, n_streams=n), bs.MaskGen(path, W, H, n_streams=n)
    batch = {k: v for k, v in flags.items() if k in BATCH}
    stream = {k: v for k, v in flags.items() if k not in BATCH}
    shared, own = _images(W, H, 1)[0], _images(W, H, n, seed0=5)
    try:
        for t in range(6):
            per_stream = t >= 3
            bg = None if flags.get("bgblur") else (own if per_stream else shared)
            f = torch.from_numpy(_frames(W, H, range(n), t)).cuda()
            fr = twin.bgr_to_yuyv(f) if flags.get("yuyv_in") else f
            a, b = _out(n, ow, oh, flags.get("yuyv")), _out(n, ow, oh, flags.get("yuyv"))
            twin.step_vcam(fr, bg, a, **flags)
            st = [bs.StreamSetting(bg=None if bg is None else (bg[i] if per_stream else bg), **stream) for i in range(n)]
            mg.step_vcam_mixed(fr, b, st, **batch)
            assert torch.equal(a, b), "t=%d: outputs differ in %d bytes" % (t, int((a != b).sum()))
            assert torch.equal(twin.masks(), mg.masks()), "t=%d: persistent masks differ" % t
            assert torch.equal(twin.ofinal(), mg.ofinal()), "t=%d: temporal state differs" % t
    finally:
        twin.close()
        mg.close()


# ---- 2. a heterogeneous batch = step_mixed into a capture-size buffer, then resize_bgr [, bgr_to_yuyv] ---------------------------------------------------------
# per stream: (background: "own" / gallery index / None, stream flags)
KINDS = [("own", {}), (0, {}), (1, {"flip_h": True}), (2, {"flip_v": True}), ("own", {"flip_h": True, "flip_v": True}), (None, {"bgblur": 7}),
         (None, {"bgblur": 25}), (None, {"bgblur": 7, "flip_h": True}), (1, {"filter_off": True}), (None, {"filter_off": True, "flip_h": True}),
         (0, {"filter_off": True, "bgblur": 25, "flip_v": True}), (2, {})]


class _Pair:
    """mg: the new call; twin: step_mixed into a capture-size BGR buffer -> resize_bgr -> [bgr_to_yuyv]"""

    def __init__(self, api, path, W, H, vg, kinds):
        self.api, self.W, self.H, self.vg, self.kinds = api, W, H, vg, kinds
        n = len(kinds)
        self.mg, self.twin = api.MaskGen(path, W, H, n_streams=n), api.MaskGen(path, W, H, n_streams=n)
        self.own, self.gallery = _images(W, H, n, seed0=11), _images(W, H, 3, seed0=31)

    def bg_of(self, s):
        b = self.kinds[s][0]
        return None if b is None else (self.own[s] if b == "own" else self.gallery[b])

    def setting(self, s, **override):
        return self.api.StreamSetting(bg=self.bg_of(s), **dict(self.kinds[s][1], **override))

    def step(self, t, batch, perm=None, overrides=None):
        """the new call alone: its output"""
        W, H, (ow, oh), n = self.W, self.H, self.vg, len(self.kinds)
        overrides = overrides or {}
        order = list(range(n)) if perm is None else [int(i) for i in perm]
        f = torch.from_numpy(_frames(W, H, order, t)).cuda()
        fr = self.mg.bgr_to_yuyv(f) if batch.get("yuyv_in") else f
        out = _out(n, ow, oh, batch.get("yuyv"))
        sett = [self.setting(s, **overrides.get(s, {})) for s in order]
        self.mg.step_vcam_mixed(fr, out, sett, ids=None if perm is None else order, **batch)
        return order, fr, sett, out

    def tick(self, t, batch, perm=None, overrides=None, msg=""):
        W, H, (ow, oh), n = self.W, self.H, self.vg, len(self.kinds)
        order, fr, sett, out = self.step(t, batch, perm, overrides)
        full = _out(n, W, H, False)
        self.twin.step_mixed(fr, full, sett, ids=None if perm is None else order, yuyv_in=bool(batch.get("yuyv_in")))
        want = self.twin.resize_bgr(full, ow, oh)
        if batch.get("yuyv"):
            want = self.twin.bgr_to_yuyv(want)
        for i, s in enumerate(order):
            assert torch.equal(out[i], want[i]), "%s t=%d position %d (stream %d, %s): %d bytes differ" % (msg, t, i, s, sett[i], int((out[i] != want[i]).sum()))
        assert torch.equal(self.mg.masks(), self.twin.masks()), "%s t=%d: persistent masks differ" % (msg, t)
        assert torch.equal(self.mg.ofinal(), self.twin.ofinal()), "%s t=%d: temporal state differs" % (msg, t)
        return out

    def close(self):
        self.mg.close()
        self.twin.close()


BATCH_SETS = [{}, {"yuyv": True}, {"yuyv_in": True, "yuyv": True}]


@pytest.mark.parametrize("permuted", [False, True], ids=["dense", "ids"])
@pytest.mark.parametrize("batch", BATCH_SETS, ids=["plain", "yuyv", "yuyv_in"])
@pytest.mark.parametrize("key,res,vg", [("lite", VGA, (426, 240)), ("mlkit", HD, (854, 480))])
def test_a_heterogeneous_batch_equals_the_separate_calls(bs, key, res, vg, batch, permuted):
    W, H = res
    m = _Pair(bs, model_path(key), W, H, vg, KINDS)
    rng = np.random.default_rng(5)
    try:
        for t in range(3):
            m.tick(t, batch, perm=rng.permutation(len(KINDS)) if permuted else None)
    finally:
        m.close()


# ---- 3. a subset leaves the other streams alone ---------------------------------------------------------------------------------------------------------------
def test_a_subset_leaves_the_other_streams_alone(bs):
    W, H = VGA
    ow, oh = 426, 240
    path, n, ids = model_path("lite"), 8, [5, 1, 6]
    mg, twin = bs.MaskGen(path, W, H, n_streams=n), bs.MaskGen(path, W, H, n_streams=n)
    bgs = _images(W, H, len(ids), seed0=21)
    try:
        f0 = torch.from_numpy(_frames(W, H, range(n), 0)).cuda()
        full = _out(n, W, H, False)
        for g in (mg, twin):                                         # every stream has a state of its own before the subset steps
            g.step_ex(f0, bgs[0], full)
        torch.cuda.synchronize()
        masks0, of0 = mg.masks().clone(), mg.ofinal().clone()
        others = [s for s in range(n) if s not in ids]
        for t in range(1, 4):
            fr = torch.from_numpy(_frames(W, H, ids, t)).cuda()
            out = _out(len(ids), ow, oh, False)
            mg.step_vcam_mixed(fr, out, [bs.StreamSetting(bg=bgs[i]) for i in range(len(ids))], ids=ids)
            part = _out(len(ids), W, H, False)
            twin.step_streams(ids, fr, bgs, part)
            want = twin.resize_bgr(part, ow, oh)
            assert torch.equal(out, want), "t=%d: stepped streams differ from step_streams + resize_bgr" % t
            assert torch.equal(mg.masks()[others], masks0[others]) and torch.equal(mg.ofinal()[others], of0[others]), "t=%d: an untouched stream moved" % t
            assert torch.equal(mg.masks(), twin.masks()) and torch.equal(mg.ofinal(), twin.ofinal()), "t=%d: state differs from the twin's" % t
        assert not torch.equal(mg.masks()[ids], masks0[ids])
    finally:
        mg.close()
        twin.close()


# ---- 4. the filter switched off and on again ------------------------------------------------------------------------------------------------------------------
def test_filter_off_then_on_tracks_a_twin_that_never_switched(bs):
    """stream 3 (flip_v, gallery background) switches its filter off at tick 2 and on at tick 4 ('s' key): its state and mask follow a twin that never switched
    (step_vcam_mixed with the filter on throughout); while off its output is the flipped, resized frame — and nothing else about the batch changes"""
    W, H = VGA
    vg = (426, 240)
    m = _Pair(bs, model_path("lite"), W, H, vg, KINDS)
    never = bs.MaskGen(model_path("lite"), W, H, n_streams=len(KINDS))
    try:
        for t in range(6):
            off = 2 <= t < 4
            out = m.tick(t, {}, overrides={3: {"filter_off": True}} if off else {}, msg="toggle")
            fr = torch.from_numpy(_frames(W, H, range(len(KINDS)), t)).cuda()
            o2 = _out(len(KINDS), vg[0], vg[1], False)
            never.step_vcam_mixed(fr, o2, [m.setting(s) for s in range(len(KINDS))])
            assert torch.equal(m.mg.masks(), never.masks()) and torch.equal(m.mg.ofinal(), never.ofinal()), "t=%d: the switch moved the state" % t
            frame3 = never.resize_bgr(never.flip_bgr(fr[3:4].contiguous(), 0), vg[0], vg[1])[0]
            if off:
                assert torch.equal(out[3], frame3), "t=%d: filter off is not the flipped, resized frame" % t
            else:
                assert torch.equal(out[3], o2[3])
            keep = [s for s in range(len(KINDS)) if s != 3]
            assert torch.equal(out[keep], o2[keep])
    finally:
        m.close()
        never.close()


# ---- 5. a capture geometry the mixed step refuses ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("yuyv_in", [False, True], ids=["bgr", "yuyv_in"])
def test_a_capture_geometry_the_mixed_step_refuses(bs, yuyv_in):
    """lite at 322x242 (width not a multiple of 4): step_mixed refuses the context, the new call takes it — the byte-wise form of the kernel — and equals
    step_streams + flip_bgr + resize_bgr per settings group"""
    from backscrub_amd import api
    W, H = 322, 242
    ow, oh = 640, 480
    path = model_path("lite")
    kinds = [(0, {}), (1, {"flip_h": True}), (None, {"bgblur": 7}), (None, {"filter_off": True, "flip_v": True}), (0, {"flip_h": True, "flip_v": True})]
    n = len(kinds)
    mg, twin = bs.MaskGen(path, W, H, n_streams=n), bs.MaskGen(path, W, H, n_streams=n)
    gallery = _images(W, H, 2, seed0=51)
    order = [3, 0, 4, 1, 2]
    try:
        for t in range(3):
            f = torch.from_numpy(_frames(W, H, order, t)).cuda()
            fr = twin.bgr_to_yuyv(f) if yuyv_in else f
            sett = [bs.StreamSetting(bg=None if kinds[s][0] is None else gallery[kinds[s][0]], **kinds[s][1]) for s in order]
            if t == 0:
                with pytest.raises(api.BsxError, match="geometry"):
                    mg.step_mixed(fr, _out(n, W, H, False), sett, ids=order, yuyv_in=yuyv_in)
            out = _out(n, ow, oh, False)
            mg.step_vcam_mixed(fr, out, sett, ids=order, yuyv_in=yuyv_in)
            for i, s in enumerate(order):                            # the twin: one stream per call
                kf = dict(kinds[s][1])
                off, fh, fv = kf.pop("filter_off", False), kf.pop("flip_h", False), kf.pop("flip_v", False)
                bg = None if kf.get("bgblur") else (gallery[0] if kinds[s][0] is None else gallery[kinds[s][0]])
                part = _out(1, W, H, False)
                twin.step_streams([s], fr[i:i + 1].contiguous(), bg, part, yuyv_in=yuyv_in, **kf)
                C = (twin.yuyv_to_bgr(fr[i:i + 1].contiguous()) if yuyv_in else f[i:i + 1].contiguous()) if off else part
                F = twin.flip_bgr(C, _flip_code(fh, fv)) if (fh or fv) else C
                want = twin.resize_bgr(F.contiguous(), ow, oh)[0]
                assert torch.equal(out[i], want), "t=%d position %d (stream %d): %d bytes differ" % (t, i, s, int((out[i] != want).sum()))
            assert torch.equal(mg.masks(), twin.masks()) and torch.equal(mg.ofinal(), twin.ofinal()), "t=%d: state differs" % t
    finally:
        mg.close()
        twin.close()


def test_an_unaligned_background_takes_the_byte_form_for_its_stream(bs):
    """d_bg at an odd address (the mixed step refuses it): same bytes as the aligned copy of the image"""
    W, H = VGA
    path = model_path("lite")
    mg, twin = bs.MaskGen(path, W, H, n_streams=3), bs.MaskGen(path, W, H, n_streams=3)
    img = _images(W, H, 2, seed0=61)
    raw = torch.zeros(W * H * 3 + 8, dtype=torch.uint8, device="cuda")
    odd = raw[1:1 + W * H * 3].view(H, W, 3)
    odd.copy_(img[1])
    assert odd.data_ptr() % 4 == 1
    try:
        fr = torch.from_numpy(_frames(W, H, range(3), 0)).cuda()
        a, b = _out(3, 426, 240, True), _out(3, 426, 240, True)
        mg.step_vcam_mixed(fr, a, [bs.StreamSetting(bg=img[0]), bs.StreamSetting(bg=odd, flip_h=True), bs.StreamSetting(bg=img[0], flip_v=True)], yuyv=True)
        twin.step_vcam_mixed(fr, b, [bs.StreamSetting(bg=img[0]), bs.StreamSetting(bg=img[1], flip_h=True), bs.StreamSetting(bg=img[0], flip_v=True)], yuyv=True)
        assert torch.equal(a, b) and torch.equal(mg.masks(), twin.masks())
    finally:
        mg.close()
        twin.close()


# ---- 6. the direct-tap form -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [{}, {"yuyv_in": True, "yuyv": True}], ids=["plain", "yuyv_in"])
def test_direct_tap_form_equals_the_lds_form(bs, debug_switches, monkeypatch, batch):
    """BSX_VCAM_DIRECT (debug library) forces the per-tap form on a table whose footprints fit LDS: the heterogeneous batch gives the same bytes either way"""
    W, H = VGA
    res = []
    rng = np.random.default_rng(7)
    perm = rng.permutation(len(KINDS))
    for env in (None, "1"):
        if env:
            monkeypatch.setenv("BSX_VCAM_DIRECT", env)
        m = _Pair(debug_switches, model_path("lite"), W, H, (426, 240), KINDS)
        try:
            outs = []
            for t in range(2):
                outs.append(m.step(t, batch, perm=perm)[3].cpu())
            torch.cuda.synchronize()
            res.append(outs)
        finally:
            m.close()
    for a, b in zip(*res):
        assert torch.equal(a, b)


# ---- 7. equal sizes -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [{}, {"yuyv": True}], ids=["plain", "yuyv"])
def test_at_the_capture_size_the_call_is_step_mixed(bs, batch):
    from backscrub_amd import api
    W, H = VGA
    m = _Pair(bs, model_path("lite"), W, H, VGA, KINDS)
    rng = np.random.default_rng(9)
    try:
        for t in range(3):
            perm = rng.permutation(len(KINDS)) if t else None
            order, fr, sett, out = m.step(t, batch, perm)
            want = _out(len(KINDS), W, H, batch.get("yuyv"))
            m.twin.step_mixed(fr, want, sett, ids=None if perm is None else order, **batch)
            assert torch.equal(out, want), "t=%d" % t
            assert torch.equal(m.mg.masks(), m.twin.masks()) and torch.equal(m.mg.ofinal(), m.twin.ofinal())
    finally:
        m.close()
    odd = bs.MaskGen(model_path("lite"), 322, 242, n_streams=1)          # ... with that call's own refusals
    try:
        fr = torch.zeros((1, 242, 322, 3), dtype=torch.uint8, device="cuda")
        with pytest.raises(api.BsxError, match="geometry"):
            odd.step_vcam_mixed(fr, torch.empty_like(fr), [bs.StreamSetting(filter_off=True)])
    finally:
        odd.close()


# ---- 8. against the CPU oracle --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vg", [(426, 240), (1280, 720)], ids=["426x240", "1280x720"])
def test_one_stream_per_mode_matches_the_oracle(bs, oracle, vg):
    """lite VGA, one stream per mode, against the CPU oracle's stateful sequence of that stream's frames: the oracle's composite, flipped, resized by the oracle's own
    resize_linear.  The bars are those of tests/test_gpu_mixed.py::test_one_stream_per_mode_matches_the_oracle: mask IoU >= 0.999; a filter-off stream exact;
    the output exact where the masks agree and within 1 everywhere.  "Where the masks agree" for an output pixel: every source pixel of its taps agrees — the
    oracle's resize of the (flipped) disagreement map, widened by one pixel to every side so that a tap whose weight rounds to nothing still counts, is 0 there."""
    W, H = VGA
    ow, oh = vg
    path = model_path("lite")
    modes = [{"bg": 0}, {"bgblur": 7}, {"bg": 1, "flip_h": True, "flip_v": True}, {"bg": 0, "filter_off": True, "flip_h": True}, {"bg": 1, "flip_v": True}]
    n = len(modes)
    mg = bs.MaskGen(path, W, H, n_streams=n)
    oc = [oracle.Ctx(path, W, H) for _ in range(n)]
    gallery = _images(W, H, 2, seed0=41)
    g_np = gallery.cpu().numpy()
    failures = []
    try:
        for t in range(4):
            frames = _frames(W, H, range(n), t)
            sett = [bs.StreamSetting(bg=gallery[m["bg"]] if "bg" in m else None, **{k: v for k, v in m.items() if k != "bg"}) for m in modes]
            out = _out(n, ow, oh, False)
            mg.step_vcam_mixed(torch.from_numpy(frames).cuda(), out, sett)
            got_m, got_o = mg.masks().cpu().numpy(), out.cpu().numpy()
            for s, m in enumerate(modes):
                want_m = oc[s].process(frames[s])
                if m.get("filter_off"):
                    C = frames[s]
                else:
                    bg = oracle.gaussian_blur(frames[s], m["bgblur"]) if m.get("bgblur") else g_np[m["bg"]]
                    C = oracle.alpha_blend(bg, frames[s], want_m)
                fh, fv = m.get("flip_h", False), m.get("flip_v", False)
                flip = (lambda a: oracle.flip_bgr(np.ascontiguousarray(a), _flip_code(fh, fv))) if (fh or fv) else (lambda a: a)
                want_o = oracle.resize_linear(np.ascontiguousarray(flip(C)), ow, oh)
                fa, fb = got_m[s] < 128, want_m < 128
                union = np.logical_or(fa, fb).sum()
                iou = 1.0 if union == 0 else np.logical_and(fa, fb).sum() / union
                diff = np.abs(got_o[s].astype(np.int16) - want_o.astype(np.int16)).max(-1)
                if m.get("filter_off"):
                    agree_max = int(diff.max())
                else:
                    dis = got_m[s] != want_m
                    wide = dis.copy()                                # one pixel to every side
                    for dy in (-1, 0, 1):
                        for dx in (-1, 0, 1):
                            wide[max(dy, 0):H + min(dy, 0), max(dx, 0):W + min(dx, 0)] |= dis[max(-dy, 0):H + min(-dy, 0), max(-dx, 0):W + min(-dx, 0)]
                    dmap = np.repeat((wide.astype(np.uint8) * 255)[..., None], 3, -1)
                    same = oracle.resize_linear(np.ascontiguousarray(flip(dmap)), ow, oh)[..., 0] == 0
                    agree_max = int(diff[same].max(initial=0))
                print("tick %d stream %d %s: IoU %.5f, max diff where the masks agree %d, max diff %d" % (t, s, m, iou, agree_max, int(diff.max())))
                if iou < 0.999:
                    failures.append("tick %d stream %d: IoU %.5f" % (t, s, iou))
                if agree_max != 0:
                    failures.append("tick %d stream %d: output differs by %d where the masks agree%s" % (t, s, agree_max, " (filter off)" if m.get("filter_off") else ""))
                if int(diff.max()) > 1:
                    failures.append("tick %d stream %d: max diff %d" % (t, s, int(diff.max())))
    finally:
        for c in oc:
            c.close()
        mg.close()
    assert not failures, "\n".join(failures)


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_position_and_value_and_leave_the_state_alone(bs):
    from backscrub_amd import api
    W, H = VGA
    path = model_path("lite")
    n = 4
    mg, twin = bs.MaskGen(path, W, H, n_streams=n), bs.MaskGen(path, W, H, n_streams=n)
    L = api.lib()
    S = api._StreamSetting
    fr = torch.from_numpy(_frames(W, H, range(n), 0)).cuda()
    bg = _images(W, H, 1, seed0=71)[0]
    out = _out(n, 426, 240, False)
    good = [bs.StreamSetting(bg=bg) for _ in range(n)]
    P = lambda t: ctypes.c_void_p(t.data_ptr())                       # noqa: E731

    def settings(*over):
        """n valid settings with (position, d_bg, flags) overrides"""
        st = (S * n)()
        for i in range(n):
            st[i].d_bg, st[i].flags = bg.data_ptr(), 0
        for i, p, f in over:
            st[i].d_bg, st[i].flags = p, f
        return st

    def ids(*v):
        return (ctypes.c_int * max(len(v), 1))(*v)

    try:
        mg.step_vcam_mixed(fr, out, good)
        twin.step_vcam_mixed(fr, out, good)
        torch.cuda.synchronize()
        masks0, of0 = mg.masks().clone(), mg.ofinal().clone()
        s = api._stream_ptr()
        ok = settings()
        # (ids, frames, settings, out, out_w, out_h, n, flags) -> what the message must contain
        calls = [
            ((ids(0, 1, 1, 2), P(fr), ok, P(out), 426, 240, 4, 0), ["ids[2] = 1", "repeats ids[1]"]),
            ((ids(0, 1, 7, 2), P(fr), ok, P(out), 426, 240, 4, 0), ["ids[2] = 7", "out of range"]),
            ((ids(0, 1, -1, 2), P(fr), ok, P(out), 426, 240, 4, 0), ["ids[2] = -1"]),
            ((ids(0), P(fr), ok, P(out), 426, 240, -1, 0), ["n = -1"]),
            ((ids(0), P(fr), ok, P(out), 426, 240, 5, 0), ["n = 5", "4 streams"]),
            ((None, P(fr), ok, P(out), 426, 240, 5, 0), ["n = 5", "4 streams"]),
            ((None, P(fr), ok, P(out), 426, 240, -2, 0), ["n = -2"]),
            ((None, P(fr), None, P(out), 426, 240, 4, 0), ["settings is NULL"]),
            ((None, P(fr), settings((2, bg.data_ptr(), 1)), P(out), 426, 240, 4, 0), ["settings[2]", "0x1"]),          # a batch bit in a stream's flags
            ((None, P(fr), settings((1, bg.data_ptr(), 8)), P(out), 426, 240, 4, 0), ["settings[1]", "0x8"]),
            ((None, P(fr), ok, P(out), 426, 240, 4, 2), ["0x2"]),                                                       # a stream bit in the batch's flags
            ((None, P(fr), ok, P(out), 426, 240, 4, 0x1900), ["0x1900"]),
            ((None, P(fr), ok, P(out), 426, 240, 4, 8), ["0x8", "no-mask"]),                                            # BSX_STEP_NO_MASK
            ((None, P(fr), ok, P(out), W, H, 4, 8), ["0x8", "no-mask"]),                                                # ... at the capture size too
            ((None, P(fr), settings((3, None, 8 << 8)), P(out), 426, 240, 4, 0), ["settings[3]", "blur size 8"]),
            ((None, P(fr), settings((0, None, 33 << 8)), P(out), 426, 240, 4, 0), ["settings[0]", "blur size 33"]),
            ((None, P(fr), settings((1, None, 32 | (4 << 8))), P(out), 426, 240, 4, 0), ["settings[1]", "blur size 4"]),  # filter off: the size must still be valid
            ((None, P(fr), settings((2, None, 2)), P(out), 426, 240, 4, 0), ["settings[2]", "d_bg is NULL"]),
            ((None, P(fr), ok, P(out), 0, 240, 4, 0), ["0 x 240"]),
            ((None, P(fr), ok, P(out), 426, -3, 4, 0), ["426 x -3"]),
            ((None, P(fr), ok, P(out), 425, 240, 4, 1), ["even width", "425"]),
            ((None, P(fr), ok, P(fr), 320, 240, 4, 0), ["overlaps the frames"]),
            ((None, P(fr), ok, ctypes.c_void_p(fr.data_ptr() + 1000), 320, 240, 4, 0), ["overlaps the frames"]),
            ((None, P(fr), settings((2, bg.data_ptr(), 4)), P(bg), 160, 120, 4, 0), ["settings[0]", "overlaps the background", "%x" % bg.data_ptr()]),
            ((None, P(fr), settings((0, None, 32), (1, None, 7 << 8), (3, None, 32)), ctypes.c_void_p(bg.data_ptr() + 3000), 160, 120, 4, 0),
             ["settings[2]", "overlaps the background"]),
            ((None, None, ok, P(out), 426, 240, 4, 0), ["null buffer"]),
        ]
        for args, needles in calls:
            rc = L.bsx_step_batch_vcam_mixed(mg.h, *args[:7], s, args[7])
            msg = (L.bsx_last_error(mg.h) or b"").decode()
            assert rc == -1, (args[4:], rc)                          # BSX_EINVAL
            assert "bsx_step_batch_vcam_mixed" in msg or "no-mask" in msg, msg
            for needle in needles:
                assert needle in msg, "%r not in %r" % (needle, msg)
        with pytest.raises(api.BsxError, match="out"):
            mg.step_vcam_mixed(fr, torch.empty((n, 240, 425, 2), dtype=torch.uint8, device="cuda"), good, yuyv=True)
        torch.cuda.synchronize()
        assert torch.equal(mg.masks(), masks0) and torch.equal(mg.ofinal(), of0)
        # n == 0: a no-op
        assert L.bsx_step_batch_vcam_mixed(mg.h, None, None, None, None, 426, 240, 0, s, 0) == 0
        mg.step_vcam_mixed(fr[:0], out, [], ids=[])
        torch.cuda.synchronize()
        assert torch.equal(mg.masks(), masks0) and torch.equal(mg.ofinal(), of0)
        # the next valid step matches the twin that saw no failed calls
        fr1 = torch.from_numpy(_frames(W, H, range(n), 1)).cuda()
        o1, o2 = torch.empty_like(out), torch.empty_like(out)
        mg.step_vcam_mixed(fr1, o1, good)
        twin.step_vcam_mixed(fr1, o2, good)
        torch.cuda.synchronize()
        assert torch.equal(o1, o2) and torch.equal(mg.masks(), twin.masks()) and torch.equal(mg.ofinal(), twin.ofinal())
    finally:
        mg.close()
        twin.close()


def test_refuses_an_odd_yuyv_capture_and_a_pending_composite(bs):
    from backscrub_amd import api
    path = model_path("lite")
    odd = bs.MaskGen(path, 321, 240, n_streams=1)
    try:
        fr = torch.zeros((1, 240, 321, 2), dtype=torch.uint8, device="cuda")
        out = torch.empty((1, 120, 160, 3), dtype=torch.uint8, device="cuda")
        with pytest.raises(api.BsxError, match="even capture width.*321"):
            odd.step_vcam_mixed(fr, out, [bs.StreamSetting(filter_off=True)], yuyv_in=True)
    finally:
        odd.close()
    W, H = VGA
    mg = bs.MaskGen(path, W, H, n_streams=2)
    try:
        fr = torch.from_numpy(_frames(W, H, range(2), 0)).cuda()
        bg = _images(W, H, 1)[0]
        full = torch.empty((2, H, W, 3), dtype=torch.uint8, device="cuda")
        mg.step_pipelined(fr, bg, full)
        small = torch.empty((2, 240, 320, 3), dtype=torch.uint8, device="cuda")
        with pytest.raises(api.BsxError, match="pending"):
            mg.step_vcam_mixed(fr, small, [bs.StreamSetting(bg=bg)] * 2)
        with pytest.raises(api.BsxError, match="pending"):
            mg.step_vcam_mixed(fr[:0], small, [], ids=[])
        mg.flush_pipelined()
        torch.cuda.synchronize()
    finally:
        mg.close()
