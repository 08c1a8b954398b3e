"""bsx_step_batch_mixed on the GPU: a batch whose streams each carry their own background, flip, blur and filter switch, stepped in ONE call, is bit-identical per
stream to what the entry points with one setting per call produce — byte-for-byte comparisons of composites, persistent masks and temporal state (`ofinal`) over
several ticks, on the moving synthetic scenes and (at 640x480) the real webcam frames of the photo fixture (streams 0-1)."""
import numpy as np
import pytest

from conftest import model_path

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

VGA, HD = (640, 480), (1280, 720)
FLAGS = [{}, {"yuyv": True, "flip_h": True}, {"no_mask": True}, {"yuyv_in": True, "yuyv": True}, {"bgblur": 25}, {"bgblur": 25, "flip_v": True}]
BATCH = ("yuyv", "no_mask", "yuyv_in")


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
    return torch.zeros((n, H, W, 2 if yuyv else 3), dtype=torch.uint8, device="cuda")


def _split(flags):
    batch = {k: v for k, v in flags.items() if k in BATCH}
    stream = {k: v for k, v in flags.items() if k not in BATCH}
    return batch, stream


# ---- 1. every stream on the same setting = the dense step_ex -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS, ids=["plain", "yuyv_flip_h", "no_mask", "yuyv_in", "bgblur", "bgblur_flip_v"])
@pytest.mark.parametrize("key,res,n", [("lite", VGA, 8), ("mlkit", HD, 4), ("deeplab_synthetic", VGA, 4), ("full", HD, 4)])
def test_uniform_settings_equal_the_dense_step(bs, key, res, n, flags):
    """ticks 0-2: every stream points at ONE image; ticks 3-5: each stream at its own image (the twin steps with the per-stream stride form)"""
    W, H = res
    path = _model(key)
    twin, mg = bs.MaskGen(path, W, H, n_streams=n), bs.MaskGen(path, W, H, n_streams=n)
    batch, stream = _split(flags)
    shared, own = _images(W, H, 1)[0], _images(W, H, n, seed0=5)
    for t in range(6):
        per_stream = t >= 3
        bg = None if flags.get("bgblur") else (own if per_stream else shared)
        f = torch.from_numpy(_frames(W, H, range(n), t)).cuda()
        fr = twin.bgr_to_yuyv(f) if flags.get("yuyv_in") else f
        a, b = _out(n, W, H, flags.get("yuyv")), _out(n, W, H, flags.get("yuyv"))
        twin.step_ex(fr, bg, a, **flags)
        st = [bs.StreamSetting(bg=None if bg is None else (bg[i] if per_stream else bg), **stream) for i in range(n)]
        mg.step_mixed(fr, b, st, **batch)
        assert torch.equal(a, b), "t=%d: composites differ" % t
        assert torch.equal(twin.masks(), mg.masks()), "t=%d: persistent masks differ" % t
        assert torch.equal(twin.ofinal(), mg.ofinal()), "t=%d: temporal state differs" % t
    twin.close()
    mg.close()


# ---- 2. a heterogeneous batch = one step_streams call per settings group --------------------------------------------------------------------------------------
# per stream: (background: "own" / gallery index / None, stream flags)
KINDS = [("own", {}), (0, {}), (1, {"flip_h": True}), (2, {"flip_v": True}), ("own", {"flip_h": True, "flip_v": True}), (None, {"bgblur": 7}),
         (None, {"bgblur": 25}), (None, {"bgblur": 7, "flip_h": True}), (1, {"filter_off": True}), (None, {"filter_off": True, "flip_h": True}),
         (0, {"filter_off": True, "bgblur": 25, "flip_v": True}), (2, {})]


def _expected_filter_off(ref, fr, kind_flags, batch):
    """the contract of a filter-off stream: the frame [YUYV -> BGR], flipped as bsx_flip_bgr, packed as bsx_bgr_to_yuyv"""
    bgr = ref.yuyv_to_bgr(fr) if batch.get("yuyv_in") else fr
    fh, fv = kind_flags.get("flip_h", False), kind_flags.get("flip_v", False)
    if fh or fv:
        bgr = ref.flip_bgr(bgr.contiguous(), -1 if (fh and fv) else (1 if fh else 0))
    return ref.bgr_to_yuyv(bgr.contiguous()) if batch.get("yuyv") else bgr


class _Mixed:
    def __init__(self, bs, path, W, H, kinds):
        self.bs, self.W, self.H, self.kinds = bs, W, H, kinds
        n = len(kinds)
        self.mg, self.twin = bs.MaskGen(path, W, H, n_streams=n), bs.MaskGen(path, W, H, n_streams=n)
        self.own, self.gallery = _images(W, H, n, seed0=11), _images(W, H, 3, seed0=31)

    def bg_of(self, s):
        b = self.kinds[s][0]
        return None if b is None else (self.own[s] if b == "own" else self.gallery[b])

    def setting(self, s, **override):
        kf = dict(self.kinds[s][1], **override)
        return self.bs.StreamSetting(bg=self.bg_of(s), **kf)

    def tick(self, t, batch, perm=None, overrides=None, msg=""):
        """one mixed call (positions in the order `perm`, None = dense) against the twin's grouped calls, compared stream by stream"""
        W, H, n = self.W, self.H, len(self.kinds)
        overrides = overrides or {}
        order = list(range(n)) if perm is None else [int(i) for i in perm]
        f = torch.from_numpy(_frames(W, H, order, t)).cuda()
        fr = self.mg.bgr_to_yuyv(f) if batch.get("yuyv_in") else f
        out = _out(n, W, H, batch.get("yuyv"))
        sett = [self.setting(s, **overrides.get(s, {})) for s in order]
        self.mg.step_mixed(fr, out, sett, ids=None if perm is None else order, **batch)
        # the twin: one step_streams call per group of equal stream flags (per-position backgrounds through the stride form)
        groups = {}
        for i, s in enumerate(order):
            kf = dict(self.kinds[s][1], **overrides.get(s, {}))
            groups.setdefault(tuple(sorted(kf.items())), []).append(i)
        want = {}
        for key, pos in groups.items():
            kf = dict(key)
            off = kf.pop("filter_off", False)
            if off:
                kf.pop("bgblur", None)
            ids = [order[i] for i in pos]
            pi = torch.tensor(pos, device="cuda")
            bg = None if kf.get("bgblur") else torch.stack([self.bg_of(s) if self.bg_of(s) is not None else self.gallery[0] for s in ids])
            o = _out(len(pos), W, H, batch.get("yuyv"))
            self.twin.step_streams(ids, fr[pi].contiguous(), bg, o, **batch, **kf)
            for j, i in enumerate(pos):
                want[i] = _expected_filter_off(self.twin, fr[i:i + 1].contiguous(), kf, batch)[0] if off else o[j]
        for i, s in enumerate(order):
            assert torch.equal(out[i], want[i]), "%s t=%d position %d (stream %d, %s): composite" % (msg, t, i, s, self.setting(s, **overrides.get(s, {})))
        assert torch.equal(self.mg.masks(), self.twin.masks()), "%s t=%d: persistent masks differ" % (msg, t)
        assert torch.equal(self.mg.ofinal(), self.twin.ofinal()), "%s t=%d: temporal state differs" % (msg, t)

    def close(self):
        self.mg.close()
        self.twin.close()


BATCH_SETS = [{}, {"yuyv": True}, {"yuyv_in": True, "yuyv": True}, {"no_mask": True}]


def _heterogeneous(bs, key, res, batch, permuted, T=3, msg=""):
    W, H = res
    m = _Mixed(bs, model_path(key), W, H, KINDS)
    rng = np.random.default_rng(5)
    for t in range(T):
        m.tick(t, batch, perm=rng.permutation(len(KINDS)) if permuted else None, msg=msg)
    m.close()


@pytest.mark.parametrize("permuted", [False, True], ids=["dense", "ids"])
@pytest.mark.parametrize("batch", BATCH_SETS, ids=["plain", "yuyv", "yuyv_in", "no_mask"])
@pytest.mark.parametrize("key,res", [("lite", VGA), ("mlkit", HD)])
def test_a_heterogeneous_batch_equals_grouped_calls(bs, key, res, batch, permuted):
    _heterogeneous(bs, key, res, batch, permuted)


# ---- 3. the filter switched off and on again ----------------------------------------------------------------------------------------------------------------
def test_filter_off_then_on_tracks_a_twin_that_never_switched(bs):
    """stream 3 (flip_v, gallery background) switches its filter off at tick 2 and on at tick 4 ('s' key): its state and mask follow the twin, which never switched;
    while off its composite is the flipped frame"""
    W, H = VGA
    m = _Mixed(bs, model_path("lite"), W, H, KINDS)
    for t in range(6):
        ov = {3: {"filter_off": True}} if 2 <= t < 4 else {}
        m.tick(t, {}, overrides=ov, msg="toggle")
    m.close()


# ---- 4. the other kernel paths --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [{}, {"yuyv_in": True, "yuyv": True}], ids=["plain", "yuyv_in"])
def test_the_generic_mask_kernel_path(bs, monkeypatch, debug_switches, batch):
    """BSX_NO_MASK_TILE=1 (debug library): every mask tile through mask_upscale_blur_k's mixed form"""
    monkeypatch.setenv("BSX_NO_MASK_TILE", "1")
    _heterogeneous(bs, "lite", VGA, batch, True, msg="no mask tile")
    _heterogeneous(bs, "mlkit", HD, batch, False, msg="no mask tile")


@pytest.mark.parametrize("batch", [{}, {"yuyv": True}], ids=["plain", "yuyv"])
def test_without_the_uniform_tile_shortcut(bs, monkeypatch, batch):
    """BSX_NO_UNIFORM_TILES=1: every tile on the general path"""
    monkeypatch.setenv("BSX_NO_UNIFORM_TILES", "1")
    _heterogeneous(bs, "lite", VGA, batch, True, msg="no uniform tiles")
    _heterogeneous(bs, "mlkit", HD, batch, False, msg="no uniform tiles")


# ---- 5. against the CPU oracle --------------------------------------------------------------------------------------------------------------------------------
def test_one_stream_per_mode_matches_the_oracle(bs, oracle):
    """lite VGA, one stream per mode — gallery background, own blur, both flips, filter off + flip, flip_v — against the CPU oracle's stateful sequence of that
    stream's frames, with the bars of tests/test_gpu_streams.py::test_two_streams_over_their_own_sub_sequences_match_the_oracle; the same batch with YUYV out is
    the oracle's bgr_to_yuyv of each composite"""
    W, H = VGA
    path = model_path("lite")
    modes = [{"bg": 0}, {"bgblur": 7}, {"bg": 1, "flip_h": True, "flip_v": True}, {"bg": 0, "filter_off": True, "flip_h": True}, {"bg": 1, "flip_v": True}]
    n = len(modes)
    mg, packed = bs.MaskGen(path, W, H, n_streams=n), bs.MaskGen(path, W, H, n_streams=n)     # packed: the same batch with YUYV out
    oc = [oracle.Ctx(path, W, H) for _ in range(n)]
    gallery = _images(W, H, 2, seed0=41)
    g_np = gallery.cpu().numpy()
    for t in range(4):
        frames = _frames(W, H, range(n), t)
        sett = [bs.StreamSetting(bg=gallery[m["bg"]] if "bg" in m else None, **{k: v for k, v in m.items() if k != "bg"}) for m in modes]
        out = _out(n, W, H, False)
        out2 = _out(n, W, H, True)
        mg.step_mixed(torch.from_numpy(frames).cuda(), out, sett)
        packed.step_mixed(torch.from_numpy(frames).cuda(), out2, sett, yuyv=True)
        got_m, got_o = mg.masks().cpu().numpy(), out.cpu().numpy()
        got_y = out2.cpu().numpy()
        for s, m in enumerate(modes):
            want_m = oc[s].process(frames[s])
            if m.get("filter_off"):
                want_o = frames[s]
            else:
                bg = oracle.gaussian_blur(frames[s], m["bgblur"]) if m.get("bgblur") else g_np[m["bg"]]
                want_o = oracle.alpha_blend(bg, frames[s], want_m)
            fh, fv = m.get("flip_h", False), m.get("flip_v", False)
            if fh or fv:
                want_o = oracle.flip_bgr(want_o, -1 if (fh and fv) else (1 if fh else 0))
            assert np.array_equal(got_y[s], oracle.bgr_to_yuyv(got_o[s])), "tick %d stream %d: YUYV out is not the pack of the composite" % (t, s)
            fa, fb = got_m[s] < 128, want_m < 128
            union = np.logical_or(fa, fb).sum()
            iou = 1.0 if union == 0 else np.logical_and(fa, fb).sum() / union
            assert iou >= 0.999, "tick %d stream %d: IoU %.5f" % (t, s, iou)
            if m.get("filter_off"):
                assert np.array_equal(got_o[s], want_o), "tick %d stream %d: filter-off composite is not the flipped frame" % (t, s)
                continue
            same = got_m[s] == want_m
            if fh or fv:
                same = oracle.flip_bgr(np.repeat(same[..., None].astype(np.uint8), 3, -1), -1 if (fh and fv) else (1 if fh else 0))[..., 0].astype(bool)
            diff = np.abs(got_o[s].astype(np.int16) - want_o.astype(np.int16)).max(-1)
            assert int(diff[same].max(initial=0)) == 0, "tick %d stream %d: composite differs where the masks agree" % (t, s)
            assert int(diff.max()) <= 1
    for c in oc:
        c.close()
    mg.close()
    packed.close()
