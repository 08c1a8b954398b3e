"""bsx_step_batch_vcam_geoms on the GPU: cameras of different capture sizes stepped together, every composite written at ONE common size.  The yardstick is the
sequence the call replaces, on a second multi-geometry context (the twin): step_geoms into capture-size BGR composites, then resize_bgr [+ bgr_to_yuyv] of each.
Per tick the outputs of the stepped streams and the persistent mask and temporal state (`ofinal`) of ALL streams are compared — byte equality throughout.  One case
checks the call against the CPU oracle with the bars of tests/test_gpu_vcam_mixed.py::test_one_stream_per_mode_matches_the_oracle."""
import functools

import numpy as np
import pytest

from conftest import model_path

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

VGA, HD, FHD, NHD = (640, 480), (1280, 720), (1920, 1080), (640, 360)
LITE = [VGA, HD, NHD]
# settings a stream cycles through: (background: "own" / "shared" / None, StreamSetting flags)
CYCLE = [("own", {}), ("shared", {}), ("own", {"flip_h": True}), ("shared", {"flip_v": True}), ("own", {"flip_h": True, "flip_v": True}), (None, {"filter_off": True})]


@pytest.fixture(scope="module")
def bs():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    import backscrub_amd
    backscrub_amd.lib()
    return backscrub_amd


def _model(key):
    return model_path("deeplab", prefer_real=False) if key == "deeplab_synthetic" else model_path(key)


@functools.lru_cache(maxsize=None)
def _frame(W, H, s, t):
    """stream s at tick t: the photo fixture on streams 0-1 at VGA, else the moving synthetic scene"""
    from backscrub_amd import synth
    if (W, H) == VGA and s < 2:
        from tools import make_photo_fixture
        return torch.from_numpy(np.ascontiguousarray(make_photo_fixture.load_frames()[s])).cuda()
    return torch.from_numpy(synth.frame(W, H, s, t)).cuda()


@functools.lru_cache(maxsize=None)
def _image(W, H, seed):
    from backscrub_amd import synth
    return torch.from_numpy(synth.background(W, H, seed=seed)).cuda()


def _out(W, H, ch):
    return torch.full((H, W, ch), 0x5a, dtype=torch.uint8, device="cuda")


class Fleet:
    """two multi-geometry contexts of the same classes: `mg` takes the new call, `twin` the sequence it replaces"""

    def __init__(self, bs, key, sizes, per_class=2):
        self.bs, self.path = bs, _model(key)
        self.geoms = [(W, H, per_class) for W, H in sizes]
        self.n = per_class * len(sizes)
        self.mg = bs.MaskGen.with_geometries(self.path, self.geoms)
        self.twin = bs.MaskGen.with_geometries(self.path, self.geoms)
        self.first = [g["first_stream"] for g in self.mg.geometries()]
        self.t = 0

    def size(self, s):
        g = max(i for i, f in enumerate(self.first) if f <= s)
        return self.geoms[g][0], self.geoms[g][1], g

    def setting(self, s, t):
        W, H, g = self.size(s)
        bg, fl = CYCLE[(s + t) % len(CYCLE)]
        img = None if bg is None else _image(W, H, 100 + s if bg == "own" else 7 + g)
        return self.bs.StreamSetting(bg=img, **fl)

    def want(self, comp, ow, oh, yuyv):
        """the capture-size BGR composite through the separate calls"""
        r = self.twin.resize_bgr(comp[None], ow, oh)
        return (self.twin.bgr_to_yuyv(r) if yuyv else r)[0]

    def tick(self, ids, ow, oh, yuyv=False, fresh=None, tag=""):
        """one call for the streams `ids` against the twin (streams in `fresh`: against that context instead), then EVERY stream's mask and ofinal.  Returns the
        outputs by stream."""
        t, fresh_ids = self.t, (fresh[1] if fresh else [])
        self.t += 1
        frames = [_frame(*self.size(s)[:2], s, t) for s in ids]
        sett = [self.setting(s, t) for s in ids]
        outs = [_out(ow, oh, 2 if yuyv else 3) for _ in ids]
        self.mg.step_vcam_geoms(ids, frames, outs, sett, yuyv=yuyv)
        comps = [_out(*self.size(s)[:2], 3) for s in ids]
        for ctx, mine in ((self.twin, [i for i, s in enumerate(ids) if s not in fresh_ids]), (fresh[0] if fresh else None, [i for i, s in enumerate(ids) if s in fresh_ids])):
            if mine:
                ctx.step_geoms([ids[i] for i in mine], [frames[i] for i in mine], [comps[i] for i in mine], [sett[i] for i in mine])
        for i, s in enumerate(ids):
            W, H, _g = self.size(s)
            assert torch.equal(outs[i], self.want(comps[i], ow, oh, yuyv)), "%st=%d stream %d (%dx%d -> %dx%d%s, %s): outputs differ" % (
                tag, t, s, W, H, ow, oh, " yuyv" if yuyv else "", CYCLE[(s + t) % len(CYCLE)])
        self.compare_state(t, fresh, tag)
        return dict(zip(ids, outs))

    def compare_state(self, t, fresh=None, tag=""):
        of, of_twin, of_fresh = self.mg.ofinal(), self.twin.ofinal(), (fresh[0].ofinal() if fresh else None)
        for s in range(self.n):
            tw, o = (fresh[0], of_fresh) if fresh and s in fresh[1] else (self.twin, of_twin)
            assert torch.equal(of[s], o[s]), "%st=%d stream %d: temporal state differs" % (tag, t, s)
            assert torch.equal(self.mg.masks_of(s), tw.masks_of(s)), "%st=%d stream %d: persistent masks differ" % (tag, t, s)

    def run(self, ow, oh, yuyv, ticks=4, seed=0, tag=""):
        """`ticks` calls: a seeded order that interleaves the classes, everyone first, then a different subset each tick"""
        rng = np.random.default_rng(9000 + seed)
        record = []
        for k in range(ticks):
            ids = [int(i) for i in rng.permutation(self.n)]
            if k:
                ids = ids[:int(rng.integers(self.n // 2, self.n))]
            record.append({s: o.cpu() for s, o in self.tick(ids, ow, oh, yuyv, tag=tag).items()})
        return record

    def close(self):
        for c in (self.mg, self.twin):
            c.close()


# ---- 1. the heterogeneous lite fleet against the separate calls ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lite(bs):
    f = Fleet(bs, "lite", LITE)
    yield f
    f.close()


# 426: width % 4 = 2; 427: odd width, byte-wise stores; 640x360: identity for one class, exact 2x of another, aspect change for the third; 1280x720: up-scale and
# identity; 160x90: 8x down
@pytest.mark.parametrize("ow,oh,yuyv", [(426, 240, False), (426, 240, True), (427, 240, False), (640, 360, False), (640, 360, True), (1280, 720, False),
                                        (1280, 720, True), (160, 90, False), (160, 90, True)])
def test_three_classes_equal_the_separate_calls(lite, ow, oh, yuyv):
    lite.run(ow, oh, yuyv, seed=ow + oh + int(yuyv))


# ---- 2. other networks --------------------------------------------------------------------------------------------------------------------------------------------
# (the per-launch DeepLab network picks its kernels by the batch's size: its twin is stepped with the same positions in the same call — the same-batch rule of
#  tests/test_gpu_geoms.py holds by construction here, the twin being a context of the same classes)
@pytest.mark.parametrize("key,sizes,ow,oh,yuyv", [("mlkit", [VGA, FHD], 854, 480, False), ("full", [VGA, HD], 640, 360, True),
                                                  ("deeplab_synthetic", [VGA, HD], 320, 240, False)])
def test_other_fleets(bs, key, sizes, ow, oh, yuyv):
    f = Fleet(bs, key, sizes)
    try:
        f.run(ow, oh, yuyv, seed=3)
    finally:
        f.close()


# ---- 3. the per-tap form forced ------------------------------------------------------------------------------------------------------------------------------------
def test_forced_per_tap_form_gives_the_same_bytes(debug_switches, monkeypatch):
    """BSX_VCAM_DIRECT (debug library) forces the per-tap form on every class; VGA -> 426x240 is a staged table otherwise (tests/test_gpu_vcam_mixed.py relies on
    that): the lite fleet gives the same bytes either way, and both equal the separate calls"""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    res = []
    for env in (None, "1"):
        if env:
            monkeypatch.setenv("BSX_VCAM_DIRECT", env)
        f = Fleet(debug_switches, "lite", LITE)
        try:
            res.append(f.run(426, 240, False, ticks=3, seed=1, tag="direct=%s " % env) + f.run(426, 240, True, ticks=2, seed=2, tag="direct=%s yuyv " % env))
            torch.cuda.synchronize()
        finally:
            f.close()
    assert len(res[0]) == len(res[1]) == 5
    for t, (a, b) in enumerate(zip(*res)):
        assert a.keys() == b.keys()
        for s in a:
            assert torch.equal(a[s], b[s]), "call %d stream %d: the per-tap form differs from the staged one" % (t, s)


# ---- 4. a context made by bsx_new ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ow,oh,yuyv", [(426, 240, False), (854, 480, True)])
def test_on_a_one_geometry_context_it_is_the_mixed_vcam_step(bs, ow, oh, yuyv):
    W, H = VGA
    n = 4
    path = _model("lite")
    mg, twin = bs.MaskGen(path, W, H, n_streams=n), bs.MaskGen(path, W, H, n_streams=n)
    try:
        for t, ids in enumerate([[2, 0, 3, 1], [3, 1], [0, 2, 1], [1, 3, 0, 2]]):
            frames = [_frame(W, H, s, t) for s in ids]
            sett = []
            for s in ids:
                bg, fl = CYCLE[(s + t) % len(CYCLE)]
                sett.append(bs.StreamSetting(bg=None if bg is None else _image(W, H, 100 + s if bg == "own" else 7), **fl))
            outs = [_out(ow, oh, 2 if yuyv else 3) for _ in ids]
            mg.step_vcam_geoms(ids, frames, outs, sett, yuyv=yuyv)
            want = torch.stack([_out(ow, oh, 2 if yuyv else 3) for _ in ids])
            twin.step_vcam_mixed(torch.stack(frames), want, sett, ids=ids, yuyv=yuyv)
            for i, s in enumerate(ids):
                assert torch.equal(outs[i], want[i]), "t=%d stream %d: outputs differ" % (t, s)
            assert torch.equal(mg.masks(), twin.masks()) and torch.equal(mg.ofinal(), twin.ofinal()), "t=%d: state differs" % t
    finally:
        mg.close()
        twin.close()


# ---- 5. a stream reset between ticks -------------------------------------------------------------------------------------------------------------------------------
def test_a_reset_stream_follows_a_fresh_twin(bs):
    f = Fleet(bs, "lite", LITE)
    fresh_ctx = None
    try:
        everyone = list(range(f.n))
        for _ in range(2):
            f.tick(everyone[::-1], 426, 240)
        victims = [1, 2, 5]                                                 # one stream per class
        f.mg.reset_streams([5, 1, 2])
        fresh_ctx = bs.MaskGen.with_geometries(f.path, f.geoms)              # a context nobody has stepped: the victims' state from now on
        fresh = (fresh_ctx, victims)
        f.compare_state(f.t, fresh)
        f.tick([3, 5, 0, 1, 4, 2], 426, 240, fresh=fresh)
        f.tick([2, 4, 1], 640, 360, yuyv=True, fresh=fresh)
        f.tick(everyone, 426, 240, fresh=fresh)
    finally:
        f.close()
        if fresh_ctx:
            fresh_ctx.close()


# ---- 6. the CPU oracle ---------------------------------------------------------------------------------------------------------------------------------------------
def _flip_code(fh, fv):
    return -1 if (fh and fv) else (1 if fh else 0)


def test_one_stream_per_class_matches_the_oracle(bs, oracle):
    """lite, one stream per class, against the CPU oracle's stateful sequence of that stream's frames: the oracle's composite, flipped, resized by the oracle's own
    resize_linear.  The bars are those of tests/test_gpu_vcam_mixed.py::test_one_stream_per_mode_matches_the_oracle, taken from there: mask IoU >= 0.999; a
    filter-off stream exact; the output exact where the masks agree and within 1 everywhere.  "Where the masks agree" for an output pixel: every source pixel of
    its taps agrees — the oracle's resize of the (flipped) disagreement map, widened by one pixel to every side, is 0 there.  Figures are printed before they are
    asserted."""
    from backscrub_amd import synth
    ow, oh = 426, 240
    path = _model("lite")
    modes = [{"bg": 0}, {"bg": 1, "flip_h": True, "flip_v": True}, {"filter_off": True, "flip_h": True}]
    mg = bs.MaskGen.with_geometries(path, [(W, H, 2) for W, H in LITE])
    ids = [1, 3, 5]                                                          # one stream per class
    size = {s: LITE[s // 2] for s in ids}
    oc = {s: oracle.Ctx(path, *size[s]) for s in ids}
    bgs = {s: [synth.background(*size[s], seed=41 + k) for k in range(2)] for s in ids}
    failures = []
    try:
        for t in range(4):
            order = ids[::-1] if t % 2 else ids
            host = {s: synth.frame(*size[s], s, t) for s in ids}
            sett = []
            for s in order:
                m = modes[ids.index(s)]
                sett.append(bs.StreamSetting(bg=torch.from_numpy(bgs[s][m["bg"]]).cuda() if "bg" in m else None, **{k: v for k, v in m.items() if k != "bg"}))
            outs = [_out(ow, oh, 3) for _ in order]
            mg.step_vcam_geoms(order, [torch.from_numpy(host[s]).cuda() for s in order], outs, sett)
            torch.cuda.synchronize()
            for i, s in enumerate(order):
                m = modes[ids.index(s)]
                W, H = size[s]
                want_m = oc[s].process(host[s])
                got_m, got_o = mg.masks_of(s).cpu().numpy(), outs[i].cpu().numpy()
                C = host[s] if m.get("filter_off") else oracle.alpha_blend(bgs[s][m["bg"]], host[s], want_m)
                fh, fv = m.get("flip_h", False), m.get("flip_v", False)
                flip = (lambda a, fh=fh, fv=fv: oracle.flip_bgr(np.ascontiguousarray(a), _flip_code(fh, fv))) if (fh or fv) else (lambda a: a)
                want_o = oracle.resize_linear(np.ascontiguousarray(flip(C)), ow, oh)
                fa, fb = got_m < 128, want_m < 128
                union = np.logical_or(fa, fb).sum()
                iou = 1.0 if union == 0 else np.logical_and(fa, fb).sum() / union
                diff = np.abs(got_o.astype(np.int16) - want_o.astype(np.int16)).max(-1)
                if m.get("filter_off"):
                    agree_max = int(diff.max())
                else:
                    dis = got_m != want_m
                    wide = dis.copy()                                # one pixel to every side
                    for dy in (-1, 0, 1):
                        for dx in (-1, 0, 1):
                            wide[max(dy, 0):H + min(dy, 0), max(dx, 0):W + min(dx, 0)] |= dis[max(-dy, 0):H + min(-dy, 0), max(-dx, 0):W + min(-dx, 0)]
                    dmap = np.repeat((wide.astype(np.uint8) * 255)[..., None], 3, -1)
                    same = oracle.resize_linear(np.ascontiguousarray(flip(dmap)), ow, oh)[..., 0] == 0
                    agree_max = int(diff[same].max(initial=0))
                print("tick %d stream %d %dx%d %s: IoU %.5f, max diff where the masks agree %d, max diff %d" % (t, s, W, H, m, iou, agree_max, int(diff.max())))
                if iou < 0.999:
                    failures.append("tick %d stream %d: IoU %.5f" % (t, s, iou))
                if agree_max != 0:
                    failures.append("tick %d stream %d: output differs by %d where the masks agree%s" % (t, s, agree_max, " (filter off)" if m.get("filter_off") else ""))
                if int(diff.max()) > 1:
                    failures.append("tick %d stream %d: max diff %d" % (t, s, int(diff.max())))
    finally:
        for c in oc.values():
            c.close()
        mg.close()
    assert not failures, "\n".join(failures)


# ---- 7. refused calls change nothing ------------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_every_stream_unchanged(bs):
    from backscrub_amd import api
    f = Fleet(bs, "lite", LITE)
    try:
        for _ in range(2):
            f.tick([5, 0, 3, 1, 4, 2], 426, 240)
        total = sum(W * H * n for W, H, n in f.geoms)
        masks, of = f.mg._view(3, "uint8", (total,)).clone(), f.mg.ofinal().clone()
        S = bs.StreamSetting

        def call(ids, ow=426, oh=240, yuyv=False, **change):
            fr = [_frame(*f.size(s)[:2], s, 9) for s in ids]
            outs = [_out(ow, oh, 2 if yuyv else 3) for _ in ids]
            st = [S(bg=_image(*f.size(s)[:2], 50)) for s in ids]
            if "same_out" in change:
                outs[2] = outs[0]
            if "out_in_frame" in change:                                     # an output-sized window of another position's frame
                outs[1] = fr[0].view(-1)[:oh * ow * 3].view(oh, ow, 3)
            if "out_in_bg" in change:
                outs[0] = st[1].bg.view(-1)[:oh * ow * 3].view(oh, ow, 3)
            return f.mg.step_vcam_geoms(ids, fr, outs, st, yuyv=yuyv)
        with pytest.raises(api.BsxError, match="repeats"):
            call([0, 3, 0])
        with pytest.raises(api.BsxError, match="out of range"):
            call([0, 6])
        with pytest.raises(api.BsxError, match="overlaps the output"):
            call([4, 2, 0], same_out=True)
        with pytest.raises(api.BsxError, match="overlaps a frame or background"):
            call([4, 2, 0], out_in_frame=True)
        with pytest.raises(api.BsxError, match="overlaps a frame or background"):
            call([0, 2, 1], out_in_bg=True)
        with pytest.raises(api.BsxError, match="even width"):
            call([0, 2], ow=427, yuyv=True)
        # the flag refusals, straight at the C entry point
        import ctypes
        ids = (ctypes.c_int * 2)(0, 2)
        items = (api._GeomItem * 2)()
        fr, outs, bg = [_frame(*f.size(s)[:2], s, 9) for s in (0, 2)], [_out(426, 240, 3) for _ in range(2)], [_image(*f.size(s)[:2], 50) for s in (0, 2)]
        for i in range(2):
            items[i].d_frame, items[i].d_out, items[i].setting.d_bg = fr[i].data_ptr(), outs[i].data_ptr(), bg[i].data_ptr()
        for flags, words in ((8, "no vcam form"), (16, "YUYV input"), (2, "outside yuyv")):
            assert api.lib().bsx_step_batch_vcam_geoms(f.mg.h, ids, items, 2, 426, 240, None, flags) == -1
            assert words in api.lib().bsx_last_error(f.mg.h).decode()
        assert api.lib().bsx_step_batch_vcam_geoms(f.mg.h, ids, items, 2, 0, 240, None, 0) == -1
        for name, fn in (("step_vcam", lambda: f.mg.step_vcam(_frame(640, 480, 0, 0)[None], _image(640, 480, 50), torch.stack([_out(426, 240, 3)]))),):
            with pytest.raises(api.BsxError, match="context has 3 geometries"):
                fn()
        torch.cuda.synchronize()
        assert torch.equal(f.mg._view(3, "uint8", (total,)), masks) and torch.equal(f.mg.ofinal(), of)
        f.compare_state(f.t)
        f.tick([2, 4, 0], 426, 240)                                          # and the context goes on as if nothing had been asked
    finally:
        f.close()
