"""bsx_new_geoms / bsx_step_batch_geoms on the GPU: cameras of different capture sizes stepped together — one prep launch, one network pass, one tile launch — are
byte-identical, per stream, to one-geometry contexts of their sizes stepped with bsx_step_batch_mixed (existing, oracle-checked code): composites, persistent masks
and temporal state (`ofinal`), every tick.  Byte equality everywhere; the oracle test asserts IoU 1.0 and a composite difference of 0."""
import functools

import numpy as np
import pytest

from conftest import model_path

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

VGA, HD, FHD = (640, 480), (1280, 720), (1920, 1080)
# classes per model: all on the fused tile route (W, roi.x, roi.w multiples of 4)
CLASSES = {
    "lite": [VGA, HD, (640, 360), (800, 600), (1280, 800)],
    "mlkit": [VGA, HD, FHD],
    "full": [VGA, HD, FHD],
    "deeplab_synthetic": [VGA, HD],
}
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


def _out(W, H, yuyv, n=None):
    shape = (H, W, 2 if yuyv else 3)
    return torch.zeros(shape if n is None else (n,) + shape, dtype=torch.uint8, device="cuda")


class Fleet:
    """one multi-geometry context and one one-geometry twin per class.

    same_batch (the per-launch DeepLab network only): that network picks the form of its pointwise convolutions by the batch's pixel count — the lane-per-output form
    up to 3 streams at 257 x 257, the MFMA GEMMs from 8 (tests/test_gpu_streams.py, test_sparse_schedule_equals_one_context_per_stream) — so a call of 10 positions
    and a call of 4 are different arithmetic whatever the capture sizes are.  Its twins therefore hold every stream of the fleet (slot = the fleet's stream id) and
    are stepped with as many positions as the geoms call: the positions of their own class with the real frames and settings, the others with a frame of the twin's
    size and the filter off; only the streams of the twin's class are compared."""

    def __init__(self, bs, key, sizes, counts, same_batch=False):
        self.bs, self.path, self.same_batch = bs, _model(key), same_batch
        self.geoms = [(W, H, n) for (W, H), n in zip(sizes, counts)]
        self.n = sum(counts)
        self.mg = bs.MaskGen.with_geometries(self.path, self.geoms)
        self.twins = [bs.MaskGen(self.path, W, H, n_streams=self.n if same_batch else n) for W, H, n in self.geoms]
        self.first = [g["first_stream"] for g in self.mg.geometries()]

    def slot(self, s):
        """stream s of the fleet in the twin of its class"""
        return s if self.same_batch else self.cls(s)[1]

    def cls(self, s):
        g = max(i for i, f in enumerate(self.first) if f <= s)
        return g, s - self.first[g]

    def setting(self, s, t):
        g, _ = self.cls(s)
        W, H, _n = self.geoms[g]
        bg, fl = CYCLE[(s + t) % len(CYCLE)]
        img = None if bg is None else _image(W, H, 100 + s if bg == "own" else 7 + g)
        return self.bs.StreamSetting(bg=img, **fl)

    def new_twin(self, s):
        """a fresh twin for stream s (after a reset of that stream): replaces its slot in a one-stream context of its own"""
        g, _ = self.cls(s)
        W, H, _n = self.geoms[g]
        return self.bs.MaskGen(self.path, W, H, n_streams=1)

    def tick(self, t, ids, yuyv=False, no_mask=False, fresh=None, check=None, tag=""):
        """one geoms call for the streams `ids` (any order) against the twins, then EVERY stream's mask and ofinal against its twin's (a stream that sits out keeps
        its state).  fresh: {stream: one-stream twin} for streams that were reset.  Returns the composites by stream."""
        fresh = fresh or {}
        frames, outs, sett = [], [], []
        for s in ids:
            g, _ = self.cls(s)
            W, H, _n = self.geoms[g]
            frames.append(_frame(W, H, s, t))
            outs.append(_out(W, H, yuyv))
            sett.append(self.setting(s, t))
        self.mg.step_geoms(ids, frames, outs, sett, yuyv=yuyv, no_mask=no_mask)
        got = dict(zip(ids, outs))
        # the twins: one mixed call per class for the streams of that class, in the caller's order
        for g, (W, H, _n) in enumerate(self.geoms):
            pos = [i for i, s in enumerate(ids) if self.cls(s)[0] == g and s not in fresh]
            if pos and self.same_batch:
                mine = set(pos)
                fr = torch.stack([frames[i] if i in mine else _frame(W, H, ids[i], t) for i in range(len(ids))])
                st = [sett[i] if i in mine else self.bs.StreamSetting(filter_off=True) for i in range(len(ids))]
                want = _out(W, H, yuyv, len(ids))
                self.twins[g].step_mixed(fr, want, st, ids=list(ids), yuyv=yuyv, no_mask=no_mask)
                for i in pos:
                    assert torch.equal(outs[i], want[i]), "%st=%d stream %d (%dx%d): composites differ" % (tag, t, ids[i], W, H)
            elif pos:
                local = [self.cls(ids[i])[1] for i in pos]
                want = _out(W, H, yuyv, len(pos))
                self.twins[g].step_mixed(torch.stack([frames[i] for i in pos]), want, [sett[i] for i in pos], ids=local, yuyv=yuyv, no_mask=no_mask)
                for k, i in enumerate(pos):
                    assert torch.equal(outs[i], want[k]), "%st=%d stream %d (%dx%d): composites differ" % (tag, t, ids[i], W, H)
        for i, s in enumerate(ids):
            if s in fresh:
                g, _ = self.cls(s)
                W, H, _n = self.geoms[g]
                want = _out(W, H, yuyv, 1)
                fresh[s].step_mixed(frames[i][None], want, [sett[i]], yuyv=yuyv, no_mask=no_mask)
                assert torch.equal(outs[i], want[0]), "%st=%d reset stream %d: composites differ" % (tag, t, s)
        if check is None or check:
            self.compare_state(t, fresh, masks=not no_mask, tag=tag)
        return got

    def compare_state(self, t, fresh=None, masks=True, tag=""):
        fresh = fresh or {}
        of = self.mg.ofinal()
        for s in range(self.n):
            g, loc = self.cls(s)
            tw, k = (fresh[s], 0) if s in fresh else (self.twins[g], self.slot(s))
            assert torch.equal(of[s], tw.ofinal()[k]), "%st=%d stream %d: temporal state differs" % (tag, t, s)
            if masks:
                assert torch.equal(self.mg.masks_of(s), tw.masks()[k]), "%st=%d stream %d: persistent masks differ" % (tag, t, s)

    def close(self):
        for c in [self.mg] + self.twins:
            c.close()


# ---- 1. one class equals the mixed step ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [{}, {"yuyv": True}, {"no_mask": True}], ids=["bgr", "yuyv", "no_mask"])
@pytest.mark.parametrize("key,res,n", [("lite", VGA, 8), ("mlkit", HD, 4), ("deeplab_synthetic", VGA, 4), ("full", HD, 4)])
def test_one_class_equals_the_mixed_step(bs, key, res, n, batch):
    f = Fleet(bs, key, [res], [n])
    assert len(f.mg.geometries()) == 1 and f.mg.info["roi"] == f.twins[0].info["roi"]
    for t in range(6):
        f.tick(t, list(range(n)), **batch)
        if batch.get("no_mask"):                      # the masks a call without the flag stored last: both still at their initial value
            assert torch.equal(f.mg.masks_of(0), f.twins[0].masks()[0])
    f.close()


# ---- 2. several classes equal their twins -------------------------------------------------------------------------------------------------------------------
def _several(bs, key, per_class, yuyv=False):
    sizes = CLASSES[key]
    counts = [per_class[i % len(per_class)] for i in range(len(sizes))]
    f = Fleet(bs, key, sizes, counts, same_batch=key == "deeplab_synthetic")
    rng = np.random.default_rng(20240 + len(sizes))
    record = []
    for t in range(8):
        ids = [int(i) for i in rng.permutation(f.n)]                       # a seeded order that interleaves the classes
        if t >= 3:                                                          # from tick 3: a different subset each tick
            ids = ids[:int(rng.integers(f.n // 2, f.n))]
        got = f.tick(t, ids, yuyv=yuyv)
        record.append({s: o.cpu() for s, o in got.items()})
    f.close()
    return record


@pytest.mark.parametrize("key,per_class", [("lite", (4, 5, 6)), ("mlkit", (4, 5, 4)), ("full", (4, 4, 5)), ("deeplab_synthetic", (6, 4))])
def test_several_classes_equal_their_twins(bs, key, per_class):
    _several(bs, key, per_class)


def test_several_classes_yuyv_out(bs):
    _several(bs, "lite", (4, 5), yuyv=True)


# ---- 3. the uniform-tile shortcut off ----------------------------------------------------------------------------------------------------------------------
def test_without_the_uniform_tile_shortcut(bs, monkeypatch):
    default = _several(bs, "lite", (4, 5, 6))
    monkeypatch.setenv("BSX_NO_UNIFORM_TILES", "1")
    general = _several(bs, "lite", (4, 5, 6))
    assert len(default) == len(general) == 8
    for t, (a, b) in enumerate(zip(default, general)):
        assert a.keys() == b.keys()
        for s in a:
            assert torch.equal(a[s], b[s]), "t=%d stream %d: the general path differs from the default run" % (t, s)


# ---- 4. resets ------------------------------------------------------------------------------------------------------------------------------------------------
def test_reset_streams_and_reset(bs):
    sizes = CLASSES["lite"][:3]
    f = Fleet(bs, "lite", sizes, [4, 4, 4])
    everyone = list(range(f.n))
    for t in range(4):
        f.tick(t, everyone[::-1])
    victims = [1, 6, 11]                                                   # one stream per class
    f.mg.reset_streams([6, 11, 1])
    fresh = {s: f.new_twin(s) for s in victims}
    f.compare_state(4, fresh)
    for t in range(4, 7):
        f.tick(t, everyone, fresh=fresh)
    f.mg.reset()
    for tw in f.twins:
        tw.reset()
    for tw in fresh.values():
        tw.close()
    f.compare_state(7)
    for t in range(7, 10):
        f.tick(t, everyone)
    f.close()


# ---- 5. the full batch: 256 streams of three sizes ------------------------------------------------------------------------------------------------------------
def test_full_batch_of_three_sizes(bs):
    from backscrub_amd import synth
    geoms = [(640, 480, 128), (1280, 720, 64), (640, 360, 64)]
    path = _model("lite")
    mg = bs.MaskGen.with_geometries(path, geoms)
    twins = [bs.MaskGen(path, W, H, n_streams=n) for W, H, n in geoms]
    first = [g["first_stream"] for g in mg.geometries()]
    assert first == [0, 128, 192] and mg.n_streams == 256
    rng = np.random.default_rng(5)
    order = [int(i) for i in rng.permutation(256)]
    gallery = [[_image(W, H, 40 + k) for k in range(3)] for W, H, _n in geoms]
    flips = [{}, {"flip_h": True}, {"flip_v": True}, {"filter_off": True}]
    sett_of = {s: (s % 3, flips[(s // 3) % 4]) for s in range(256)}
    outs = [_out(W, H, False, n) for W, H, n in geoms]
    want = [_out(W, H, False, n) for W, H, n in geoms]
    for t in range(3):
        fr = [torch.from_numpy(synth.frames(n, W, H, t=t, distinct=8)).cuda() for W, H, n in geoms]

        def where(s):
            g = max(i for i, f0 in enumerate(first) if f0 <= s)
            return g, s - first[g]
        frames, os_, st = [], [], []
        for s in order:
            g, k = where(s)
            frames.append(fr[g][k])
            os_.append(outs[g][k])
            st.append(bs.StreamSetting(bg=gallery[g][sett_of[s][0]], **sett_of[s][1]))
        mg.step_geoms(order, frames, os_, st)
        for g, (W, H, n) in enumerate(geoms):
            twins[g].step_mixed(fr[g], want[g], [bs.StreamSetting(bg=gallery[g][sett_of[first[g] + k][0]], **sett_of[first[g] + k][1]) for k in range(n)])
            assert torch.equal(outs[g], want[g]), "t=%d class %d: composites differ" % (t, g)
            assert torch.equal(mg.ofinal()[first[g]:first[g] + n], twins[g].ofinal()), "t=%d class %d: temporal state differs" % (t, g)
            off = mg.geometries()[g]["mask_offset"]
            whole = mg._view(3, "uint8", (sum(a * b * c for a, b, c in geoms),))
            assert torch.equal(whole[off:off + n * W * H].view(n, H, W), twins[g].masks()), "t=%d class %d: persistent masks differ" % (t, g)
    for c in [mg] + twins:
        c.close()


# ---- 6. the CPU oracle ----------------------------------------------------------------------------------------------------------------------------------------
def test_one_stream_per_class_against_the_oracle(bs, oracle):
    """one stream per class of the lite fleet against the CPU oracle over the same frames from a reset state.  The figures are printed before they are asserted."""
    from backscrub_amd import synth
    sizes = CLASSES["lite"]
    path = _model("lite")
    mg = bs.MaskGen.with_geometries(path, [(W, H, 2) for W, H in sizes])
    ids = [2 * g + 1 for g in range(len(sizes))][::-1]
    bgs = {s: synth.background(sizes[s // 2][0], sizes[s // 2][1], seed=3 + s) for s in ids}
    ocs = {s: oracle.Ctx(path, sizes[s // 2][0], sizes[s // 2][1]) for s in ids}
    T = 4
    figures = []
    for t in range(T):
        host = {s: synth.frame(sizes[s // 2][0], sizes[s // 2][1], s, t) for s in ids}
        frames = [torch.from_numpy(host[s]).cuda() for s in ids]
        outs = [_out(sizes[s // 2][0], sizes[s // 2][1], False) for s in ids]
        mg.step_geoms(ids, frames, outs, [bs.StreamSetting(bg=torch.from_numpy(bgs[s]).cuda()) for s in ids])
        torch.cuda.synchronize()
        for i, s in enumerate(ids):
            want = ocs[s].process(host[s])
            got = mg.masks_of(s).cpu().numpy()
            fa, fb = got < 128, want < 128
            union = np.logical_or(fa, fb).sum()
            iou = 1.0 if union == 0 else float(np.logical_and(fa, fb).sum()) / float(union)
            comp = oracle.alpha_blend(bgs[s], host[s], want)
            diff = int(np.abs(outs[i].cpu().numpy().astype(np.int16) - comp.astype(np.int16)).max())
            figures.append((t, s, sizes[s // 2], iou, diff, int((got != want).sum())))
    for fgr in figures:
        print("t=%d stream %d %s: IoU %.6f, composite max |difference| %d, mask bytes that differ %d" % fgr)
    for oc in ocs.values():
        oc.close()
    mg.close()
    for t, s, size, iou, diff, _ in figures:
        assert iou == 1.0, "t=%d stream %d %s: mask IoU %.6f" % (t, s, size, iou)
        assert diff == 0, "t=%d stream %d %s: composite differs by %d" % (t, s, size, diff)


# ---- 7. refused calls change nothing ------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_every_stream_unchanged(bs):
    sizes = CLASSES["lite"][:3]
    f = Fleet(bs, "lite", sizes, [2, 2, 2])
    for t in range(3):
        f.tick(t, [5, 0, 3, 1, 4, 2])
    total = sum(W * H * n for W, H, n in f.geoms)
    masks, of = f.mg._view(3, "uint8", (total,)).clone(), f.mg.ofinal().clone()
    S = bs.StreamSetting

    def call(ids, **change):
        fr = [_frame(*sizes[f.cls(s)[0]], s, 9) for s in ids]
        outs = [_out(*sizes[f.cls(s)[0]], False) for s in ids]
        st = [S(bg=_image(*sizes[f.cls(s)[0]], 50)) for s in ids]
        if "out_is_frame" in change:
            outs[1] = fr[1]
        if "overlap" in change:
            outs[0] = st[2].bg if f.cls(ids[0])[0] == f.cls(ids[2])[0] else outs[0]
        return f.mg.step_geoms(ids, fr, outs, st)
    from backscrub_amd import api
    with pytest.raises(api.BsxError, match="repeats"):
        call([0, 3, 0])
    with pytest.raises(api.BsxError, match="out of range"):
        call([0, 6])
    with pytest.raises(api.BsxError, match="overlaps a frame or background"):
        call([4, 2, 0], out_is_frame=True)
    with pytest.raises(api.BsxError, match="overlaps a frame or background"):
        call([0, 2, 1], overlap=True)
    for name, fn in (("step", lambda: f.mg.step(_frame(640, 480, 0, 0)[None], _image(640, 480, 50), _out(640, 480, False, 1))),
                     ("process_batch", lambda: f.mg.process_batch(_frame(640, 480, 0, 0)[None]))):
        with pytest.raises(api.BsxError, match="context has 3 geometries"):
            fn()
    torch.cuda.synchronize()
    assert torch.equal(f.mg._view(3, "uint8", (total,)), masks) and torch.equal(f.mg.ofinal(), of)
    f.compare_state(3)
    f.tick(3, [2, 4, 0])                                                    # and the context goes on as if nothing had been asked
    f.close()
