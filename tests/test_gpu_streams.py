"""bsx_step_batch_streams / bsx_reset_streams on the GPU: a step for a chosen subset of a context's streams, addressed by stream id, is bit-identical per stream to
that stream's frames stepped alone — byte-for-byte comparisons of composites, persistent masks and temporal state (`ofinal`), on the moving synthetic scenes and
(at 640x480) the real webcam frames of the photo fixture."""
import numpy as np
import pytest

from conftest import model_path

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

VGA, HD = (640, 480), (1280, 720)


@pytest.fixture(scope="module")
def bs():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    import backscrub_amd
    backscrub_amd.lib()
    return backscrub_amd


def _frames(W, H, streams, t):
    """frame of each listed stream at tick t: moving synthetic scenes; at 640x480 streams 0 and 1 are the photo fixture's real webcam frames"""
    from backscrub_amd import synth
    out = []
    for s in streams:
        if (W, H) == VGA and s < 2:
            from tools import make_photo_fixture
            out.append(make_photo_fixture.load_frames()[s])
        else:
            out.append(synth.frame(W, H, s, t))
    return np.stack(out)


def _bgs(W, H, n):
    from backscrub_amd import synth
    return torch.from_numpy(np.stack([synth.background(W, H, seed=1 + s) for s in range(n)])).cuda()


def _model(key):
    return model_path("deeplab", prefer_real=False) if key == "deeplab_synthetic" else model_path(key)


def _ids(v):
    return [int(i) for i in v]


FLAGS = [{}, {"yuyv": True, "flip_h": True}, {"no_mask": True}, {"yuyv_in": True, "yuyv": True}, {"bgblur": 25}, {"bgblur": 25, "flip_v": True}]


def _inputs(mg, W, H, streams, t, flags):
    f = torch.from_numpy(_frames(W, H, streams, t)).cuda()
    return mg.bgr_to_yuyv(f) if flags.get("yuyv_in") else f


def _out(n, W, H, flags):
    return torch.zeros((n, H, W, 2 if flags.get("yuyv") else 3), dtype=torch.uint8, device="cuda")


# ---- 1. identity ids = the dense step ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS, ids=["plain", "yuyv_flip_h", "no_mask", "yuyv_in", "bgblur_fused", "bgblur_two_pass"])
@pytest.mark.parametrize("key,res,n", [("lite", VGA, 8), ("mlkit", HD, 4), ("deeplab_synthetic", VGA, 4), ("full", HD, 4)])
def test_identity_ids_equal_the_dense_step(bs, key, res, n, flags):
    W, H = res
    path = _model(key)
    dense, ids_mg = bs.MaskGen(path, W, H, n_streams=n), bs.MaskGen(path, W, H, n_streams=n)
    bg = None if flags.get("bgblur") else _bgs(W, H, 1)[0]
    for t in range(3):
        fr = _inputs(dense, W, H, range(n), t, flags)
        a, b = _out(n, W, H, flags), _out(n, W, H, flags)
        dense.step_ex(fr, bg, a, **flags)
        ids_mg.step_streams(list(range(n)), fr, bg, b, **flags)
        assert torch.equal(a, b), "t=%d: composites differ" % t
        assert torch.equal(dense.masks(), ids_mg.masks()), "t=%d: persistent masks differ" % t
        assert torch.equal(dense.ofinal(), ids_mg.ofinal()), "t=%d: temporal state differs" % t
    dense.close()
    ids_mg.close()


@pytest.mark.parametrize("flags", [{}, {"yuyv": True, "flip_h": True}, {"bgblur": 25}], ids=["plain", "yuyv_flip_h", "bgblur"])
def test_identity_ids_on_the_unfused_geometry(bs, flags):
    """width % 4 != 0: the fused tile kernel refuses the geometry — process (mask up-scale kernel) + stand-alone blend [+ flip / pack passes]"""
    W, H = 642, 480
    n = 4
    path = model_path("lite")
    dense, ids_mg = bs.MaskGen(path, W, H, n_streams=n), bs.MaskGen(path, W, H, n_streams=n)
    bg = None if flags.get("bgblur") else _bgs(W, H, n)
    for t in range(3):
        fr = _inputs(dense, W, H, range(n), t, flags)
        a, b = _out(n, W, H, flags), _out(n, W, H, flags)
        dense.step_ex(fr, bg, a, **flags)
        ids_mg.step_streams(list(range(n)), fr, bg, b, **flags)
        assert torch.equal(a, b) and torch.equal(dense.masks(), ids_mg.masks()) and torch.equal(dense.ofinal(), ids_mg.ofinal()), "t=%d" % t
    dense.close()
    ids_mg.close()


# ---- 2. permutations carry state ---------------------------------------------------------------------------------------------------------------------------
def _permutation_run(bs, path, W, H, n, T, seed):
    rng = np.random.default_rng(seed)
    twin, mg = bs.MaskGen(path, W, H, n_streams=n), bs.MaskGen(path, W, H, n_streams=n)
    bgs = _bgs(W, H, n)                                       # stream s composites over ITS background, wherever its frame sits in the batch
    for t in range(T):
        p = rng.permutation(n)
        fr = torch.from_numpy(_frames(W, H, range(n), t)).cuda()
        a, b = _out(n, W, H, {}), _out(n, W, H, {})
        twin.step_ex(fr, bgs, a)
        pi = torch.from_numpy(p).cuda()
        mg.step_streams(p, fr[pi].contiguous(), bgs[pi].contiguous(), b)
        assert torch.equal(b, a[pi]), "t=%d: out[i] != twin_out[p[i]]" % t
        assert torch.equal(mg.masks(), twin.masks()), "t=%d: persistent masks differ" % t
        assert torch.equal(mg.ofinal(), twin.ofinal()), "t=%d: temporal state differs" % t
    twin.close()
    mg.close()


@pytest.mark.parametrize("key,res,n", [("lite", VGA, 8), ("full", HD, 6), ("deeplab_synthetic", VGA, 4)])
def test_permutations_carry_the_state(bs, key, res, n):
    _permutation_run(bs, _model(key), res[0], res[1], n, 4, seed=7)


def test_permutations_on_the_lane_route(bs, monkeypatch, debug_switches):
    """BSX_LANES=4 (debug library): the batch splits into four contiguous groups on their own HIP streams — lane k reads ids[f0 ..]"""
    monkeypatch.setenv("BSX_LANES", "4")
    _permutation_run(bs, model_path("lite"), VGA[0], VGA[1], 64, 3, seed=11)


# ---- 3. a sparse schedule = one context per stream ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,sizes", [("lite", [1, 12, 5, 3, 9, 7]), ("deeplab", [1, 3, 2, 3, 1, 2])])
def test_sparse_schedule_equals_one_context_per_stream(bs, key, sizes):
    """N = 12 streams, 6 ticks, seeded random subsets in shuffled order.  The reference is 12 one-stream contexts, context s stepped only on the ticks that list s.
    (DeepLab's per-launch network picks its pointwise-convolution form by the batch's pixel count — the lane-per-output form up to 3 streams at 257 x 257, the GEMMs
    from 8 — and a one-stream context runs the former: its subsets stay within that form, so that "stepped alone" is the same arithmetic.)"""
    N = 12
    W, H = VGA
    path = model_path(key)
    rng = np.random.default_rng(3)
    mg = bs.MaskGen(path, W, H, n_streams=N)
    ref = [bs.MaskGen(path, W, H, n_streams=1) for _ in range(N)]
    bgs = _bgs(W, H, N)
    for t, k in enumerate(sizes):
        ids = rng.permutation(N)[:k]
        before_m, before_o = mg.masks().clone(), mg.ofinal().clone()
        fr = torch.from_numpy(_frames(W, H, ids, t)).cuda()
        pi = torch.from_numpy(ids).cuda()
        out = _out(k, W, H, {})
        mg.step_streams(ids, fr, bgs[pi].contiguous(), out)
        for i, s in enumerate(_ids(ids)):
            o = _out(1, W, H, {})
            ref[s].step_ex(fr[i:i + 1].contiguous(), bgs[s], o)
            assert torch.equal(out[i], o[0]), "tick %d position %d (stream %d): composite" % (t, i, s)
            assert torch.equal(mg.masks()[s], ref[s].masks()[0]), "tick %d stream %d: persistent mask" % (t, s)
            assert torch.equal(mg.ofinal()[s], ref[s].ofinal()[0]), "tick %d stream %d: temporal state" % (t, s)
        rest = torch.from_numpy(np.setdiff1d(np.arange(N), ids)).cuda()
        assert torch.equal(mg.masks()[rest], before_m[rest]) and torch.equal(mg.ofinal()[rest], before_o[rest]), "tick %d: a stream not listed changed" % t
    for r in ref:
        r.close()
    mg.close()


# ---- 4. against the CPU oracle -----------------------------------------------------------------------------------------------------------------------------
def test_two_streams_over_their_own_sub_sequences_match_the_oracle(bs, oracle):
    """streams 0 (the photo fixture) and 2 (a moving synthetic scene) of a 4-stream context, each stepped on its own ticks (in either order within a tick), against
    the CPU oracle's stateful sequence of that stream's frames — the bars of the end-to-end parity tests (tests/test_gpu_parity.py)"""
    from backscrub_amd import synth
    W, H = VGA
    path = model_path("lite")
    mg = bs.MaskGen(path, W, H, n_streams=4)
    oc = {0: oracle.Ctx(path, W, H), 2: oracle.Ctx(path, W, H)}
    bg = synth.background(W, H)
    d_bg = torch.from_numpy(bg).cuda()
    schedule = [[0, 2], [2], [0], [2, 0], [2], [0, 2]]
    for t, ids in enumerate(schedule):
        frames = _frames(W, H, ids, t)
        out = _out(len(ids), W, H, {})
        mg.step_streams(ids, torch.from_numpy(frames).cuda(), d_bg, out)
        got_m, got_o = mg.masks().cpu().numpy(), out.cpu().numpy()
        for i, s in enumerate(ids):
            want_m = oc[s].process(frames[i])
            want_o = oracle.alpha_blend(bg, frames[i], want_m)
            fa, fb = got_m[s] < 128, want_m < 128
            union = np.logical_or(fa, fb).sum()
            iou = 1.0 if union == 0 else np.logical_and(fa, fb).sum() / union
            assert iou >= 0.999, "tick %d stream %d: IoU %.5f" % (t, s, iou)
            same = got_m[s] == want_m
            diff = np.abs(got_o[i].astype(np.int16) - want_o.astype(np.int16)).max(-1)
            assert int(diff[same].max(initial=0)) == 0, "tick %d stream %d: composite differs where the masks agree" % (t, s)
            assert int(diff.max()) <= 1
    for c in oc.values():
        c.close()
    mg.close()


# ---- 5. reset_streams --------------------------------------------------------------------------------------------------------------------------------------
def test_reset_streams_resets_only_the_listed_streams(bs):
    W, H = VGA
    n = 6
    path = model_path("lite")
    mg = bs.MaskGen(path, W, H, n_streams=n)
    bgs = _bgs(W, H, n)
    for t in range(3):
        mg.step_ex(torch.from_numpy(_frames(W, H, range(n), t)).cuda(), bgs, _out(n, W, H, {}))
    before_m, before_o = mg.masks().clone(), mg.ofinal().clone()
    mg.reset_streams([4, 1])
    torch.cuda.synchronize()
    assert bool((mg.ofinal()[[1, 4]] == 0).all()) and bool((mg.masks()[[1, 4]] == 255).all())
    keep = [0, 2, 3, 5]
    assert torch.equal(mg.masks()[keep], before_m[keep]) and torch.equal(mg.ofinal()[keep], before_o[keep])
    assert bool((before_o[[1, 4]] != 0).any())                 # the reset really changed something
    # the next tick: a reset stream is a new camera — equal to a fresh one-stream context's first tick
    ids = [1, 3]
    fr = torch.from_numpy(_frames(W, H, ids, 5)).cuda()
    out = _out(2, W, H, {})
    mg.step_streams(ids, fr, bgs[[1, 3]].contiguous(), out)
    fresh = bs.MaskGen(path, W, H, n_streams=1)
    o = _out(1, W, H, {})
    fresh.step_ex(fr[:1].contiguous(), bgs[1], o)
    assert torch.equal(out[0], o[0]) and torch.equal(mg.masks()[1], fresh.masks()[0]) and torch.equal(mg.ofinal()[1], fresh.ofinal()[0])
    mg.reset_streams([])                                         # an empty list: a no-op
    with pytest.raises(bs.BsxError, match=r"ids\[1\] = 3 repeats ids\[0\]"):
        mg.reset_streams([3, 3])
    fresh.close()
    mg.close()
