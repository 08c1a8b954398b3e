"""bsx_resize_bgr_batch / bsx_background_grab_batch on the GPU.  Every comparison is byte equality (torch.equal / np.array_equal): n images resized in one launch
against n bsx_resize_bgr calls and against the CPU oracle's resize_linear — all three table modes, the dword and the byte store form in one launch; the pictures
an explicit time names; and the purpose of the change, end to end: grab_backgrounds + step_mixed per tick against one bsx_resize_bgr per stream + the same
step_mixed.  One leg of the end-to-end test compares with the CPU oracle's stateful sequence and takes the bars of
tests/test_gpu_mixed.py::test_one_stream_per_mode_matches_the_oracle unchanged (the network's logits are f32-close to the oracle's, not equal)."""
import math

import numpy as np
import pytest

from conftest import model_path

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

VGA = (640, 480)
# (sw, sh) -> VGA: up-scaling, down-scaling, the exact 2x area mean, the identity copy
SIZES = [(2, 2), (120, 90), (517, 333), (1280, 720), (1920, 1080), (1280, 960), (640, 480)]
GUARD = 0x5a


@pytest.fixture(scope="module")
def bs():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    import backscrub_amd
    backscrub_amd.lib()
    return backscrub_amd


def _picture(rng, w, h):
    """noise over a gradient: every tap and every coefficient matters"""
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x * 255 // max(w - 1, 1)), (y * 255 // max(h - 1, 1)), ((x + y) * 255 // max(w + h - 2, 1))], -1).astype(np.int32)
    return np.clip(base + rng.integers(-60, 61, (h, w, 3)), 0, 255).astype(np.uint8)


# ---- 5. one launch = n single resizes = the oracle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dw,dh,pad", [(640, 480, 0), (426, 240, 0), (640, 480, 2)], ids=["vga_dwords", "w426_bytes", "vga_odd_entries_unaligned"])
def test_a_batch_of_mixed_sizes_equals_single_resizes_and_the_oracle(bs, oracle, dw, dh, pad):
    """pad = 2: destination i lies at i * (image + 2) bytes, so the odd entries are not 4-byte aligned and take the byte stores, the even ones the dword stores —
    in ONE launch; the bytes between the destinations stay untouched"""
    mg = bs.MaskGen(model_path("lite"), *VGA, n_streams=8)
    rng = np.random.default_rng(17)
    src_np = [_picture(rng, w, h) for w, h in SIZES]
    srcs = [torch.from_numpy(a).cuda() for a in src_np]
    n, img = len(srcs), dw * dh * 3
    flat = torch.full((n * (img + pad),), GUARD, dtype=torch.uint8, device="cuda")
    out = flat.as_strided((n, dh, dw, 3), (img + pad, dw * 3, 3, 1))
    assert out.data_ptr() % 4 == 0
    got = mg.resize_bgr_batch(srcs, dw, dh, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    for i, (w, h) in enumerate(SIZES):
        single = mg.resize_bgr(srcs[i][None], dw, dh)[0]
        assert torch.equal(out[i], single), "entry %d (%dx%d -> %dx%d): the batch differs from bsx_resize_bgr" % (i, w, h, dw, dh)
        assert np.array_equal(out[i].cpu().numpy(), oracle.resize_linear(src_np[i], dw, dh)), "entry %d (%dx%d -> %dx%d): differs from the oracle" % (i, w, h, dw, dh)
    if pad:
        assert {int(out[i].data_ptr() % 4) for i in range(n)} == {0, 2}
        gaps = flat.view(n, img + pad)[:, img:]
        assert bool((gaps == GUARD).all()), "bytes between the destinations were written"
    # without `out`: a new contiguous tensor, the same bytes
    assert torch.equal(mg.resize_bgr_batch(srcs, dw, dh), out)
    mg.close()


# ---- 6. the pictures a time names -------------------------------------------------------------------------------------------------------------------------------
# (w, h, pictures, fps): stills and animations of different sizes, lengths and rates
SOURCES = [(640, 480, 1, 0.0), (120, 90, 5, 10.0), (1280, 720, 1, 0.0), (517, 333, 3, 24.0), (1280, 960, 2, 12.5), (320, 200, 1, 0.0)]


def _sources(bs, mg, rng):
    pics = [np.stack([_picture(rng, w, h) for _ in range(k)]) for w, h, k, _ in SOURCES]
    bgs = [bs.Background(mg, frames=p, fps=f) for p, (_, _, _, f) in zip(pics, SOURCES)]
    for b, (w, h, k, f) in zip(bgs, SOURCES):
        assert (b.width, b.height, b.n_frames, b.video) == (w, h, k, k >= 2 and f > 0)
    return pics, bgs


def _frame_no(at, pictures, fps):
    """what the header says: picture floor(at * fps) mod n of an animation, reported as 1..n; a still is always 1"""
    return (int(math.floor(at * fps)) % pictures + 1) if (pictures >= 2 and fps > 0) else 1


def test_grab_backgrounds_at_an_explicit_time(bs, oracle):
    W, H = VGA
    mg = bs.MaskGen(model_path("lite"), W, H, n_streams=8)
    pics, bgs = _sources(bs, mg, np.random.default_rng(23))
    order = [1, 0, 3, 4, 2, 1, 5, 3]                       # sources 1 and 3 appear twice
    resized = {}
    for at in (0.0, 0.26, 1.03, 7.77, 123.456):            # below, around and far beyond one loop of every animation; none near a picture boundary
        nos, out = bs.grab_backgrounds([bgs[j] for j in order], W, H, at=at)
        torch.cuda.synchronize()
        assert nos == [_frame_no(at, SOURCES[j][2], SOURCES[j][3]) for j in order], (at, nos)
        got = out.cpu().numpy()
        for i, j in enumerate(order):
            key = (j, nos[i])
            if key not in resized:
                resized[key] = oracle.resize_linear(pics[j][nos[i] - 1], W, H)
            assert np.array_equal(got[i], resized[key]), "at=%g entry %d: not the resize of picture %d of source %d" % (at, i, nos[i], j)
    assert len({k for k in resized if k[0] == 1}) >= 3, "the times must reach several pictures of the 5-picture animation"
    # the clock: every entry is the resize of the picture its own frame number names, and entries naming one source agree
    buf = torch.full((len(order), H, W, 3), GUARD, dtype=torch.uint8, device="cuda")
    nos, out = bs.grab_backgrounds([bgs[j] for j in order], W, H, out=buf, at=None)
    torch.cuda.synchronize()
    assert out.data_ptr() == buf.data_ptr()
    assert nos[0] == nos[5] and nos[2] == nos[7], nos
    got = out.cpu().numpy()
    for i, j in enumerate(order):
        assert 1 <= nos[i] <= SOURCES[j][2]
        assert np.array_equal(got[i], oracle.resize_linear(pics[j][nos[i] - 1], W, H)), "clock, entry %d" % i
    for b in bgs:
        b.close()
    mg.close()


# ---- 7. end to end: a tick = grab_backgrounds + step_mixed ------------------------------------------------------------------------------------------------------
STREAMS = [0, 1, 2, 3, 4, 5, 1, 3]                        # stream -> source: stills and animations; streams 1 / 6 and 3 / 7 share a source
TICKS = (0.05, 0.15, 0.60)                                # rising: every animation changes its picture at least once


def _scene(W, H, n, t):
    from backscrub_amd import synth
    return np.stack([synth.frame(W, H, s, t) for s in range(n)])


def test_a_tick_of_grab_and_mixed_step_equals_one_resize_per_stream(bs, oracle):
    W, H = VGA
    n = len(STREAMS)
    path = model_path("lite")
    mg, twin = bs.MaskGen(path, W, H, n_streams=n), bs.MaskGen(path, W, H, n_streams=n)
    pics, bgs = _sources(bs, mg, np.random.default_rng(29))
    d_pics = [torch.from_numpy(p).cuda() for p in pics]
    oc = [oracle.Ctx(path, W, H) for _ in range(n)]
    buf = torch.zeros((n, H, W, 3), dtype=torch.uint8, device="cuda")
    seen = set()
    for t, at in enumerate(TICKS):
        frames = _scene(W, H, n, t)
        f = torch.from_numpy(frames).cuda()
        # this change's tick: ONE grab launch into one buffer, every d_bg a slice of it
        nos, _ = bs.grab_backgrounds([bgs[j] for j in STREAMS], W, H, out=buf, at=at)
        out = torch.zeros((n, H, W, 3), dtype=torch.uint8, device="cuda")
        mg.step_mixed(f, out, [bs.StreamSetting(bg=buf[i]) for i in range(n)])
        # the parent's way: one bsx_resize_bgr of the named picture per stream, then the same step
        assert nos == [_frame_no(at, SOURCES[j][2], SOURCES[j][3]) for j in STREAMS], (at, nos)
        singles = [twin.resize_bgr(d_pics[j][nos[i] - 1][None], W, H)[0] for i, j in enumerate(STREAMS)]
        want = torch.zeros((n, H, W, 3), dtype=torch.uint8, device="cuda")
        twin.step_mixed(f, want, [bs.StreamSetting(bg=singles[i]) for i in range(n)])
        torch.cuda.synchronize()
        for i in range(n):
            assert torch.equal(out[i], want[i]), "tick %d stream %d: composite differs from the per-stream resize" % (t, i)
        assert torch.equal(mg.masks(), twin.masks()), "tick %d: persistent masks differ" % t
        # the CPU oracle's stateful sequence of each stream: mask pipeline + alpha_blend over resize_linear of that picture
        got_m, got_o = mg.masks().cpu().numpy(), out.cpu().numpy()
        for i, j in enumerate(STREAMS):
            seen.add((j, nos[i]))
            want_m = oc[i].process(frames[i])
            want_o = oracle.alpha_blend(oracle.resize_linear(pics[j][nos[i] - 1], W, H), frames[i], want_m)
            fa, fb = got_m[i] < 128, want_m < 128
            union = np.logical_or(fa, fb).sum()
            iou = 1.0 if union == 0 else np.logical_and(fa, fb).sum() / union
            print("tick %d stream %d: IoU %.6f" % (t, i, iou))
            assert iou >= 0.999, "tick %d stream %d: IoU %.5f" % (t, i, iou)
            same = got_m[i] == want_m
            diff = np.abs(got_o[i].astype(np.int16) - want_o.astype(np.int16)).max(-1)
            print("tick %d stream %d: max composite difference where the masks agree %d, elsewhere %d" % (t, i, int(diff[same].max(initial=0)), int(diff.max())))
            assert int(diff[same].max(initial=0)) == 0, "tick %d stream %d: composite differs where the masks agree" % (t, i)
            assert int(diff.max()) <= 1
    for j, (_, _, k, fps) in enumerate(SOURCES):
        if k >= 2:
            assert len({s for s in seen if s[0] == j}) >= 2, "source %d never changed its picture" % j
    for c in oc:
        c.close()
    for b in bgs:
        b.close()
    mg.close()
    twin.close()


def test_a_tick_of_grab_and_vcam_mixed_step_equals_one_resize_per_stream(bs):
    """the same tick through step_vcam_mixed at a smaller output size (426x240: neither dimension a simple ratio), with flips on two streams"""
    W, H = VGA
    ow, oh = 426, 240
    n = len(STREAMS)
    path = model_path("lite")
    mg, twin = bs.MaskGen(path, W, H, n_streams=n), bs.MaskGen(path, W, H, n_streams=n)
    pics, bgs = _sources(bs, mg, np.random.default_rng(31))
    d_pics = [torch.from_numpy(p).cuda() for p in pics]
    buf = torch.zeros((n, H, W, 3), dtype=torch.uint8, device="cuda")
    extra = [{}, {"flip_h": True}, {}, {"flip_v": True}, {}, {}, {}, {}]
    for t, at in enumerate(TICKS):
        f = torch.from_numpy(_scene(W, H, n, t)).cuda()
        nos, _ = bs.grab_backgrounds([bgs[j] for j in STREAMS], W, H, out=buf, at=at)
        out = torch.full((n, oh, ow, 3), GUARD, dtype=torch.uint8, device="cuda")
        mg.step_vcam_mixed(f, out, [bs.StreamSetting(bg=buf[i], **extra[i]) for i in range(n)])
        singles = [twin.resize_bgr(d_pics[j][nos[i] - 1][None], W, H)[0] for i, j in enumerate(STREAMS)]
        want = torch.full((n, oh, ow, 3), GUARD, dtype=torch.uint8, device="cuda")
        twin.step_vcam_mixed(f, want, [bs.StreamSetting(bg=singles[i], **extra[i]) for i in range(n)])
        torch.cuda.synchronize()
        for i in range(n):
            assert torch.equal(out[i], want[i]), "tick %d stream %d: vcam composite differs from the per-stream resize" % (t, i)
        assert torch.equal(mg.masks(), twin.masks()), "tick %d: persistent masks differ" % t
    for b in bgs:
        b.close()
    mg.close()
    twin.close()
