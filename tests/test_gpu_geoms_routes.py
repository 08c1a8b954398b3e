"""bsx_step_batch_geoms / bsx_step_batch_vcam_geoms on every route a class can take (docs/design/02b-geometry-audit.md, "Multi-geometry steps"): the fleets of
tests/geoms_route_cases.py — general prep, the classifier's zero-fill, the LDS fit boundary, portrait classes, 8 classes in one call, absent classes, the remainder
of the one-XCD-per-frame order inside a class segment — stepped on the GPU and compared with the CPU oracle.

The method is tests/test_gpu_geometry.py's: every comparison is byte equality and none depends on the network's float result.  After each call the temporal state
the DEVICE holds is read back; the oracle's resize and blur make the mask that state implies (geometry_cases.mask_of_state), the oracle's blend, flip, resize and
YUYV pack the output that mask implies.  Prep is compared directly: the 8-bit network input the call wrote (MaskGen.input_u8) against oracle.Ctx.prep.  Streams a
call does not name keep every byte of their state and mask.  A failure names the fleet, call, stream, class size, the number of differing bytes and the first
differing (y, x)."""
import functools

import numpy as np
import pytest

from conftest import model_path
import geometry_cases as gc
import geoms_route_cases as rc
from test_gpu_geometry import bs, _dev, _flip          # noqa: F401 (bs: the library fixture)
from test_gpu_geoms import CYCLE

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = 0xA5                                           # every output buffer holds it before the call
FLAT = (32, 96, 160)                                      # one stream per fleet shows one flat colour: its state saturates, its mask tiles turn uniform
VCAM_SIZES = [(320, 180, False), (320, 180, True), (427, 240, False)]      # down for most classes, up for the small ones; packed; an odd width


def _flat_stream(name):
    """the first stream of the fleet's 640 x 480 class (none in the xcd fleets)"""
    for c, f in zip(rc.FLEETS[name]["classes"], rc.first_streams(name)):
        if c["size"] == (640, 480):
            return f
    return None


class Data:
    """host data of one fleet, computed once, shared by every test of the fleet and never written: per stream a base frame (the last stream of every class pure
    noise, frames above 1 MP rendered at a quarter of the size and repeated) and a background of its own, per class a shared background"""

    def __init__(self, name):
        from backscrub_amd import synth
        self.name, self.first = name, rc.first_streams(name)
        self.sizes = [c["size"] for c in rc.FLEETS[name]["classes"]]
        self.cls_of, self.base, self.own, self.shared = [], [], [], []
        flat = _flat_stream(name)
        for g, c in enumerate(rc.FLEETS[name]["classes"]):
            W, H = c["size"]
            self.shared.append(synth.random_u8((H, W, 3), 7 + g))
            for k in range(c["n"]):
                s = self.first[g] + k
                if k == c["n"] - 1:
                    fr = synth.random_u8((H, W, 3), 700 + s)
                elif s == flat:
                    fr = np.empty((H, W, 3), np.uint8)
                    fr[:] = FLAT
                elif W * H > 1 << 20:
                    fr = np.ascontiguousarray(np.repeat(np.repeat(synth.frame((W + 3) // 4, (H + 3) // 4, s), 4, 0), 4, 1)[:H, :W])
                else:
                    fr = synth.frame(W, H, s)
                self.cls_of.append(g)
                self.base.append(fr)
                self.own.append(synth.random_u8((H, W, 3), 100 + s))
        self.n = len(self.base)
        self._dev = {}

    def frame(self, s, t):
        """fresh frames every call: the scene shifted, the noise with it"""
        return np.ascontiguousarray(np.roll(self.base[s], (3 * t, 5 * t), axis=(0, 1)))

    def bg(self, kind, s):
        """(host, device) background of stream s: its own or its class's"""
        key = (kind, s if kind == "own" else self.cls_of[s])
        host = self.own[key[1]] if kind == "own" else self.shared[key[1]]
        if key not in self._dev:
            self._dev[key] = _dev(host)
        return host, self._dev[key]


@functools.lru_cache(maxsize=None)
def _data(name):
    return Data(name)


def _same(got, want, what):
    if np.array_equal(got, want):
        return
    ne = got != want
    y, x = np.argwhere(ne.reshape(ne.shape[0], ne.shape[1], -1).any(-1))[0]
    pytest.fail("%s: %d bytes differ, the first at (y, x) = (%d, %d)" % (what, int(ne.sum()), y, x))


class Run:
    """one multi-geometry context of a fleet, one oracle context per class, and (twin_classes) one-geometry twins"""

    def __init__(self, bs, oracle, name, twin_classes=()):
        self.bs, self.oracle, self.name, self.data = bs, oracle, name, _data(name)
        self.path = model_path(rc.FLEETS[name]["model"])
        self.classes = rc.FLEETS[name]["classes"]
        self.mg = bs.MaskGen.with_geometries(self.path, rc.geoms(name))
        self.geo = self.mg.geometries()
        self.oc = [oracle.Ctx(self.path, W, H) for W, H in self.data.sizes]
        self.n = self.data.n
        self.total = sum(W * H * c["n"] for (W, H), c in zip(self.data.sizes, self.classes))
        self.twins = {g: bs.MaskGen(self.path, *self.data.sizes[g], n_streams=self.classes[g]["n"]) for g in twin_classes}
        self.lively = False
        self.tiles = [[0, 0] for _ in self.classes]       # per class: mask tiles constant 0 / 255, and the others (from the oracle-implied masks)

    def check_classes(self):
        """a. the library's rectangles, the oracle's and the table's"""
        assert self.mg.n_streams == self.n and len(self.geo) == len(self.classes)
        for g, (c, q, oc) in enumerate(zip(self.classes, self.geo, self.oc)):
            what = "%s class %d (%dx%d)" % ((self.name, g) + c["size"])
            assert (q["width"], q["height"], q["n_streams"], q["first_stream"]) == c["size"] + (c["n"], self.data.first[g]), what
            assert tuple(q["roi"]) == oc.roidim == c["roi"], "%s: roi %s, oracle %s, table %s" % (what, q["roi"], oc.roidim, c["roi"])
            assert tuple(q["in_roi"]) == oc.in_roidim == c["in_roi"], "%s: in_roi %s, oracle %s, table %s" % (what, q["in_roi"], oc.in_roidim, c["in_roi"])

    def whole(self):
        return self.mg._view(3, "uint8", (self.total,))

    def mask(self, whole, s):
        """stream s's persistent mask inside a host copy of the whole allocation"""
        g = self.data.cls_of[s]
        W, H = self.data.sizes[g]
        off = self.geo[g]["mask_offset"] + (s - self.data.first[g]) * W * H
        return whole[off:off + W * H].reshape(H, W)

    def call(self, t, ids, yuyv=False, no_mask=False, plain=False, yin=(), vcam=None, prep=False, judge=True):
        """call number t for the streams `ids`: step_geoms, or step_vcam_geoms at vcam = (ow, oh).  Settings: plain = every stream its own background, else the
        cycle of tests/test_gpu_geoms.py by stream and call; yin: the streams whose frame travels as YUYV 4:2:2.  judge: against the oracle (else the caller
        compares the returned bytes with another context's).  Returns ({stream: output}, ofinal, the mask allocation) as host arrays."""
        d, mg, oracle, S = self.data, self.mg, self.oracle, self.bs.StreamSetting
        tag = "%s call %d%s" % (self.name, t, " (vcam %dx%d%s)" % (vcam + (" yuyv" if yuyv else "",)) if vcam else "")
        items = []
        for s in ids:
            g = d.cls_of[s]
            fr = d.frame(s, t)
            if s in yin:
                pk = oracle.bgr_to_yuyv(fr)
                seen, dev = oracle.yuyv_to_bgr(pk), _dev(pk)
            else:
                seen, dev = fr, _dev(fr)
            kind, fl = ("own", {}) if plain else CYCLE[(s + t) % len(CYCLE)]
            bg, d_bg = (None, None) if kind is None else d.bg(kind, s)
            items.append(dict(s=s, g=g, size=d.sizes[g], seen=seen, dev=dev, bg=bg, d_bg=d_bg, fl=fl, yin=s in yin))
        ch = 2 if yuyv else 3
        outs = [torch.full((vcam[1], vcam[0], ch) if vcam else (it["size"][1], it["size"][0], ch), SENTINEL, dtype=torch.uint8, device="cuda") for it in items]
        sett = [S(bg=it["d_bg"], yuyv_in=it["yin"], **it["fl"]) for it in items]
        of0, m0 = mg.ofinal().cpu().numpy(), self.whole().cpu().numpy()
        if vcam:
            mg.step_vcam_geoms(ids, [it["dev"] for it in items], outs, sett, yuyv=yuyv)
        else:
            mg.step_geoms(ids, [it["dev"] for it in items], outs, sett, yuyv=yuyv, no_mask=no_mask)
        torch.cuda.synchronize()
        of1, m1 = mg.ofinal().cpu().numpy(), self.whole().cpu().numpy()
        # streams the call does not name keep every byte
        named = set(ids)
        for s in range(self.n):
            if s not in named:
                what = "%s stream %d (%dx%d), not in the call" % ((tag, s) + d.sizes[d.cls_of[s]])
                _same(of1[s], of0[s], what + ": state")
                _same(self.mask(m1, s), self.mask(m0, s), what + ": persistent mask")
        res = {}
        for it, out in zip(items, outs):
            s, g, (W, H) = it["s"], it["g"], it["size"]
            got = out.cpu().numpy()
            res[s] = got
            if not judge:
                continue
            what = "%s stream %d (%dx%d, %s)" % (tag, s, W, H, ", ".join(sorted(it["fl"])) or "blend")
            st = of1[s]
            self.lively = self.lively or bool(((st < 128).any() and (st >= 128).any()) or ((st != 0) & (st != 255)).any())
            want_m = gc.mask_of_state(oracle, st, self.geo[g], W, H)
            mk = self.mask(m1, s)
            if no_mask:
                _same(mk, self.mask(m0, s), what + ": persistent mask under no_mask")
            else:
                _same(mk, want_m, what + ": persistent mask")
            self.count_tiles(g, want_m)
            off = it["fl"].get("filter_off", False)
            fh, fv = it["fl"].get("flip_h", False), it["fl"].get("flip_v", False)
            if vcam:                                      # the device's own persistent mask: blend -> flip -> resize [-> pack]
                C = it["seen"] if off else oracle.alpha_blend(it["bg"], it["seen"], mk)
                want = oracle.resize_linear(_flip(oracle, C, fh, fv), vcam[0], vcam[1])
            else:
                want = _flip(oracle, it["seen"] if off else oracle.alpha_blend(it["bg"], it["seen"], want_m), fh, fv)
            if yuyv:
                want = oracle.bgr_to_yuyv(want)
            _same(got, want, what + (": output" if vcam else ": composite"))
        if prep:
            self.check_prep(tag, items)
        if self.twins:
            self.check_twins(tag, items, outs, of1, yuyv, no_mask)
        return res, of1, m1

    def count_tiles(self, g, mask):
        x, y, w, h = self.geo[g]["roi"]
        for ty in range(y, y + h, rc.TILE_H):
            for tx in range(x, x + w, rc.TILE_W):
                t = mask[ty:min(ty + rc.TILE_H, y + h), tx:min(tx + rc.TILE_W, x + w)]
                lo = int(t.min())
                self.tiles[g][0 if (lo == int(t.max()) and lo in (0, 255)) else 1] += 1

    def check_prep(self, tag, items):
        """c. the network input as prep wrote it, position by position: positions are ordered by class, the caller's order kept within a class (the stable counting
        sort of geoms_front).  The oracle's prep is f32 q * scale: q is recovered as rint(prep * 255), exact for either form of the normalisation once prep * 255
        is seen to lie within 1e-3 of an integer."""
        got = self.mg.input_u8()[:len(items)].cpu().numpy()              # (raises where the model does not take the byte path: a failure, not a skip)
        order = sorted(range(len(items)), key=lambda i: items[i]["g"])   # (sorted is stable)
        for j, i in enumerate(order):
            it = items[i]
            b = self.oc[it["g"]].prep(it["seen"]).astype(np.float64) * 255.0
            q = np.rint(b)
            assert np.abs(b - q).max() < 1e-3, "%s: the oracle's prep * 255 is %g away from an integer" % (tag, np.abs(b - q).max())
            want = np.zeros(q.shape[:2] + (4,), np.uint8)
            want[..., :3] = q                                             # word = R | G << 8 | B << 16
            _same(got[j], want, "%s stream %d (%dx%d%s), position %d: network input" % ((tag, it["s"]) + it["size"] + (", YUYV" if it["yin"] else "", j)))

    def check_twins(self, tag, items, outs, of1, yuyv, no_mask):
        """d. a class's streams on a one-geometry context (code the oracle already judges), stepped with step_mixed on the same frames and settings — one call per
        pixel format, which the mixed step takes batch-wide: composites and state byte-equal every call"""
        S = self.bs.StreamSetting
        for g, tw in self.twins.items():
            W, H = self.data.sizes[g]
            for fmt in (False, True):
                pos = [i for i, it in enumerate(items) if it["g"] == g and it["yin"] == fmt]
                if not pos:
                    continue
                want = torch.full((len(pos), H, W, 2 if yuyv else 3), SENTINEL, dtype=torch.uint8, device="cuda")
                tw.step_mixed(torch.stack([items[i]["dev"] for i in pos]), want, [S(bg=items[i]["d_bg"], **items[i]["fl"]) for i in pos],
                              ids=[items[i]["s"] - self.data.first[g] for i in pos], yuyv=yuyv, no_mask=no_mask, yuyv_in=fmt)
                for k, i in enumerate(pos):
                    _same(outs[i].cpu().numpy(), want[k].cpu().numpy(), "%s stream %d (%dx%d): composite against the one-geometry twin" % (tag, items[i]["s"], W, H))
            st = tw.ofinal().cpu().numpy()
            for k in range(self.classes[g]["n"]):
                _same(of1[self.data.first[g] + k], st[k], "%s stream %d (%dx%d): state against the one-geometry twin" % (tag, self.data.first[g] + k, W, H))

    def streams_of(self, g):
        return list(range(self.data.first[g], self.data.first[g] + self.classes[g]["n"]))

    def close(self):
        for c in [self.mg] + list(self.twins.values()) + self.oc:
            c.close()


def _everyone_reversed(r):
    """every stream, class order reversed and interleaved: the first stream of the last class, of the one before, ..., then the second streams"""
    return [r.data.first[g] + k for k in range(max(c["n"] for c in r.classes)) for g in reversed(range(len(r.classes))) if k < r.classes[g]["n"]]


def _first_calls(r):
    """calls 1-3 of the step schedule: (t, ids, arguments)"""
    rng = np.random.default_rng(2024)
    middle = len(r.classes) // 2
    perm = [int(s) for s in rng.permutation(r.n)]
    return [(1, _everyone_reversed(r), dict(plain=True, prep=True)),
            (2, perm, dict(prep=True)),
            (3, [int(s) for s in rng.permutation(r.n) if r.data.cls_of[s] != middle], dict())]


# ---- a. the classes ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rc.FLEETS))
def test_classes_are_accepted(bs, oracle, name):
    """with_geometries takes every class (each matrix row among them is a fused tile row: a refusal here means bsx_new_geoms' rule and the matrix disagree), and
    geometries() gives the oracle's rectangles, which are the table's"""
    r = Run(bs, oracle, name)
    try:
        r.check_classes()
    finally:
        r.close()


# ---- b, c, d. the step schedule ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.STEP_FLEETS)
def test_step_schedule(bs, oracle, name):
    from backscrub_amd.api import BsxError
    twin = [g for g, c in enumerate(rc.FLEETS[name]["classes"]) if c["down"] == 2 or c["size"][1] > c["size"][0]] if name in ("lite8", "mlkit4") else []
    r = Run(bs, oracle, name, twin)
    try:
        r.check_classes()
        last = len(r.classes) - 1
        everyone = list(range(r.n))
        for t, ids, kw in _first_calls(r):                 # 1 everyone, reversed and interleaved; 2 a seeded permutation, the settings cycling; 3 no middle class
            r.call(t, ids, **kw)
        r.call(4, r.streams_of(last)[::-1])                # 4 only the last class
        r.call(5, [r.data.first[0]])                       # 5 only one stream of the first class
        r.call(6, everyone, yuyv=True)                     # 6 everyone, packed composites
        r.whole().fill_(0x5A)                              # 7 everyone, no_mask: any byte the call stores into the persistent masks shows
        r.call(7, everyone[::-1], no_mask=True)
        assert bool((r.whole() == 0x5A).all()), "%s call 7: the persistent masks changed under no_mask" % name
        r.whole().fill_(255)                               # as bsx_new_geoms left them: the ROI is rewritten by the next storing call, outside it 255 stays
        # 8 everyone; the even streams of the classes whose prep reads YUYV deliver it
        admitted = [g for g, c in enumerate(r.classes) if rc.yuyv_in_admitted(c)]
        yin = {s for g in admitted for s in r.streams_of(g) if s % 2 == 0}
        assert yin and len(admitted) < len(r.classes)
        r.call(8, everyone, yin=yin, prep=True)
        # ... and a YUYV item of a class whose down-scale is the 2x2 area mean is refused, and nothing changes
        g2 = [g for g, c in enumerate(r.classes) if c["down"] == 2][0]
        other = admitted[0]
        ids = [r.data.first[other], r.data.first[g2]]
        S = bs.StreamSetting
        (W, H), (W2, H2) = r.data.sizes[other], r.data.sizes[g2]
        frames = [_dev(r.data.frame(ids[0], 9)), torch.zeros((H2, W2, 2), dtype=torch.uint8, device="cuda")]
        outs = [torch.full((H, W, 3), SENTINEL, dtype=torch.uint8, device="cuda"), torch.full((H2, W2, 3), SENTINEL, dtype=torch.uint8, device="cuda")]
        of0, m0 = r.mg.ofinal().clone(), r.whole().clone()
        with pytest.raises(BsxError, match="2x2 area"):
            r.mg.step_geoms(ids, frames, outs, [S(bg=r.data.bg("own", ids[0])[1]), S(bg=r.data.bg("own", ids[1])[1], yuyv_in=True)])
        torch.cuda.synchronize()
        assert torch.equal(r.mg.ofinal(), of0) and torch.equal(r.whole(), m0), "%s: the refused call changed state or masks" % name
        assert all(bool((o == SENTINEL).all()) for o in outs), "%s: the refused call wrote an output" % name
        # the checks above are not trivial: some state the device held had both sides of the threshold, or a byte that is neither 0 nor 255
        assert r.lively, name
    finally:
        r.close()


# ---- e. the step at the virtual camera's geometry ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.STEP_FLEETS)
def test_vcam_schedule(bs, oracle, name):
    r = Run(bs, oracle, name)
    try:
        rng = np.random.default_rng(77)
        middle, last = len(r.classes) // 2, len(r.classes) - 1
        yin = {s for g, c in enumerate(r.classes) if rc.yuyv_in_admitted(c) for s in r.streams_of(g) if s % 2 == 0}
        t = 0
        for k, (ow, oh, yuyv) in enumerate(VCAM_SIZES):
            for ids, kw in (([int(s) for s in rng.permutation(r.n)], dict(yin=yin) if k == 1 else {}),
                            ([int(s) for s in rng.permutation(r.n) if r.data.cls_of[s] != middle], {}),
                            (r.streams_of(last), {})):
                t += 1
                r.call(t, ids, yuyv=yuyv, vcam=(ow, oh), **kw)
        assert r.lively, name
    finally:
        r.close()


# ---- f. the one-XCD-per-frame order inside a class segment ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.XCD_FLEETS)
def test_xcd_order_inside_a_class_segment(bs, oracle, name):
    """the second class's rows share cache lines, so its segment of the tile grid takes the one-XCD-per-frame order: 11 positions = 8 in that order + 3 in the
    remainder branch (then 9 = 8 + 1), behind a first class whose workgroups are no multiple of 8"""
    r = Run(bs, oracle, name)
    try:
        r.check_classes()
        rng = np.random.default_rng(5)
        second = r.streams_of(1)
        assert len(second) == 11
        r.call(1, [int(s) for s in rng.permutation(r.n)], prep=True)
        r.call(2, [second[int(i)] for i in rng.permutation(11)[:9]], prep=True)
        r.call(3, [int(s) for s in rng.permutation(r.n)])
        r.call(4, [int(s) for s in rng.permutation(r.n)], vcam=(160, 90))
        assert r.lively, name
    finally:
        r.close()


# ---- g. the uniform-tile path on these classes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lite8", "full6"])
def test_uniform_tile_path_equals_the_general_one(bs, oracle, monkeypatch, capsys, name):
    """a second context created under BSX_NO_UNIFORM_TILES (read when the context is created: no class bytes, every tile takes the general body) steps calls 1-3
    on the same frames: composites, masks and state equal the default context's.  So that the comparison is not empty, the default context's oracle-implied
    masks must hold both kinds of 128 x 32 tile, constant 0 / 255 and not — a condition on the inputs (one stream shows a flat colour), not on the kernel."""
    a = Run(bs, oracle, name)
    monkeypatch.setenv("BSX_NO_UNIFORM_TILES", "1")
    b = Run(bs, oracle, name)
    try:
        for t, ids, kw in _first_calls(a):
            kw = {k: v for k, v in kw.items() if k != "prep"}
            ra, ofa, ma = a.call(t, ids, **kw)
            rb, ofb, mb = b.call(t, ids, judge=False, **kw)
            for s in ids:
                W, H = a.data.sizes[a.data.cls_of[s]]
                what = "%s call %d stream %d (%dx%d), general path against the default" % (name, t, s, W, H)
                _same(rb[s], ra[s], what + ": composite")
                _same(b.mask(mb, s), a.mask(ma, s), what + ": persistent mask")
                _same(ofb[s], ofa[s], what + ": state")
        with capsys.disabled():
            print()
            for c, (u, g) in zip(a.classes, a.tiles):
                print("%s %dx%d: %d mask tiles constant 0 / 255, %d not" % ((name,) + c["size"] + (u, g)))
        assert sum(u for u, _ in a.tiles) > 0 and sum(g for _, g in a.tiles) > 0, a.tiles
    finally:
        a.close()
        b.close()
