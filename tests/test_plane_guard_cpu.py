"""The guarded arena's checker (tests/plane_guard.py) shown able to fail: one changed word of every violation class, planted in a copy
of a clean buffer, is reported with its class and position; so is one owned pixel left unwritten; a clean buffer reports nothing.
Both element types, a pitch equal to the width and a padded one, one image and three."""
import numpy as np
import pytest

import plane_guard as pg

W, H = 20, 7


def arena(dtype, p, nimg):
    """src (an input), an interleaved {Lx, Ly} plane, det (both written by the imagined call) and tmp (not to be touched)"""
    a = pg.Arena(dtype, [("src", W, H, p), ("dxy", W, H, p, 2), ("det", W, H, p), ("tmp", W, H, p)], nimg)
    rng = np.random.default_rng(p + nimg)
    a.put("src", rng.integers(1, 1000, (nimg, H, W)).astype(dtype))
    return a


def written(a):
    """the buffer a well-behaved call leaves: every owned pixel of dxy and det written, nothing else"""
    buf = a.buffer()
    a.owned(buf, "dxy")[...] = 3
    a.owned(buf, "det")[...] = 4
    return buf


CASES = [(dtype, p, nimg) for dtype in (np.float32, np.int32) for p in (W, W + 4) for nimg in (1, 3)]
IDS = [f"{np.dtype(d).name}-p{p}-n{n}" for d, p, n in CASES]


@pytest.mark.parametrize("dtype,p,nimg", CASES, ids=IDS)
def test_layout_and_fill(dtype, p, nimg):
    a = arena(dtype, p, nimg)
    assert a.stride % 4 == 0 and a.size == a.stride * nimg and all(a.offset(n) % 4 == 0 for n in a.order)
    assert a.guard >= pg.GUARD_ROWS * 2 * p                                 # rows of the widest plane, the interleaved one
    offs = [a.offset(n) for n in a.order]
    assert offs[0] == a.guard and offs[1] - (offs[0] + H * p) == a.guard and a.stride - (offs[3] + H * p) >= a.guard
    buf = a.buffer()
    bits = buf.view(np.uint32)
    word = pg.POISON_F32_BITS if dtype == np.float32 else pg.POISON_I32
    assert (bits != word).sum() == nimg * W * H                             # the input pixels and nothing else
    assert (a.owned(bits, "src") != word).all()
    if p > W:
        assert (a.rows(bits, "src")[:, :, W:] == word).all()                # an input's pad columns are poisoned too
    assert a.address(1 << 20, "det", nimg - 1) == (1 << 20) + 4 * ((nimg - 1) * a.stride + a.offset("det"))


@pytest.mark.parametrize("dtype,p,nimg", CASES, ids=IDS)
def test_clean_buffer_reports_nothing(dtype, p, nimg):
    a = arena(dtype, p, nimg)
    buf = written(a)
    rep = a.violations(buf, ["dxy", "det"])
    assert rep.count == 0 and list(rep) == [] and rep.classes == {}
    assert a.unwritten(buf, "dxy") == [] and a.unwritten(buf, "det") == []
    assert len(a.unwritten(buf, "tmp")) == nimg * W * H                     # (never written: every pixel still poison)


def plants(a, p, nimg):
    """(class, word index within the slot, image, [images the call was given], expected (plane, row, column))"""
    img = nimg - 1
    every = list(range(nimg))
    out = [(pg.BELOW, a.offset("det") + H * p + 2, img, every, ("det", H, 2)),
           (pg.BELOW, a.offset("tmp") + H * p + a.guard - 1, img, every, ("tmp", H + (a.guard - 1) // p, (a.guard - 1) % p)),
           (pg.FRONT, a.offset("src") - 1, img, every, ("src", -1, p - 1)),
           (pg.FRONT, a.offset("det") - p + 3, img, every, ("det", -1, 3)),
           (pg.FRONT, 0, img, every, ("src", -(a.guard // p), 0 if a.guard % p == 0 else p - a.guard % p)),
           (pg.OTHER_PLANE, a.offset("tmp") + 3 * p + 5, img, every, ("tmp", 3, 5)),
           (pg.OTHER_PLANE, a.offset("src") + 2 * p + 1, img, every, ("src", 2, 1))]             # an input pixel overwritten
    if p > W:
        out += [(pg.PAD, a.offset("det") + 4 * p + W, img, every, ("det", 4, W)),
                (pg.PAD, a.offset("dxy") + 2 * (2 * p) + 2 * W + 1, img, every, ("dxy", 2, 2 * W + 1)),
                (pg.OTHER_PLANE, a.offset("tmp") + p - 1, img, every, ("tmp", 0, p - 1))]        # padding of a plane not written
    if nimg > 1:
        out += [(pg.OTHER_IMAGE, a.offset("det") + 5, 2, [0, 1], ("det", 0, 5)),
                (pg.OTHER_IMAGE, 1, 1, [0], ("src", -(a.guard // p) + (1 // p), 1 % p) if a.guard % p == 0 else None)]
    return out


@pytest.mark.parametrize("dtype,p,nimg", CASES, ids=IDS)
def test_every_class_is_reported_with_its_position(dtype, p, nimg):
    a = arena(dtype, p, nimg)
    clean = written(a)
    seen = set()
    for cls, k, img, given, where in plants(a, p, nimg):
        buf = clean.copy()
        if cls == pg.OTHER_IMAGE:                                           # the call was given fewer images: the others stay as they were
            for i in set(range(nimg)) - set(given):
                buf[i * a.stride:(i + 1) * a.stride] = a.init[i * a.stride:(i + 1) * a.stride]
        buf.view(np.uint32)[img * a.stride + k] ^= 0x00000100               # one changed word (for float: another NaN payload)
        rep = a.violations(buf, ["dxy", "det"], images=given)
        assert rep.count == 1 and rep.classes == {cls: 1} and len(rep) == 1, (cls, k, str(rep))
        v = rep[0]
        assert v.cls == cls and v.image == img, (cls, k, v)
        if where:
            assert (v.plane, v.row, v.col) == where, (cls, k, v, where)
        assert v.got == int(buf.view(np.uint32)[img * a.stride + k])
        seen.add(cls)
    assert seen == set(pg.CLASSES) - ({pg.PAD} if p == W else set()) - ({pg.OTHER_IMAGE} if nimg == 1 else set())


@pytest.mark.parametrize("dtype,p,nimg", CASES, ids=IDS)
def test_the_p_equals_w_overrun_lands_in_the_next_row(dtype, p, nimg):
    """a store to column w of an owned row: padding when p > w; with p == w it is pixel 0 of the next row, which only the comparison
    with the oracle sees -- except behind the last row, where it is the first word below the plane"""
    a = arena(dtype, p, nimg)
    buf = written(a)
    buf.view(np.uint32)[a.offset("det") + (H - 1) * p + W] ^= 0x100
    rep = a.violations(buf, ["dxy", "det"])
    assert rep.count == 1 and rep[0].cls == (pg.BELOW if p == W else pg.PAD)


@pytest.mark.parametrize("dtype,p,nimg", CASES, ids=IDS)
def test_an_unwritten_pixel_is_reported(dtype, p, nimg):
    a = arena(dtype, p, nimg)
    buf = written(a)
    img = nimg - 1
    a.owned(buf, "det")[img, 5, W - 1] = a.poison
    a.owned(buf, "dxy")[0, 0, 2 * W - 1] = a.poison
    assert a.unwritten(buf, "det") == [(img, 5, W - 1)]
    assert a.unwritten(buf, "dxy") == [(0, 0, 2 * W - 1)]
    assert a.violations(buf, ["dxy", "det"]).count == 0                     # (not a violation: a skipped pixel changes nothing)


def test_many_violations_are_counted_and_the_first_few_listed():
    a = arena(np.int32, W + 4, 1)
    buf = written(a)
    a.rows(buf, "det")[0, :, W:] = 7                                        # every pad column of det
    a.rows(buf, "tmp")[...] = 9
    rep = a.violations(buf, ["dxy", "det"], first=3)
    assert rep.classes == {pg.PAD: 4 * H, pg.OTHER_PLANE: (W + 4) * H} and rep.count == 4 * H + (W + 4) * H
    assert len(rep) == 6 and [v.cls for v in rep] == [pg.PAD] * 3 + [pg.OTHER_PLANE] * 3
    assert (rep[0].plane, rep[0].row, rep[0].col, rep[0].got) == ("det", 0, W, 7)


def test_refusals():
    with pytest.raises(ValueError):
        pg.Arena(np.float32, [("a", 8, 4, 8)], guard_rows=8)               # thinner guards than the kernels' warm-up
    with pytest.raises(TypeError):
        pg.Arena(np.float64, [("a", 8, 4, 8)])
    with pytest.raises(ValueError):
        pg.Arena(np.float32, [("a", 9, 4, 8)])                              # pitch below the width
    a = pg.Arena(np.float32, [("a", 8, 4, 8)])
    with pytest.raises(TypeError):
        a.put("a", np.zeros((4, 8), np.int32))
    with pytest.raises(KeyError):
        a.violations(a.buffer(), ["b"])


def test_u8_padding():
    u = pg.padded_u8(np.ones((2, 3, 5), np.uint8), 8)
    assert u.shape == (2, 3, 8) and (u[..., :5] == 1).all() and (u[..., 5:] == pg.POISON_U8).all()
