"""The value-domain inputs (tests/value_domain.py) and the oracle on them, checked without a GPU: the conditions that keep
tests/test_gpu_value_domain.py from passing for the wrong reason.

  * generators are deterministic, float32, in their declared range, and not quantised
  * tier A: every oracle stage output and every plane of the pipeline is finite -- so the comparison rule's "both NaN" clause can
    never apply to a tier-A case (stage cases with one of the two extreme contrast factors KC_EXTREME count as tier B whatever the
    input: ikc = inf times a zero gradient is NaN)
  * tiers B and C: every stage output and the pipeline's level (0, 0) keep at least half of their pixels non-NaN; every tier-C
    input makes NaNs at pixels that were finite in the input
  * `spikes` / `spikes_strip`: conductivity denominators on both sides of 2^64 inside one 64-pixel row segment / a whole 256-pixel
    strip at or above 2^64, from the oracle's own low-pass, Scharr differences and ikc
  * `sub_squares`: subnormal squared gradients, conductivity denominators minus one, determinants and keypoint responses occur in
    the oracle's own intermediates and outputs, next to normal ones -- `tiny` and `denormal` only reach the linear kernels
  * the oracle against a float64 statement of lowpass, hessian, PM_G2 flow and one FED step, within a DERIVED bound
"""
import hashlib
import json

import numpy as np
import pytest

import value_domain as vd

SEED = 5
U = 2.0 ** -24                                   # unit roundoff of float32


@pytest.fixture(scope="module", autouse=True)
def _quiet():
    with np.errstate(all="ignore"):
        yield


def planes_of(okz, r):
    return [((kind, o, s), okz.plane(r, kind, o, s)) for o in range(r.noct) for s in range(r.ms) for kind in (0, 1, 2, 3)]


# ------------------------------------------------------------------------------------------------ the generators
@pytest.mark.parametrize("name", list(vd.GENERATORS))
def test_generator_is_deterministic_and_in_range(name):
    g = vd.GENERATORS[name]
    a, b = g(260, 203, SEED), g(260, 203, SEED)
    assert a.dtype == np.float32 and a.shape == (203, 260) and a.flags.c_contiguous
    assert a.tobytes() == b.tobytes()
    if name != "ulp_noise":
        assert g(260, 203, SEED + 1).tobytes() != a.tobytes() or name == "ramp"
    if g.tier == "A":
        assert np.isfinite(a).all() and a.min() >= 0.0 and a.max() <= 1.0
    elif g.tier == "B":
        assert np.isfinite(a).all() and (a.min() < 0.0 or a.max() > 1.0)
    else:
        assert not np.isfinite(a).all() and np.isfinite(a).mean() > 0.95


def test_class_properties():
    w, h = 320, 240
    base = vd.hdr(w, h, SEED)
    # full-mantissa content: (nearly) every pixel its own value, and the low significand bits are in use -- uint8 / 255 has 256 values
    inner = base[(base > 0) & (base < 1)]
    assert len(np.unique(inner)) > 0.9 * inner.size > 60000
    assert len(np.unique(inner.view(np.uint32) & 0xFF)) == 256
    r = vd.ramp(w, h, SEED)
    assert len(np.unique(r)) > 0.9 * r.size
    u = vd.ulp_noise(w, h, SEED)
    assert set(np.unique(u.view(np.uint32))) == {0x3F000000, 0x3F000001}
    d = vd.denormal(w, h, SEED)
    assert d.max() < np.finfo(np.float32).tiny and (d > 0).mean() > 0.99           # subnormal, and not flushed by the generator
    z = vd.signed_zero(w, h, SEED).view(np.uint32)
    assert (z == 0).sum() > 500 and (z == 0x80000000).sum() > 500
    s = vd.spikes(w, h, SEED)
    assert s.max() == np.float32(1e25) and np.sort(s.ravel())[-len(vd.spike_sites(w, h))] >= np.float32(1e12)
    f = vd.nan_frame(w, h, SEED)
    assert np.isnan(f[0]).all() and np.isnan(f[-1]).all() and np.isnan(f[:, 0]).all() and np.isnan(f[:, -1]).all()
    assert np.isfinite(f[1:-1, 1:-1]).all()


def test_comparison_rule():
    a = np.array([1.0, -0.0, np.nan, np.inf, 3.0], np.float32)
    b = a.copy()
    b.view(np.uint32)[2] = 0xFFC00001                                              # another NaN: sign and payload are free
    assert vd.same_bits(a, b) == (True, 1, None)
    b[1] = 0.0                                                                     # +0 is not -0
    assert vd.same_bits(a, b) == (False, 1, (1,))
    b[1], b[4] = -0.0, np.nan                                                      # NaN against a number
    assert vd.same_bits(a, b)[0] is False
    assert vd.same_bits(a, a) == (True, 1, None)


# ------------------------------------------------------------------------------------------------ tier conditions, stage level
@pytest.mark.parametrize("name", list(vd.GENERATORS))
def test_tier_conditions_of_the_stage_cases(okz, name):
    g = vd.GENERATORS[name]
    ncases = 0
    for w, h in vd.STAGE_SHAPES:
        dense = g(w, h, SEED)
        a = vd.pitched(dense)
        made_nan = False
        for op, label, extreme, _, outs in vd.oracle_stage_cases(okz, a, w):
            ncases += 1
            for nm, o, ww in outs:
                if o.dtype != np.float32:
                    continue
                v = o[:, :ww]
                where = f"{name} {w}x{h} {op} {label} {nm}"
                if g.tier == "A" and not extreme:
                    assert np.isfinite(v).all(), where
                if g.tier != "A":
                    assert np.isnan(v).mean() <= 0.5, where
                if g.tier == "C" and v.shape == dense.shape:
                    made_nan |= bool((np.isnan(v) & np.isfinite(dense)).any())
        assert made_nan or g.tier != "C", f"{name} {w}x{h}: no NaN spread to a pixel that was finite in the input"
    assert ncases == 3 * (len(vd.LOWPASS) + 1 + 1 + 2 * 4 * (2 + len(vd.KC_EXTREME)) + len(vd.TAU_LISTS) + len(vd.HESS_STEPS))


# ------------------------------------------------------------------------------------------------ tier conditions, pipeline level
@pytest.mark.parametrize("w,h", [(320, 240), (1284, 200)])
@pytest.mark.parametrize("name", list(vd.GENERATORS))
def test_tier_conditions_of_the_pipeline(okz, name, w, h):
    g = vd.GENERATORS[name]
    p = (w + 127) // 128 * 128
    dense = g(w, h, SEED)
    r = okz.detect_and_compute(vd.pitched(dense, p), w, max_pts=20000, keep_arena=True)
    planes = planes_of(okz, r)
    if g.tier == "A":
        assert np.isfinite(r.kcontrast)
        for key, v in planes:
            assert np.isfinite(v).all(), (name, key)
        for f in ("x", "y", "response", "size", "angle"):
            assert np.isfinite(r.points[f]).all()
    else:
        for key, v in planes:
            if key[1:] == (0, 0):
                assert np.isnan(v).mean() <= 0.5, (name, key)
        if g.tier == "C":
            assert any((np.isnan(v) & np.isfinite(dense)).any() for key, v in planes if key[1] == 0)
    assert len(r.points) < 20000


def test_low_thresholds_come_from_the_oracle(okz):
    """classes far below the default detector threshold: LOW_DTHRESHOLD gives the oracle > 50 keypoints where one exists; where the
    determinants underflow to zero no threshold can"""
    w, h, p = 320, 240, 384
    for name in ("dark", "sub_squares", "ulp_noise", "tiny", "denormal"):
        a = vd.pitched(vd.GENERATORS[name](w, h, SEED), p)
        r = okz.detect_and_compute(a, w, keep_arena=True)
        assert len(r.points) == 0
        if name in vd.LOW_DTHRESHOLD:
            assert len(okz.detect_and_compute(a, w, okz.default_params(dthreshold=vd.LOW_DTHRESHOLD[name])).points) > 50
        else:
            assert all(not v.any() for key, v in planes_of(okz, r) if key[0] == 1), name      # every determinant is +-0
            assert any(v.any() for key, v in planes_of(okz, r) if key[0] == 0)                # ... of planes that are not trivial
    assert set(vd.LOW_DTHRESHOLD) == {"dark", "sub_squares"}


# ------------------------------------------------------------------------------------------------ spikes: both sides of 2^64
def scharr32(sm, w):
    """dx, dy of scharr_dxdy (akaze_oracle.c), float32 operation by operation in the same order, reflect-101"""
    v = sm[:, :w]
    h = v.shape[0]
    xm, xp = np.abs(np.arange(w) - 1), np.where(np.arange(w) + 1 < w, np.arange(w) + 1, 2 * w - 2 - (np.arange(w) + 1))
    ym, yp = np.abs(np.arange(h) - 1), np.where(np.arange(h) + 1 < h, np.arange(h) + 1, 2 * h - 2 - (np.arange(h) + 1))
    r0, r1, r2 = v[ym], v, v[yp]
    f10, f3 = np.float32(10), np.float32(3)
    dx = f10 * (r1[:, xp] - r1[:, xm]) + f3 * (((r0[:, xp] + r2[:, xp]) - r0[:, xm]) - r2[:, xm])
    dy = f10 * (r2 - r0) + f3 * (((r2[:, xm] + r2[:, xp]) - r0[:, xm]) - r0[:, xp])
    return dx, dy


def denominators(okz, a, w, kc):
    """1 + dif2 of the PM_G2 conductivity, float32, from the oracle's low-pass; checked against okz.flow before it is trusted"""
    sm = okz.lowpass(a, w, 1.0, 2)
    dx, dy = scharr32(sm, w)
    ikc = np.float32(1.0) / (np.float32(kc) * np.float32(kc))
    den = np.float32(1.0) + ikc * (dx * dx + dy * dy)
    ok, _, first = vd.same_bits(np.float32(1.0) / den, okz.flow(sm, w, 1, float(kc))[:, :w])
    assert ok, f"the numpy restatement of the denominators differs from okz.flow at {first}"
    return den


@pytest.mark.parametrize("w,h", vd.STAGE_SHAPES + [(320, 240), (1284, 200)])
def test_spikes_put_both_sides_of_2_64_into_one_segment(okz, w, h):
    a = vd.pitched(vd.spikes(w, h, SEED), (w + 127) // 128 * 128)
    kc = vd.own_kcontrast(okz, a, w)[0]
    assert np.isfinite(kc) and 0.01 < kc < 10                                      # the spikes stay off the contrast lattice
    den = denominators(okz, a, w, kc)
    nseg = w // 64
    seg = den[:, :nseg * 64].reshape(h, nseg, 64)
    above, below = (seg >= vd.TWO64), (seg < vd.TWO64)
    mixed = above.any(axis=2) & below.any(axis=2)
    assert mixed.sum() >= 8
    finite_above = (seg >= vd.TWO64) & np.isfinite(seg)
    assert (finite_above.any(axis=2) & below.any(axis=2)).any()                    # finite values >= 2^64 next to fast lanes ...
    assert (np.isinf(seg).any(axis=2) & below.any(axis=2)).any()                   # ... and inf next to fast lanes
    # neighbours: some 4-pixel group (one lane of the streaming kernels) above, the next one below
    lane = seg.reshape(h, nseg, 16, 4)
    la, lb = (lane >= vd.TWO64).any(axis=3), (lane < vd.TWO64).all(axis=3)
    assert (la[:, :, :-1] & lb[:, :, 1:]).any() and (lb[:, :, :-1] & la[:, :, 1:]).any()


@pytest.mark.parametrize("w,h", vd.STAGE_SHAPES + [(320, 240), (1284, 200)])
def test_spikes_strip_puts_a_whole_strip_above_2_64(okz, w, h):
    a = vd.pitched(vd.spikes_strip(w, h, SEED), (w + 127) // 128 * 128)
    kc = vd.own_kcontrast(okz, a, w)[0]
    assert np.isfinite(kc) and 0.01 < kc < 10
    den = denominators(okz, a, w, kc)
    n = min(w, 256)
    rows = (den[:, :n] >= vd.TWO64).all(axis=1)
    assert rows.sum() >= 4 and (den < vd.TWO64).all(axis=1).sum() >= h // 2


# ------------------------------------------------------------------------------------------------ sub_squares: subnormal squares and products
TINY = np.finfo(np.float32).tiny                 # 2^-126, the smallest normal float32


def subnormal(a):
    a = np.abs(a)
    return (a < TINY) & (a > 0)


@pytest.mark.parametrize("w,h", vd.STAGE_SHAPES + [(320, 240), (1284, 200)])
def test_sub_squares_reaches_the_subnormal_range_of_every_product(okz, w, h):
    """the denormal precondition is only tested if subnormal values occur where a kernel could flush them: in
    the squares of the Scharr differences, their sum, the conductivity argument, the determinant -- and normal values beside them"""
    p = (w + 127) // 128 * 128
    a = vd.pitched(vd.sub_squares(w, h, SEED), p)
    n = w * h
    assert a[:, :w].max() > 1e-19 and not subnormal(a).any()                       # the plane itself is ordinary
    kc, hmax, hist, sm = vd.own_kcontrast(okz, a, w)
    dx, dy = scharr32(sm, w)
    q = dx * dx + dy * dy
    for nm, v in (("dx * dx", dx * dx), ("dy * dy", dy * dy), ("dx * dx + dy * dy", q)):
        assert subnormal(v).sum() > n // 4 and (np.abs(v) >= TINY).sum() > n // 10, nm
    # den - 1 = ikc * q at KC_UNIT is q itself (the restatement is checked against okz.flow inside denominators())
    den = denominators(okz, a, w, vd.KC_UNIT)
    assert (den == 1).all()
    # at the class's own contrast factor (the floor: hmax stays 0.03) ikc * q is normal again; at kc = 1e-30 it is inf where q > 0 and
    # NaN where q == 0 -- a flushed square would turn an inf into a NaN, i.e. a conductivity of 0 into a NaN
    assert kc == np.float32(1e-4) and hmax == np.float32(0.03) and np.count_nonzero(hist) == 1
    g = okz.flow(sm, w, 1, 1e-30)[:, :w]
    assert (g[subnormal(q)] == 0).all() and np.isnan(g[q == 0]).all() and (q == 0).any()
    for step in vd.HESS_STEPS:
        det = okz.hessian(a, w, step)[2][:, :w]
        assert subnormal(det).sum() > n // 2 and (np.abs(det) >= TINY).any(), step
    if (w, h) == (320, 240):
        r = okz.detect_and_compute(a, w, okz.default_params(dthreshold=vd.LOW_DTHRESHOLD["sub_squares"]), keep_arena=True)
        dets = np.concatenate([v.ravel() for key, v in planes_of(okz, r) if key[0] == 1])
        assert subnormal(dets).mean() > 0.5 and (np.abs(dets) >= TINY).any()
        resp = r.points["response"]
        assert subnormal(resp).sum() > 50 and (np.abs(resp) >= TINY).any()         # the threshold 1e-39 is subnormal too


# ------------------------------------------------------------------------------------------------ the oracle against float64 statements
# Bound per pixel: k * 2^-24 * sum|term|.  Standard forward analysis: a float32 expression of k rounded operations whose exact value
# is a sum of terms t_i returns sum t_i (1 + d_i) with |d_i| <= (1 + u)^k_i - 1, k_i <= k the operations term i passes through; k_i
# is strictly smaller than k in every statement below, which covers the second-order remainder k^2 u^2.  Products of two such sums
# (determinant, squared gradient) expand into the products of the terms, so their sum|term| is the product of the factors' sums.
# Inputs that are the oracle's own float32 results of an earlier statement (the row pass inside lowpass is not: it is part of the
# statement) are taken as exact: each kernel statement is checked on its own.
F64_CLASSES = ("hdr", "ramp", "x255", "offset", "dark")
F64_SHAPES = [(211, 173), (128, 96)]


def reflect(n, d):
    i = np.arange(n)
    c = i + d
    return np.abs(i - d), np.where(c < n, c, 2 * n - 2 - c)


def lowpass64(v, taps):
    """gConv2d (akazed.cu:204-290) in float64 with the float32 taps: value and sum of |terms|"""
    h, w = v.shape
    k = taps.astype(np.float64)

    def rows(x):
        out = x * k[0]
        for i in range(1, len(k)):
            m, p = reflect(w, i)
            out = out + k[i] * (x[:, m] + x[:, p])
        return out

    def cols(x):
        out = x * k[0]
        for i in range(1, len(k)):
            m, p = reflect(h, i)
            out = out + k[i] * (x[m] + x[p])
        return out
    return cols(rows(v)), cols(rows(np.abs(v)))


def stencil64(v, step, fac1, fac2):
    """gDerivate (akazed.cu:1267-1296) in float64: (d/dx, d/dy) and their sums of |terms|"""
    h, w = v.shape
    xm, xp = reflect(w, step)
    ym, yp = reflect(h, step)
    ul, uc, ur = v[ym][:, xm], v[ym], v[ym][:, xp]
    cl, cr = v[:, xm], v[:, xp]
    ll, lc, lr = v[yp][:, xm], v[yp], v[yp][:, xp]
    dx = fac1 * (ur + lr - ul - ll) + fac2 * (cr - cl)
    dy = fac1 * (lr + ll - ur - ul) + fac2 * (lc - uc)
    a = np.abs
    sx = fac1 * (a(ur) + a(lr) + a(ul) + a(ll)) + fac2 * (a(cr) + a(cl))
    sy = fac1 * (a(lr) + a(ll) + a(ur) + a(ul)) + fac2 * (a(lc) + a(uc))
    return dx, dy, sx, sy


def check(name, got32, ref64, sum_terms, k):
    err = np.abs(got32.astype(np.float64) - ref64)
    bound = k * U * sum_terms
    worst = np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0)))
    assert worst <= 1.0, f"{name}: error / derived bound = {worst:.3f} (k = {k})"
    return worst


@pytest.mark.parametrize("w,h", F64_SHAPES)
@pytest.mark.parametrize("name", F64_CLASSES)
def test_oracle_against_float64_statements(okz, name, w, h):
    a = vd.pitched(vd.GENERATORS[name](w, h, SEED))
    v = a[:, :w].astype(np.float64)
    # ---- lowpass: each pass is 1 product + R x (add, multiply, accumulate) = 1 + 3R operations; two passes: k = 2 (1 + 3R)
    for var, R in vd.LOWPASS:
        ref, s = lowpass64(v, okz.gauss_taps(var, R))
        check(f"lowpass var={var}", okz.lowpass(a, w, var, R)[:, :w], ref, s, 2 * (1 + 3 * R))
    # ---- derivatives: fac1 * (ur + lr - ul - ll) + fac2 * (cr - cl): 3 additions, 1 subtraction, 2 products, 1 addition: k = 7
    f1, f2 = (float(x) for x in okz.deriv_factors())
    for step in (2, 4):
        lx, ly, det = okz.hessian(a, w, step)
        dx, dy, sx, sy = stencil64(v, step, f1, f2)
        check(f"Lx step={step}", lx[:, :w], dx, sx, 7)
        check(f"Ly step={step}", ly[:, :w], dy, sy, 7)
        # determinant dxx * dyy - dxy * dxy from the oracle's own Lx, Ly: three 7-operation stencils, 2 products, 1 subtraction: k = 24
        lx64, ly64 = lx[:, :w].astype(np.float64), ly[:, :w].astype(np.float64)
        dxx, dxy, sxx, sxy = stencil64(lx64, step, f1, f2)
        _, dyy, _, syy = stencil64(ly64, step, f1, f2)
        check(f"det step={step}", det[:, :w], dxx * dyy - dxy * dxy, sxx * syy + sxy * sxy, 24)
    # ---- PM_G2 conductivity g = 1 / (1 + ikc (dx^2 + dy^2)) with the un-normalised Scharr pair (10, 3): dx and dy 7 operations
    # each, 2 squares, 1 addition, the product with ikc, 1 + ., the division: k = 20.  With D = 1 + ikc (Sx^2 + Sy^2) >= den the
    # error of den is <= 18 u D and |dg| <= (error of den) / den^2 + u / den <= 19 u D / den^2: the "sum of terms" of g is D / den^2.
    # ikc itself is formed as the oracle forms it (float32) and enters as a constant.
    kc = vd.own_kcontrast(okz, a, w)[0]
    ikc = float(np.float32(1.0) / (np.float32(kc) * np.float32(kc)))
    xm, xp = reflect(w, 1)
    ym, yp = reflect(h, 1)
    r0, r1, r2 = v[ym], v, v[yp]
    ab = np.abs
    dx = 10 * (r1[:, xp] - r1[:, xm]) + 3 * (r0[:, xp] + r2[:, xp] - r0[:, xm] - r2[:, xm])
    dy = 10 * (r2 - r0) + 3 * (r2[:, xm] + r2[:, xp] - r0[:, xm] - r0[:, xp])
    sx = 10 * (ab(r1[:, xp]) + ab(r1[:, xm])) + 3 * (ab(r0[:, xp]) + ab(r2[:, xp]) + ab(r0[:, xm]) + ab(r2[:, xm]))
    sy = 10 * (ab(r2) + ab(r0)) + 3 * (ab(r2[:, xm]) + ab(r2[:, xp]) + ab(r0[:, xm]) + ab(r0[:, xp]))
    den = 1 + ikc * (dx * dx + dy * dy)
    g = okz.flow(a, w, 1, float(kc))
    check("flow PM_G2", g[:, :w], 1 / den, (1 + ikc * (sx * sx + sy * sy)) / (den * den), 20)
    # ---- one FED step fma(0.5 tau, sum of four (f + f') * (L' - L), L): 4 x (add, subtract, multiply) + 3 additions + the fma: k = 16
    tau = 0.19
    g64 = g[:, :w].astype(np.float64)
    sf = float(np.float32(0.5) * np.float32(tau))
    nb = [(r1[:, xp], g64[:, xp]), (r1[:, xm], g64[:, xm]), (r2, g64[yp]), (r0, g64[ym])]
    step = sum((g64 + gn) * (ln - v) for ln, gn in nb)
    ssum = sum((ab(g64) + ab(gn)) * (ab(ln) + ab(v)) for ln, gn in nb)
    check("nld step", okz.nld_steps(a, g, w, [tau])[:, :w], v + sf * step, ab(v) + abs(sf) * ssum, 16)


# ------------------------------------------------------------------------------------------------ the fuzz generator's content leg
def test_fuzz_content_leg_is_drawn_last():
    """float_content joins the case dictionary without moving any earlier field of a (seed, index): digests of the first cases of four
    seeds, taken before the field existed"""
    import fuzz_parity as fp

    def digest(seed, n, big):
        hsh = hashlib.sha256()
        for i in range(n):
            c = fp.draw_case(seed, i, big)
            c.pop("float_content")
            hsh.update(json.dumps(c, sort_keys=True, default=str).encode())
        return hsh.hexdigest()[:16]
    assert (digest(5, 200, 0), digest(21, 100, 0), digest(5, 100, 1), digest(9, 50, 2)) == \
        ("e7d1a757227347bb", "aeda2748dda0dfed", "ef96d95bdeeab180", "36db07d1c3a1f44e")
    drawn = [fp.draw_case(5, i)["float_content"] for i in range(400)]
    assert set(drawn) == {None, "hdr", "x255", "offset", "dark"} and 0.4 < drawn.count(None) / 400 < 0.7
    c = next(fp.draw_case(5, i) for i in range(400) if fp.draw_case(5, i)["float_content"] == "offset")
    assert "content=offset" in fp.describe(c)
