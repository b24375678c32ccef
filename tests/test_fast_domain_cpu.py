"""The inputs of the integer FAST stage-parity tests (tests/fast_domain.py) and the oracle on them, checked without a GPU: what keeps
tests/test_gpu_fast_stages.py from passing for the wrong reason.  numpy int64 restatements and the oracle only, never the kernels.

  * the generators are deterministic and hold what they claim
  * the wrapped int64 restatement of every integer stage (low-pass, decimation, contrast histogram, FED step, Hessian) equals the
    oracle's stage function on every generator and shape: the statement is pinned to a second, independent one
  * `u8_range`: no product or sum of any stage leaves int32 (the FED step for the step sizes below the stability limit: at tau = 41
    stepfac * step wraps on ANY content, which is why the case list has it)
  * `ramp_blown`: the Scharr sum of squares is exact at >= 5 % of the pixels, wrapped negative at >= 5 %, wrapped but non-negative
    at >= 1 %; the Hessian wraps at >= 1 % for every dilation; stepfac * step exceeds int32 at >= 1 % for tau = 41; the conductivity
    conversion saturates (PM_G1) and takes the NaN -> 0 branch (Charbonnier)
  * `full_range`: a histogram index grad * hfactor wraps below zero and is counted in bin 0
  * `signed`: `>> 16` and C's division by 65536 differ at >= 1 % of the low-pass outputs
  * micro-fixtures of three or four pixels per wrapped operation, derived by hand in the comments: they pin the stage functions to
    arithmetic, not to the oracle itself

On the Hessian: one would want the determinant product dxx * dyy - dxy * dxy itself to wrap on some input.  It cannot: every
second derivative is (fac1 * a + fac2 * b) >> 16 of a WRAPPED 32-bit sum, so |dxx|, |dyy|, |dxy| <= 2^15, dxx * dyy lies in
[-2^30, 2^30], dxy * dxy in [0, 2^30] and their difference in [-2^31, 2^30] -- inside int32 for every input.  The test below asserts
that bound on `full_range` and `ramp_blown`, and asks for the wraps where they do happen: in the products of the derivative stages.
"""
import numpy as np
import pytest

import fast_domain as fd

SEED = fd.SEED
INT_MIN, INT_MAX = fd.INT_MIN, fd.INT_MAX
SHAPES = fd.SHAPES


@pytest.fixture(scope="module", autouse=True)
def _quiet():
    with np.errstate(all="ignore"):
        yield


def plane(name, w, h):
    d = fd.GENERATORS[name](w, h, SEED)
    return d, fd.pitched(d)


# ------------------------------------------------------------------------------------------------ the generators
@pytest.mark.parametrize("name", list(fd.GENERATORS) + list(fd.U8_GENERATORS))
def test_generator_is_deterministic(name):
    g = fd.GENERATORS.get(name) or fd.U8_GENERATORS[name]
    a, b = g(260, 203, SEED), g(260, 203, SEED)
    assert a.dtype == (np.uint8 if name in fd.U8_GENERATORS else np.int32) and a.shape == (203, 260) and a.flags.c_contiguous
    assert a.tobytes() == b.tobytes()
    if name != "u8_flat255":
        assert g(260, 203, SEED + 1).tobytes() != a.tobytes()


@pytest.mark.parametrize("w,h", SHAPES)
def test_generators_hold_what_they_claim(w, h):
    u8 = fd.u8_range(w, h, SEED)
    assert u8.min() >= 0 and u8.max() <= 255 and len(np.unique(u8)) > 100
    assert np.array_equal(fd.u8_scene(w, h, SEED), u8)
    s = fd.signed(w, h, SEED)
    assert np.array_equal(s, u8 - 128) and (s < 0).mean() > 0.2 and (s > 0).mean() > 0.2
    amp = fd.ramp_amplitude(w)
    assert amp.min() == 64 and amp.max() == 2 ** 22
    r = fd.ramp_blown(w, h, SEED)
    assert np.array_equal(r.astype(np.int64), u8.astype(np.int64) * amp[None, :]) and r.max() > 2 ** 29
    f = fd.full_range(w, h, SEED)
    for edge in (f[0], f[h - 1], f[:, 0], f[:, w - 1]):
        assert {INT_MIN, INT_MAX, -1, 0} <= set(edge.tolist())
    if w > 256:
        assert set(f[h // 3: h // 3 + 4, 256].tolist()) == {INT_MIN, INT_MAX, -1, 0}
    assert (f < -2 ** 30).mean() > 0.2 and (f > 2 ** 30).mean() > 0.2
    b = fd.int_min_block(w, h, SEED)
    assert (b == INT_MIN).sum() == 16 and (b == INT_MAX).sum() == 16 and np.array_equal(b[(b != INT_MIN) & (b != INT_MAX)], s[(b != INT_MIN) & (b != INT_MAX)])
    c = fd.u8_checker(w, h, SEED)
    assert set(np.unique(c)) == {0, 255} and (c[:, 1:] != c[:, :-1]).all() and (c[1:] != c[:-1]).all()
    assert (fd.u8_flat255(w, h, SEED) == 255).all()


# ------------------------------------------------------------------------------------------------ restatement == oracle
@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("name", list(fd.GENERATORS))
def test_wrapped_restatement_equals_the_oracle(okz, name, w, h):
    d, a = plane(name, w, h)
    A = fd.Arith(True)
    for var, R in fd.LOWPASS:
        assert np.array_equal(fd.np_conv(A, d, okz.fast_gauss_taps(var, R), R), okz.fast_lowpass(a, w, var, R)[:, :w]), (var, R)
    dw, dh = w >> 1, h >> 1
    dst, sm = fd.np_down_smooth(A, d, okz.fast_gauss_taps(1.0, 2), dw, dh)
    odst, osm = okz.fast_down_smooth(a, w, dw, dh, (dw + 63) // 64 * 64)
    assert np.array_equal(dst, odst[:, :dw]) and np.array_equal(sm, osm[:, :dw])
    kc, hmax, hist, _ = fd.np_kcontrast(d, fd.PER)
    okc, ohmax, ohist = okz.fast_kcontrast(a, w, fd.PER)
    assert (kc, hmax) == (okc, ohmax) and np.array_equal(hist, ohist)
    g = okz.fast_flow(a, w, 1, fd.own_kcontrast(okz, a, w))
    for taus in fd.TAU_LISTS:
        cur = d.astype(np.int64)
        for t in taus:
            cur, _ = fd.np_nld_step(A, cur, g[:, :w], t)
        assert np.array_equal(cur, okz.fast_nld_steps(a, g, w, taus)[:, :w]), taus
    f1, f2 = okz.fast_deriv_factors()
    for step in fd.HESS_STEPS:
        lx, ly, det, _, _ = fd.np_hessian(A, d, step, f1, f2)
        olx, oly, odet = okz.fast_hessian(a, w, step)
        assert np.array_equal(lx, olx[:, :w]) and np.array_equal(ly, oly[:, :w]) and np.array_equal(det, odet[:, :w]), step


def test_the_u8_operators_equal_the_int_ones_on_the_same_values(okz):
    """fkz_conv_u8 is fkz_conv_int of the widened image (the restatement above covers the latter)"""
    for name in fd.U8_GENERATORS:
        for w, h in SHAPES:
            u8 = fd.pitched(fd.U8_GENERATORS[name](w, h, SEED))
            for var, R in fd.LOWPASS + [fd.BASE_UNFUSED]:
                assert np.array_equal(okz.fast_conv_u8(u8, w, u8.shape[1], var, R), okz.fast_lowpass(u8.astype(np.int32), w, var, R))


# ------------------------------------------------------------------------------------------------ conditions on the inputs
@pytest.mark.parametrize("w,h", SHAPES)
def test_u8_range_never_leaves_int32(okz, w, h):
    """the control: exact and wrapped arithmetic agree at every operation of every stage"""
    d, a = plane("u8_range", w, h)
    A = fd.Arith(False)                                                          # exact; counts what would not fit
    for var, R in fd.LOWPASS:
        assert np.array_equal(fd.np_conv(A, d, okz.fast_gauss_taps(var, R), R), okz.fast_lowpass(a, w, var, R)[:, :w])
    _, sm = fd.np_down_smooth(A, d, okz.fast_gauss_taps(1.0, 2), w >> 1, h >> 1)
    low = fd.np_conv(A, d, okz.fast_gauss_taps(1.0, 2), 2)
    for src in (d, low):
        _, _, ss = fd.np_scharr(A, src)
        assert ss.min() >= 0
        kc, hmax, hist, prod = fd.np_kcontrast(src, fd.PER)
        assert prod.max() <= INT_MAX and prod.min() >= 0
    g = okz.fast_flow(a, w, 1, fd.own_kcontrast(okz, a, w))
    for taus in fd.TAU_LISTS[:2]:                                                # (0.07; 0.1, 0.68, 0.08, 0.19)
        cur = d.astype(np.int64)
        for t in taus:
            cur, prod = fd.np_nld_step(A, cur, g[:, :w], t)
            assert np.abs(prod).max() <= INT_MAX, t
        assert np.array_equal(cur, okz.fast_nld_steps(a, g, w, taus)[:, :w])
    f1, f2 = okz.fast_deriv_factors()
    for step in fd.HESS_STEPS:
        _, _, det, _, _ = fd.np_hessian(A, low, step, f1, f2)
        assert np.array_equal(det, okz.fast_hessian(fd.pitched(low.astype(np.int32)), w, step)[2][:, :w])
    assert A.out_of_range == 0


@pytest.mark.parametrize("w,h", SHAPES)
def test_ramp_blown_sum_of_squares_is_exact_wrapped_negative_and_wrapped_positive(okz, w, h):
    d, a = plane("ramp_blown", w, h)
    _, _, exact = fd.np_scharr(fd.Arith(False), d)
    # (dx and dy themselves wrap too at the far end of the ramp; the sum of squares of fkz_flow is that of the WRAPPED differences)
    wdx, wdy, wrapped = fd.np_scharr(fd.Arith(True), d)
    true_sum = wdx * wdx + wdy * wdy
    assert (true_sum == wrapped).mean() >= 0.05
    assert ((true_sum != wrapped) & (wrapped < 0)).mean() >= 0.05
    assert ((true_sum != wrapped) & (wrapped >= 0)).mean() >= 0.01
    # ... and inside ONE 256-px strip all three occur
    strip = slice(0, min(w, 256))
    for sel in (true_sum == wrapped, (true_sum != wrapped) & (wrapped < 0), (true_sum != wrapped) & (wrapped >= 0)):
        assert sel[:, strip].mean() >= 0.01
    assert exact.max() > 2 ** 40


@pytest.mark.parametrize("w,h", SHAPES)
def test_ramp_blown_hessian_wraps_for_every_dilation(okz, w, h):
    f1, f2 = okz.fast_deriv_factors()
    for name in ("ramp_blown", "full_range"):
        d, a = plane(name, w, h)
        for step in fd.HESS_STEPS:
            A = fd.Arith(True)
            lx, ly, det, p1, p2 = fd.np_hessian(A, d, step, f1, f2)
            # the determinant itself cannot leave int32 (module docstring) ...
            assert np.abs(p1).max() <= 2 ** 30 and p2.min() >= 0 and p2.max() <= 2 ** 30
            assert (p1 - p2).min() >= INT_MIN and (p1 - p2).max() <= INT_MAX
            # ... the derivative stages that feed it do, on every dilation
            assert A.mask.mean() >= 0.01, (name, step, A.mask.mean())
            assert np.array_equal(det, okz.fast_hessian(a, w, step)[2][:, :w])


@pytest.mark.parametrize("w,h", SHAPES)
def test_stepfac_times_step_wraps_at_tau_41_and_not_at_tau_007(okz, w, h):
    assert fd.stepfac_of(41.0) == 1343488 and fd.stepfac_of(0.07) == 2294
    d, a = plane("ramp_blown", w, h)
    g = okz.fast_flow(a, w, 1, fd.own_kcontrast(okz, a, w))
    _, prod = fd.np_nld_step(fd.Arith(True), d, g[:, :w], 41.0)
    assert ((prod < INT_MIN) | (prod > INT_MAX)).mean() >= 0.01
    d, a = plane("u8_range", w, h)
    g = okz.fast_flow(a, w, 1, fd.own_kcontrast(okz, a, w))
    _, prod = fd.np_nld_step(fd.Arith(True), d, g[:, :w], 0.07)
    assert ((prod < INT_MIN) | (prod > INT_MAX)).sum() == 0


@pytest.mark.parametrize("w,h", SHAPES)
def test_ramp_blown_conductivity_saturates_and_converts_nan(okz, w, h):
    """decided from the float value the oracle converts: dif2 = (float)wrapped sum * ikc, contrast factor 1 (ikc = 1)"""
    d, a = plane("ramp_blown", w, h)
    _, _, ss = fd.np_scharr(fd.Arith(True), d)
    dif2 = ss.astype(np.float32) * np.float32(1.0)
    # PM_G1: g = exp(-dif2); g * 65536 + 0.5 >= 2^31 from -dif2 >= ln(2^15) = 10.4 on, far from it: -dif2 > 100 -> exp = inf
    sat = dif2 < -100
    # Charbonnier: g = 1 / sqrt(1 + dif2) is NaN for 1 + dif2 < 0
    nan = (np.float32(1.0) + dif2) < 0
    assert sat.sum() >= 1 and nan.sum() >= 1
    assert (okz.fast_flow(a, w, 0, 1)[:, :w][sat] == INT_MAX).all()
    assert (okz.fast_flow(a, w, 3, 1)[:, :w][nan] == 0).all()
    # a zero contrast factor (a flat image's): ikc = inf, dif2 = 0 * inf = NaN where the gradient vanishes -> every conductivity converts to 0
    flat = ss == 0
    if flat.any():
        for diff in (0, 1, 2, 3):
            assert (okz.fast_flow(a, w, diff, 0)[:, :w][flat] == 0).all(), diff


@pytest.mark.parametrize("w,h", SHAPES)
def test_full_range_histogram_index_wraps_negative_into_bin_0(okz, w, h):
    d, a = plane("full_range", w, h)
    kc, hmax, hist, prod = fd.np_kcontrast(d, fd.PER)
    wrapped = fd.wrap32(prod)
    neg = (wrapped != prod) & (wrapped < 0)
    assert neg.sum() >= 1 and hmax < 400
    okc, ohmax, ohist = okz.fast_kcontrast(a, w, fd.PER)
    assert (okc, ohmax) == (kc, hmax) and np.array_equal(ohist, hist)
    # bin 0 holds them: without the clamp's lower end the same histogram has exactly that many entries fewer there
    hi = wrapped >> 16
    extra0 = ((w + 31) // 32 * 32 - w) * h + ((h + 15) // 16 * 16 - h) * w
    assert int(ohist[0]) == int((hi <= 0).sum()) + extra0 and int((hi < 0).sum()) >= int(neg.sum())


@pytest.mark.parametrize("w,h", SHAPES)
def test_signed_floor_and_truncation_differ(okz, w, h):
    d, a = plane("signed", w, h)
    sums = []
    out = fd.np_conv(fd.Arith(True), d, okz.fast_gauss_taps(1.0, 2), 2, sums)
    col = sums[1]                                                               # the column pass's sums, from the floor-shifted rows
    trunc = np.where(col < 0, -((-col) >> 16), col >> 16)                       # C's col / 65536
    assert np.array_equal(col >> 16, out)
    assert (trunc != out).mean() >= 0.01
    assert np.array_equal(out, okz.fast_lowpass(a, w, 1.0, 2)[:, :w])


# ------------------------------------------------------------------------------------------------ micro-fixtures, derived by hand
def test_micro_negative_shift(okz):
    """One pixel of -1 in a 9 x 9 plane of zeros, sigma = 1 low-pass (radius 2).  Every tap k_i lies in (0, 65536), so a row-pass product
    k_i * (-1) = -k_i and -k_i >> 16 = floor(-k_i / 65536) = -1 (truncation would give 0): row 4 becomes -1 at columns 2..6.  The column
    pass sees that row at distance 0, 1 or 2 from rows 2..6 and computes k_j * (-1) >> 16 = -1 again: a 5 x 5 block of -1 around the
    pixel, zero elsewhere (no tap of rows 0, 1, 7, 8 reaches row 4: their mirrored taps read rows 0..3 and 5..8).  With C division the
    whole result would be zero."""
    k = okz.fast_gauss_taps(1.0, 2)
    assert all(0 < int(v) < 65536 for v in k)
    a = np.zeros((9, 64), np.int32)
    a[4, 4] = -1
    want = np.zeros((9, 9), np.int32)
    want[2:7, 2:7] = -1
    assert np.array_equal(okz.fast_lowpass(a, 9, 1.0, 2)[:, :9], want)


def test_micro_nld_step_with_a_wrapping_stepfac_product(okz):
    """3 x 3 plane, L = 0 except L(1, 2) = 2000, conductivity 32768 (g = 0.5) everywhere, tau = 41: stepfac = (int)(0.5 * 41 * 65536 +
    0.5) = 1 343 488.  Every pair sum of conductivities is 65536, so a term is 65536 * dL and `>> 16` gives dL back.
      centre (1, 1): E = 2000, W = S = N = 0 -> step = 2000; stepfac * step = 2 686 976 000 >= 2^31, wrapped: - 4 294 967 296 =
                     -1 607 991 296 = -24536 * 65536 -> L' = -24536 + 0            (the 64-bit product would give 41000)
      (1, 2):        E and W both mirror onto (1, 1): 2 * (0 - 2000); N, S = (0 - 2000) each -> step = -8000; stepfac * step =
                     -10 747 904 000, + 3 * 2^32 = 2 136 997 888 = 32608 * 65536 -> L' = 32608 + 2000 = 34608
      (0, 2), (2, 2): N and S both read (1, 2): 2 * 2000, E = W = 0 -> step = 4000; 5 373 952 000 - 2^32 = 1 078 984 704 =
                     16464 * 65536 -> L' = 16464
      everything else: all four differences are 0 -> L' = 0"""
    s = np.zeros((3, 64), np.int32)
    s[1, 2] = 2000
    f = np.zeros((3, 64), np.int32)
    f[:, :3] = 32768
    want = np.array([[0, 0, 16464], [0, -24536, 34608], [0, 0, 16464]], np.int32)
    assert np.array_equal(okz.fast_nld_steps(s, f, 3, [41.0])[:, :3], want)


def test_micro_flow_with_a_negative_sum_of_squares(okz):
    """3 x 3 plane [[0, 0, 2], [0, 0, 4633], [0, 0, 2]], centre pixel: dx = 10 * (4633 - 0) + 3 * (2 + 2 - 0 - 0) = 46342, dy = 10 * 0 +
    3 * (0 + 2 - 0 - 2) = 0; dx * dx = 2 147 580 964 >= 2^31, wrapped: -2 147 386 332; as a float (spacing 128 up there) -2 147 386 368.
      contrast factor 1 (ikc = 1, dif2 = -2.1e9):
        PM_G1        g = exp(+2.1e9) = inf                          -> INT_MAX     (unwrapped: exp(-2.1e9) = 0 -> 0)
        PM_G2        g = 1 / (1 - 2.1e9) = -4.7e-10, * 65536 + 0.5 = 0.49997 -> 0
        Weickert     dif2^4 = 2.1e37 (finite), exp(-3.315 / 2.1e37) = 1, g = 0 -> 0 (the square loses the sign)
        Charbonnier  g = 1 / sqrt(1 - 2.1e9) = NaN                  -> 0           (unwrapped: 1 / sqrt(2.1e9) * 65536 + 0.5 = 1.9 -> 1)
      contrast factor 46340 (kc * kc = 2 147 395 600, dif2 = -0.999996, 1 + dif2 = 4e-6 with an error below 2e-7):
        PM_G2        g = 1 / 4e-6 = 2.3e5 >= 32768, so g * 65536 >= 2^31 -> INT_MAX     (unwrapped: dif2 = +1.00009, g = 0.49998 -> 32767)"""
    a = np.zeros((3, 64), np.int32)
    a[0, 2], a[1, 2], a[2, 2] = 2, 4633, 2
    dx, dy, ss = fd.np_scharr(fd.Arith(True), a[:, :3])
    assert (dx[1, 1], dy[1, 1], ss[1, 1]) == (46342, 0, -2147386332) and np.float32(ss[1, 1]) == np.float32(-2147386368.0)
    for diff, want in ((0, INT_MAX), (1, 0), (2, 0), (3, 0)):
        assert okz.fast_flow(a, 3, diff, 1)[1, 1] == want, diff
    assert okz.fast_flow(a, 3, 1, 46340)[1, 1] == INT_MAX
