"""CPU suite of epipolar guided matching (hak_match_epipolar, include/hipakaze.h): the ABI, the argument checks that need no device,
and the numpy statement tests/epipolar_match_ref.py against a plain double loop and against a brute-force 2-NN statement.  Also
home of the fixture builder the GPU suite shares (tests/test_gpu_epipolar_match.py), with the properties that make it a test of
EPIPOLAR matching checked here, on the statement."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import epipolar_match_ref as er
from conftest import ROOT
from test_guided_match_cpu import SIZES, brute_knn2, flip_bits, random_points

# pure sideways translation: the line of (x, y) is y2 = y
F_XSHIFT = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], np.float32)


def scene_F():
    """the fundamental matrix of synth.two_view_matches' camera pair at 640 x 480, focal 500, largest |entry| 1, float32"""
    from akaze_hip import synth
    F = synth.two_view_matches(8, 0, 1, w=640, h=480, focal=500.0)[2].ravel()
    return (F / F[np.argmax(np.abs(F))]).astype(np.float32)


def on_line(rng, a, b, c, off):
    """a point of the 640 x 480 frame's span along the line a x + b y + c = 0 (float64), moved `off` px along the normal"""
    s = np.hypot(a, b)
    if abs(a) >= abs(b):
        y = rng.uniform(0, 480)
        x = -(b * y + c) / a
    else:
        x = rng.uniform(0, 640)
        y = -(a * x + c) / b
    return np.float32(x + off * a / s), np.float32(y + off * b / s)


def build_pair_epipolar(n1, n2, seed, dtype, F=None):
    """n1 queries in 640 x 480 and n2 train points under F (default: scene_F()):
      - about 60 % of the queries have a true partner: a random place on their line, up to 0.3 px off it, descriptor 5-40 bits away;
      - decoy (a): a train point inside the band (within 0.45 px of the line, anywhere along it) with a far (random) descriptor, or
        with one only slightly farther than the partner's (what the ratio test inside the band rejects);
      - decoy (b): a train point 60-200 px off the line whose descriptor is CLOSER than the partner's, by 1-4 bits: the plain 2-NN
        search takes it or fails its ratio test on it, the epipolar one must not see it;
      - about 10 % of the queries have no partner but a look-alike 60-200 px off their line (a moving object): the plain 2-NN search
        accepts it, the epipolar one must not;
      - about 5 % of the queries are rivals: a copy of an earlier query, a fraction of a pixel away, whose descriptor is closer to that
        query's partner -- the earlier query then fails the cross-check alone;
      - everything else: random points with random descriptors.  The train order is shuffled."""
    F = scene_F() if F is None else F
    rng = np.random.default_rng(seed)
    q = random_points(rng, n1, dtype)
    nrival = n1 // 20
    nbase = n1 - nrival
    train = []                                                   # (x, y, features)
    budget = n2
    la, lb, lc, _ = (v.astype(np.float64) for v in er.line(q, F))
    partner_of = {}
    order1 = rng.permutation(nbase)
    npart = int(0.6 * nbase)
    for i in order1[:npart]:
        if budget < 1:
            break
        nflip = int(rng.integers(5, 41))
        pf = flip_bits(rng, q["features"][i], nflip)
        pos = on_line(rng, la[i], lb[i], lc[i], rng.uniform(-0.3, 0.3))
        partner_of[int(i)] = (pos, pf)
        train.append((pos[0], pos[1], pf))
        budget -= 1
        kind = rng.random()
        if kind < 0.35 and budget >= 1:                          # decoy (a)
            far = rng.random() < 0.5
            f = rng.integers(0, 256, 61, dtype=np.uint8) if far else flip_bits(rng, pf, int(rng.integers(1, 6)))
            f[60] &= 0x3F
            train.append(on_line(rng, la[i], lb[i], lc[i], rng.uniform(-0.45, 0.45)) + (f,))
            budget -= 1
        elif kind < 0.6 and budget >= 1:                         # decoy (b)
            off = rng.uniform(60, 200) * rng.choice((-1.0, 1.0))
            f = flip_bits(rng, q["features"][i], max(nflip - int(rng.integers(1, 5)), 0))
            train.append(on_line(rng, la[i], lb[i], lc[i], off) + (f,))
            budget -= 1
    for i in order1[npart:npart + n1 // 10]:                     # look-alikes off the line of partnerless queries
        if budget < 1:
            break
        off = rng.uniform(60, 200) * rng.choice((-1.0, 1.0))
        train.append(on_line(rng, la[i], lb[i], lc[i], off) + (flip_bits(rng, q["features"][i], int(rng.integers(5, 41))),))
        budget -= 1
    partnered = sorted(partner_of)
    for k in range(nrival):                                      # rivals take the last slots of the query set
        i = nbase + k
        if not partnered:
            break
        src = partnered[int(rng.integers(0, len(partnered)))]
        q["x"][i] = q["x"][src] + np.float32(rng.uniform(-0.1, 0.1))
        q["y"][i] = q["y"][src] + np.float32(rng.uniform(-0.1, 0.1))
        q["features"][i] = flip_bits(rng, partner_of[src][1], int(rng.integers(0, 4)))
    t = random_points(rng, n2, dtype)
    order = rng.permutation(n2)
    for k, (x, y, f) in enumerate(train[:n2]):
        t["x"][order[k]], t["y"][order[k]], t["features"][order[k]] = x, y, f
    return q, t


# ---------------------------------------------------------------------------------------------- ABI
def test_header_declares_and_library_exports(ah):
    hdr = open(os.path.join(ROOT, "include", "hipakaze.h")).read()
    for name in ("hak_match_epipolar", "hak_match_epipolar_batch"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in ah.SYMBOLS
        assert getattr(ah.lib.product, name) is not None


def test_refusals_need_no_device(ah):
    lib = ah.lib
    buf = np.zeros(4 * 104, np.uint8)                            # never read: every call below is refused before a device is touched
    p = buf.ctypes.data
    cnt = C.c_int(-5)
    fp = C.POINTER(C.c_float)

    def call(n1=2, n2=2, F=F_XSHIFT, radius=2.0, num=4, den=5, p1=p, p2=p, count=cnt):
        f = None if F is None else np.ascontiguousarray(F, np.float32).ctypes.data_as(fp)
        return lib.hak_match_epipolar(None, p1, n1, p2, n2, f, radius, num, den, 1, 0, None, None, C.byref(count) if count is not None else None, None)

    for bad_radius in (0.0, -1.0, float("nan"), float("inf"), 3e19):      # 3e19 ** 2 overflows float32
        assert call(radius=bad_radius) != 0, bad_radius
        assert ah.lib.hak_last_error()
    for k in range(9):
        for v in (np.nan, np.inf, -np.inf):
            f = F_XSHIFT.copy()
            f[k] = v
            assert call(F=f) != 0, (k, v)
            assert ah.lib.hak_last_error()
    assert call(F=None) != 0 and b"F" in lib.hak_last_error()
    assert call(n1=-1) != 0 and call(n2=-1) != 0
    assert call(num=0) != 0 and call(den=0) != 0 and call(num=-4) != 0
    assert call(p1=None) != 0 and call(p2=None) != 0
    assert call(count=None) != 0
    # nothing to match is not an error, and needs no device either
    assert call(n1=0, p1=None) == 0 and cnt.value == 0
    assert lib.hak_match_epipolar_batch(None, p, p, 1, p, 2.0, 4, 5, 1, 0, p, p) != 0
    assert b"context" in lib.hak_last_error()


# ---------------------------------------------------------------------------------------------- the statement
def loop_statement(pts1, pts2, F, radius, ratio, cross_check, max_dist):
    """the rule of include/hipakaze.h as a plain double loop over float32 scalars"""
    f = np.float32
    F = [f(v) for v in np.asarray(F, np.float32).reshape(9)]
    r2 = f(radius) * f(radius)
    L, den_min = f(16384.0), f(2.0 ** -100)
    max_dist = 96 if max_dist <= 0 else max_dist
    n1, n2 = len(pts1), len(pts2)
    G = np.zeros((n1, n2), bool)
    D = np.zeros((n1, n2), np.int64)
    with np.errstate(all="ignore"):
        for i in range(n1):
            x, y = f(pts1["x"][i]), f(pts1["y"][i])
            a = f(f(f(F[0] * x) + f(F[1] * y)) + F[2])
            b = f(f(f(F[3] * x) + f(F[4] * y)) + F[5])
            c = f(f(f(F[6] * x) + f(F[7] * y)) + F[8])
            den = f(f(a * a) + f(b * b))
            qdom = bool(abs(x) <= L) and bool(abs(y) <= L) and bool(den >= den_min) and bool(np.isfinite(den))
            for j in range(n2):
                x2, y2 = f(pts2["x"][j]), f(pts2["y"][j])
                e = f(f(f(a * x2) + f(b * y2)) + c)
                G[i, j] = qdom and bool(abs(x2) <= L) and bool(abs(y2) <= L) and bool(f(e * e) < f(r2 * den))
                D[i, j] = sum(bin(int(u) ^ int(v)).count("1") for u, v in zip(pts1["features"][i], pts2["features"][j]))
    match = np.full(n1, -1, np.int64)
    pairs = []
    for i in range(n1):
        J = [j for j in range(n2) if G[i, j]]
        if not J:
            continue
        j1 = min(J, key=lambda j: (D[i, j], j))
        d1 = int(D[i, j1])
        d2 = min([int(D[i, j]) for j in J if j != j1], default=512)
        rev = min([k for k in range(n1) if G[k, j1]], key=lambda k: (D[k, j1], k))
        if d1 < max_dist and d1 * ratio[1] < d2 * ratio[0] and (not cross_check or rev == i):
            match[i] = j1
            pairs.append((i, j1, d1, d2))
    return match, pairs


@pytest.mark.parametrize("seed", range(6))
def test_statement_equals_double_loop(ah, seed):
    rng = np.random.default_rng(seed)
    n1, n2 = int(rng.integers(1, 41)), int(rng.integers(1, 41))
    F = scene_F()
    if seed == 4:                                                # forward motion, epipole (320, 240) inside the frame: F = [e]_x
        F = np.array([0, -1, 240, 1, 0, -320, -240, 320, 0], np.float32)
    if seed == 5:                                                # a = 0, b = -2^-50: den is exactly the floor 2^-100 (in the domain)
        F = F_XSHIFT * np.float32(2.0 ** -50)
    q, t = build_pair_epipolar(n1, n2, 50 + seed, ah.POINT_DTYPE, F=F)
    if seed == 1:                                                # non-finite and out-of-domain records on both sides
        q["x"][0], t["y"][0] = np.nan, np.inf
        if n1 > 2 and n2 > 2:
            q["y"][1], t["x"][1], q["x"][2], t["y"][2] = 16384.0, -16384.0, 16385.0, 20000.0
    if seed == 3:                                                # few prototypes: ties in both directions
        t["features"] = t["features"][np.arange(n2) % 3]
        q["features"] = q["features"][np.arange(n1) % 2]
    if seed == 4:
        q["x"][0], q["y"][0] = 320.0, 240.0                       # at the epipole: a = b = 0
    Fs = [F]
    if seed == 5:                                                # ... and one float32 step towards 0: den below the floor, no gate at all
        Fs.append(F.copy())
        Fs[1][5] = np.nextafter(F[5], np.float32(0))
        assert er.gate(q, t, Fs[0], 300.0).any() and not er.gate(q, t, Fs[1], 300.0).any()
    for F, (radius, ratio, cross, md) in ((F, c) for F in Fs for c in ((0.5, (4, 5), True, 0), (2.0, (1, 1), True, 40), (8.0, (4, 5), False, 0), (300.0, (1, 1), True, 0))):
        out, pairs, _ = er.match_epipolar(q, t, F, radius, ratio, cross, md)
        match, lp = loop_statement(q, t, F, radius, ratio, cross, md)
        assert np.array_equal(out["match"], match), (seed, radius)
        assert [(int(p["query"]), int(p["train"]), int(p["distance"]), int(p["second"])) for p in pairs] == lp
        acc = match >= 0
        assert np.array_equal(out["distance"][acc], [p[2] for p in lp]) and (out["distance"][~acc] == -1).all()
        assert np.array_equal(out["match_x"][acc].view(np.uint32), t["x"][match[acc]].view(np.uint32)) and (out["match_x"][~acc] == -1).all()
        assert np.array_equal(out["match_y"][acc].view(np.uint32), t["y"][match[acc]].view(np.uint32)) and (out["match_y"][~acc] == -1).all()
    if seed == 4:
        assert not er.gate(q, t, F, 1e4)[0].any()


@pytest.mark.parametrize("n1,n2", [(1, 1), (2, 1), (40, 37), (150, 200)])
def test_huge_radius_is_the_2nn_rule(ah, n1, n2):
    q, t = build_pair_epipolar(n1, n2, 9, ah.POINT_DTYPE)
    for F in (scene_F(), F_XSHIFT, np.arange(1, 10, dtype=np.float32) / 9):
        assert (er.line(q, F)[3] >= er.DEN_MIN).all()
        for ratio, cross, md in (((1, 1), True, 0), ((4, 5), True, 0), ((4, 5), False, 40)):
            out, _, _ = er.match_epipolar(q, t, F, 1e5, ratio, cross, md)
            assert np.array_equal(out["match"], brute_knn2(q, t, ratio, cross, md)), (ratio, cross, md)


def fixture_facts(q, t, radius):
    """what makes build_pair_epipolar a test of epipolar matching, measured on the statement at ratio 4/5 with the cross-check:
    how often each outcome occurs (why 0..4) and how many queries the band decides differently from the plain 2-NN rule"""
    d = er.hamming(q, t)
    out, _, why = er.match_epipolar(q, t, scene_F(), radius, (4, 5), True, 0, dist=d)
    plain = brute_knn2(q, t, (4, 5), True, 0)
    return dict(why=np.bincount(why, minlength=5), only_epipolar=int(((out["match"] >= 0) & (plain < 0)).sum()),
                only_plain=int(((out["match"] < 0) & (plain >= 0)).sum()))


@pytest.mark.parametrize("n1,n2", [s for s in SIZES if s[0] >= 300])
def test_fixture_separates_epipolar_from_plain_matching(ah, n1, n2):
    """the seeds the GPU suite uses (100 + n1).  At radius 2 acceptance and every rejection reason 1 to 4 occur (at radius 8 no band
    is empty at these densities; the other outcomes are asserted at every radius of the GPU suite), and at every radius some query
    is accepted under F and rejected by the plain 2-NN rule, and some query the other way round"""
    q, t = build_pair_epipolar(n1, n2, 100 + n1, ah.POINT_DTYPE)
    for radius in (0.5, 2.0, 8.0):
        s = fixture_facts(q, t, radius)
        print(n1, n2, radius, s)
        assert s["why"][0] >= n1 // 4 and (s["why"][[2, 3, 4]] > 0).all(), (radius, s)
        assert s["only_epipolar"] > 0 and s["only_plain"] > 0, (radius, s)
        assert radius != 2.0 or (s["why"] > 0).all(), s
