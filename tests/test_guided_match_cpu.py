"""CPU suite of guided matching (hak_match_guided, include/hipakaze.h): the ABI, the argument checks that need no device, and the
numpy statement tests/guided_match_ref.py against a plain double loop and against a brute-force 2-NN statement.  Also home of
the fixture builder the GPU suite shares (tests/test_gpu_guided_match.py), with the properties that make it a test of GUIDED
matching checked here, on the statement."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import guided_match_ref as gr
from conftest import ROOT

IDENTITY = np.eye(3, dtype=np.float32).ravel()
# a mild perspective map of a 640 x 480 frame
H_MILD = np.array([1.02, 0.03, 5.0, -0.02, 0.98, -3.0, 2e-5, -1e-5, 1.0], np.float32)
SIZES = [(0, 5), (5, 0), (1, 1), (2, 1), (63, 65), (64, 64), (65, 63), (300, 1000), (2000, 2000)]


def flip_bits(rng, feat, nbits):
    """a copy of the 61-byte descriptor with nbits distinct bits of its 486 flipped"""
    f = feat.copy()
    for b in rng.choice(486, size=nbits, replace=False):
        f[b >> 3] ^= np.uint8(1 << (b & 7))
    return f


def random_points(rng, n, dtype, w=640.0, h=480.0):
    p = np.zeros(n, dtype)
    p["x"] = rng.uniform(0, w, n).astype(np.float32)
    p["y"] = rng.uniform(0, h, n).astype(np.float32)
    p["features"] = rng.integers(0, 256, size=(n, 61), dtype=np.uint8)
    p["features"][:, 60] &= 0x3F
    p["_pad"] = 0xA5                                             # struct padding must not matter
    p["match"], p["distance"], p["match_x"], p["match_y"] = 7, 7, 7.0, 7.0
    return p


def build_pair(n1, n2, seed, dtype, H=H_MILD):
    """n1 queries in 640 x 480 and n2 train points under H:
      - about 60 % of the queries have a true partner: their projection plus sub-pixel noise, descriptor 5-40 bits away;
      - decoy (a): a train point inside the gate (within 0.45 px of the projection) with a far (random) descriptor, or with one only
        slightly farther than the partner's (what the ratio test inside the gate rejects);
      - decoy (b): a train point far outside the gate (60-200 px) whose descriptor is CLOSER than the partner's: the plain 2-NN
        search takes it, the guided one must not;
      - about 5 % of the queries are rivals: a copy of an earlier query, a fraction of a pixel away, whose descriptor is closer to that
        query's partner -- the earlier query then fails the cross-check alone;
      - everything else: random points with random descriptors.  The train order is shuffled."""
    rng = np.random.default_rng(seed)
    q = random_points(rng, n1, dtype)
    nrival = n1 // 20
    nbase = n1 - nrival
    train = []                                                   # (x, y, features)
    budget = n2
    px, py, _ = gr.project(q, H)
    partner_of = {}
    for i in rng.permutation(nbase)[:int(0.6 * nbase)]:
        if budget < 1:
            break
        pf = flip_bits(rng, q["features"][i], int(rng.integers(5, 41)))
        pos = (np.float32(px[i] + rng.uniform(-0.3, 0.3)), np.float32(py[i] + rng.uniform(-0.3, 0.3)))
        partner_of[int(i)] = (pos, pf)
        train.append((pos[0], pos[1], pf))
        budget -= 1
        kind = rng.random()
        if kind < 0.35 and budget >= 1:                          # decoy (a)
            a = rng.uniform(0, 2 * np.pi)
            r = rng.uniform(0.05, 0.45)
            far = rng.random() < 0.5
            f = rng.integers(0, 256, 61, dtype=np.uint8) if far else flip_bits(rng, pf, int(rng.integers(1, 6)))
            f[60] &= 0x3F
            train.append((np.float32(px[i] + r * np.cos(a)), np.float32(py[i] + r * np.sin(a)), f))
            budget -= 1
        elif kind < 0.6 and budget >= 1:                         # decoy (b)
            a = rng.uniform(0, 2 * np.pi)
            r = rng.uniform(60, 200)
            train.append((np.float32(px[i] + r * np.cos(a)), np.float32(py[i] + r * np.sin(a)), flip_bits(rng, q["features"][i], int(rng.integers(0, 4)))))
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


def brute_knn2(pts1, pts2, ratio, cross_check, max_dist):
    """the rule of hak_match_knn2 (include/hipakaze.h), written out: the match index of every query, -1 when rejected"""
    n1, n2 = len(pts1), len(pts2)
    max_dist = 96 if max_dist <= 0 else max_dist
    d = gr.hamming(pts1, pts2)
    match = np.full(n1, -1, np.int32)
    for i in range(n1):
        if n2 == 0:
            break
        j1 = int(np.argmin(d[i]))                                # first minimum
        d1 = int(d[i, j1])
        others = np.delete(d[i], j1)
        d2 = int(others.min()) if len(others) else 512
        ok = d1 < max_dist and d1 * ratio[1] < d2 * ratio[0]
        if ok and cross_check:
            ok = int(np.argmin(d[:, j1])) == i
        if ok:
            match[i] = j1
    return match


# ---------------------------------------------------------------------------------------------- ABI
def test_header_declares_and_library_exports(ah):
    hdr = open(os.path.join(ROOT, "include", "hipakaze.h")).read()
    for name in ("hak_match_guided", "hak_match_guided_batch"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in ah.SYMBOLS
        assert getattr(ah.lib.product, name) is not None


def test_refusals_need_no_device(ah):
    lib = ah.lib
    buf = np.zeros(4 * 104, np.uint8)                            # never read: every call below is refused before a device is touched
    p = buf.ctypes.data
    cnt = C.c_int(-5)
    fp = C.POINTER(C.c_float)

    def call(n1=2, n2=2, H=IDENTITY, radius=8.0, num=4, den=5, p1=p, p2=p, count=cnt):
        h = None if H is None else np.ascontiguousarray(H, np.float32).ctypes.data_as(fp)
        return lib.hak_match_guided(None, p1, n1, p2, n2, h, radius, num, den, 1, 0, None, None, C.byref(count) if count is not None else None, None)

    for bad_radius in (0.0, -1.0, float("nan"), float("inf"), 3e19):      # 3e19 ** 2 overflows float32
        assert call(radius=bad_radius) != 0, bad_radius
        assert ah.lib.hak_last_error()
    for k in range(9):
        for v in (np.nan, np.inf, -np.inf):
            h = IDENTITY.copy()
            h[k] = v
            assert call(H=h) != 0, (k, v)
    assert call(H=None) != 0
    assert call(n1=-1) != 0 and call(n2=-1) != 0
    assert call(num=0) != 0 and call(den=0) != 0 and call(num=-4) != 0
    assert call(p1=None) != 0 and call(p2=None) != 0
    assert call(count=None) != 0
    # nothing to match is not an error, and needs no device either
    assert call(n1=0, p1=None) == 0 and cnt.value == 0
    assert lib.hak_match_guided_batch(None, p, p, 1, p, 8.0, 4, 5, 1, 0, p, p) != 0
    assert b"context" in lib.hak_last_error()


# ---------------------------------------------------------------------------------------------- the statement
def loop_statement(pts1, pts2, H, radius, ratio, cross_check, max_dist):
    """the rule of include/hipakaze.h as a plain double loop over float32 scalars"""
    f = np.float32
    h = [f(v) for v in np.asarray(H, np.float32).reshape(9)]
    r2 = f(radius) * f(radius)
    max_dist = 96 if max_dist <= 0 else max_dist
    n1, n2 = len(pts1), len(pts2)
    G = np.zeros((n1, n2), bool)
    D = np.zeros((n1, n2), np.int64)
    with np.errstate(all="ignore"):
        for i in range(n1):
            x, y = f(pts1["x"][i]), f(pts1["y"][i])
            wz = f(f(f(h[6] * x) + f(h[7] * y)) + h[8])
            u = f(f(f(h[0] * x) + f(h[1] * y)) + h[2])
            v = f(f(f(h[3] * x) + f(h[4] * y)) + h[5])
            px, py = f(u / wz), f(v / wz)
            for j in range(n2):
                dx, dy = f(f(pts2["x"][j]) - px), f(f(pts2["y"][j]) - py)
                G[i, j] = bool(wz > 0) and bool(f(f(dx * dx) + f(dy * dy)) < r2)
                D[i, j] = sum(bin(int(a) ^ int(b)).count("1") for a, b in zip(pts1["features"][i], pts2["features"][j]))
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
    q, t = build_pair(n1, n2, 50 + seed, ah.POINT_DTYPE)
    if seed == 1:                                                # non-finite records on both sides
        q["x"][0], t["y"][0] = np.nan, np.inf
    H = H_MILD.copy()
    if seed == 2:                                                # wz <= 0 right of x = 320
        H[6], H[7] = np.float32(-1.0 / 320.0), 0.0
    if seed == 3:                                                # few prototypes: ties in both directions
        t["features"] = t["features"][np.arange(n2) % 3]
        q["features"] = q["features"][np.arange(n1) % 2]
    for radius, ratio, cross, md in ((0.5, (4, 5), True, 0), (3.0, (1, 1), True, 40), (20.0, (4, 5), False, 0), (300.0, (1, 1), True, 0)):
        out, pairs, _ = gr.match_guided(q, t, H, radius, ratio, cross, md)
        match, lp = loop_statement(q, t, H, radius, ratio, cross, md)
        assert np.array_equal(out["match"], match), (seed, radius)
        assert [(int(p["query"]), int(p["train"]), int(p["distance"]), int(p["second"])) for p in pairs] == lp
        acc = match >= 0
        assert np.array_equal(out["distance"][acc], [p[2] for p in lp]) and (out["distance"][~acc] == -1).all()
        assert np.array_equal(out["match_x"][acc].view(np.uint32), t["x"][match[acc]].view(np.uint32)) and (out["match_x"][~acc] == -1).all()
        assert np.array_equal(out["match_y"][acc].view(np.uint32), t["y"][match[acc]].view(np.uint32)) and (out["match_y"][~acc] == -1).all()


@pytest.mark.parametrize("n1,n2", [(1, 1), (2, 1), (40, 37), (150, 200)])
def test_identity_and_huge_radius_is_the_2nn_rule(ah, n1, n2):
    q, t = build_pair(n1, n2, 9, ah.POINT_DTYPE)
    for ratio, cross, md in (((1, 1), True, 0), ((4, 5), True, 0), ((4, 5), False, 40)):
        out, _, _ = gr.match_guided(q, t, IDENTITY, 1e5, ratio, cross, md)
        assert np.array_equal(out["match"], brute_knn2(q, t, ratio, cross, md)), (ratio, cross, md)


def fixture_shares(q, t, radius=3.0):
    """what makes build_pair a test of guided matching, measured on the statement at ratio 4/5 with the cross-check"""
    d = gr.hamming(q, t)
    out, _, why = gr.match_guided(q, t, H_MILD, radius, (4, 5), True, 0, dist=d)
    ungated = brute_knn2(q, t, (4, 5), True, 0)
    n = float(len(q))
    return dict(accepted=(why == 0).sum() / n, differs=(out["match"] != ungated).sum() / n, ratio=(why == 3).sum() / n,
                cross=(why == 4).sum() / n)


@pytest.mark.parametrize("n1,n2", [s for s in SIZES if s[0] >= 300])
def test_fixture_separates_guided_from_plain_matching(ah, n1, n2):
    """the seeds the GPU suite uses (100 + n1): enough accepted matches, enough queries whose match differs from the ungated rule's,
    enough rejections by the ratio test inside the gate and by the cross-check alone"""
    q, t = build_pair(n1, n2, 100 + n1, ah.POINT_DTYPE)
    s = fixture_shares(q, t)
    assert s["accepted"] >= 0.25 and s["differs"] >= 0.05 and s["ratio"] >= 0.05 and s["cross"] >= 0.01, s
