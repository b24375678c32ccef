"""CPU suite: RANSAC fundamental matrix (hak_find_fundamental).  The entry points are exported and refuse bad arguments without a
device, and the numpy statement of the contract (tests/fundamental_ref.py, the checker of the GPU tests) is held against
independent geometry: np.roots for its root finder, planted two-view scenes with a known F, the degenerate inputs, and the
project's golden pair."""
import os
import re
import subprocess

import numpy as np
import pytest

import fundamental_ref as fr
import homography_ref as hr
from conftest import GOLDEN


def golden_records():
    """the 2 464 accepted 1-NN matches of the golden left / right pair as (n, 4) float32 {x1, y1, x2, y2}"""
    p = np.load(os.path.join(GOLDEN, "left_right_oracle.npz"))["pts1"]
    p = p[p["match"] >= 0]
    return np.stack([p["x"], p["y"], p["match_x"], p["match_y"]], axis=1).astype(np.float32)


def _check_roots(c):
    """c = (c3, c2, c1, c0), arrays of one cubic each, against np.roots: the real-root count wherever np.roots' three roots are
    separated by more than 1e-6 (closer, it cannot tell a double root from a conjugate pair), and every root within 1e-9 relative
    of the nearest np.roots root (measured on the 1 000 random cubics when written: 6.8e-15 at worst).  Returns the number of
    counts compared."""
    roots, count, ok = fr.real_roots(*c)
    assert ok.all()
    compared = 0
    for k in range(len(c[0])):
        ref = np.roots([c[0][k], c[1][k], c[2][k], c[3][k]])
        if min(abs(a - b) for i, a in enumerate(ref) for b in ref[i + 1:]) > 1e-6:
            assert count[k] == int((ref.imag == 0.0).sum()), (k, count[k], ref)
            compared += 1
        assert count[k] in (1, 3)
        for r in roots[k, :count[k]]:
            near = ref[np.argmin(np.abs(ref - r))]
            assert abs(near - r) <= 1e-9 * abs(r), (k, r, ref)
    return compared


def test_root_finder_against_np_roots():
    rng = np.random.default_rng(7)
    c = rng.normal(size=(4, 1000))
    c[0] *= 10.0 ** rng.uniform(-3, 1, 1000)                            # leading coefficients over four decades
    assert _check_roots(tuple(c)) > 950
    # (a-1)(a-2)(a-3), (a-1)^2 (a+2), a^3 + a + 1
    named = np.array([[1.0, -6.0, 11.0, -6.0], [1.0, 0.0, -3.0, 2.0], [1.0, 0.0, 1.0, 1.0]]).T
    assert _check_roots(tuple(named)) == 2                              # (the double root's count is not np.roots' to judge)
    roots, count, ok = fr.real_roots(*named)
    assert count[0] == 3 and np.abs(roots[0] - [1.0, 2.0, 3.0]).max() <= 1e-12
    assert abs(roots[1, 0] + 2.0) <= 1e-12                              # q(1) = 0 exactly fails the sign test: the double root is skipped
    assert count[2] == 1 and abs(roots[2, 0] + 0.6823278038280193) <= 1e-12
    # a vanishing or non-finite leading coefficient, or a non-finite coefficient, is degenerate
    _, _, ok = fr.real_roots(np.array([0.0, np.nan, 1.0]), np.ones(3), np.ones(3), np.array([1.0, 1.0, np.inf]))
    assert not ok.any()


def test_null_space_and_cubic_are_what_they_claim():
    """A and B annihilate the 7 x 9 system, and the cubic's coefficients are det(a A + B) expanded"""
    rng = np.random.default_rng(11)
    M = rng.normal(size=(50, 7, 9))
    A, B, ok = fr.null_space([[M[:, r, q] for q in range(9)] for r in range(7)])
    assert ok.all()
    A, B = np.stack(A, axis=1), np.stack(B, axis=1)
    assert np.array_equal(A[:, 7:], np.tile([1.0, 0.0], (50, 1))) and np.array_equal(B[:, 7:], np.tile([0.0, 1.0], (50, 1)))
    for V in (A, B):
        res = np.abs(np.einsum("hrq,hq->hr", M, V)).max(axis=1)
        assert (res <= 1e-9 * np.abs(V).max(axis=1)).all()
    c3, c2, c1, c0 = fr.cubic(list(A.T), list(B.T))
    for a in (-1.5, 0.3, 2.0):
        want = np.linalg.det((a * A + B).reshape(-1, 3, 3))
        got = ((c3 * a + c2) * a + c1) * a + c0
        assert np.allclose(got, want, rtol=1e-9, atol=1e-9 * np.abs(want).max())


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_planted_scene(seed):
    """140 noise-free inliers of a known two-view geometry + 60 random records, 256 hypotheses, 1 px.  Measured when written,
    seeds 1..5: smallest / largest singular value of F 9e-16 .. 1.4e-14; largest float64 Sampson distance of a planted inlier
    under the returned F 1e-4 .. 5e-3 px."""
    from akaze_hip import synth
    recs, planted, Ft = synth.two_view_matches(140, 60, seed)
    assert planted.sum() == 140 and fr.sampson(Ft, recs[planted]).max() < 1e-3           # the scene is what it says
    r, mask = fr.find_fundamental(recs, 256, 1.0, seed)
    assert r["hypothesis"] >= 0 and 0 <= r["root"] <= 2 and r["n"] == 200
    assert mask[planted].all() and r["inliers"] >= 140 and r["inliers"] == mask.sum()
    F = r["F"].astype(np.float64).reshape(3, 3)
    assert np.abs(r["F"]).max() == np.float32(1.0)
    sv = np.linalg.svd(F, compute_uv=False)
    assert sv[2] <= 1e-5 * sv[0]
    # |x2^T F x1| of a planted inlier is what a Sampson distance below 1 px allows: |e| < 1 px * sqrt(a^2 + b^2 + p^2 + q^2)
    p = recs[planted].astype(np.float64)
    x1 = np.concatenate([p[:, :2], np.ones((140, 1))], axis=1)
    x2 = np.concatenate([p[:, 2:], np.ones((140, 1))], axis=1)
    l2, l1 = x1 @ F.T, x2 @ F
    e = np.abs((x2 * l2).sum(axis=1))
    assert (e < np.sqrt(l2[:, 0] ** 2 + l2[:, 1] ** 2 + l1[:, 0] ** 2 + l1[:, 1] ** 2)).all()
    # and it is the planted geometry: the true F explains the mask's inliers as the returned one does
    assert fr.sampson(Ft, recs[mask.astype(bool)]).max() < 5.0


def test_degenerate_inputs_give_no_model():
    rng = np.random.default_rng(5)
    for n in (0, 6):
        r, mask = fr.find_fundamental(rng.uniform(0, 1000, (n, 4)).astype(np.float32), 64)
        assert r["hypothesis"] == -1 and r["inliers"] == 0 and r["n"] == n and len(mask) == n and not mask.any()
        assert not r["F"].any()
    one = np.tile(np.array([[100.0, 200.0, 130.0, 210.0]], np.float32), (7, 1))
    r, mask = fr.find_fundamental(one, 64)
    assert r["hypothesis"] == -1 and not mask.any() and not r["F"].any()
    _, ok = fr.sample_indices(0, np.arange(64), 7)
    assert ok.any()                                                     # (samples were drawn: the normalisation refused them)
    lst = np.full((40, 4), np.nan, np.float32)
    lst[[1, 5, 11, 20, 33, 39]] = rng.uniform(0, 1000, (6, 4)).astype(np.float32)
    r, mask = fr.find_fundamental(lst, 256)
    assert r["hypothesis"] == -1 and not mask.any()
    # NaN / inf coordinates never count and never enter a usable sample
    from akaze_hip import synth
    recs, planted, _ = synth.two_view_matches(140, 60, 3)
    bad = np.zeros(200, bool)
    bad[::9] = True
    recs[bad, 1] = np.nan
    recs[4, 2] = np.inf
    bad[4] = True
    r, mask = fr.find_fundamental(recs, 256, 1.0, 3)
    assert r["hypothesis"] >= 0 and not mask[bad].any() and mask[planted & ~bad].all()


def test_sampler_is_a_function_of_seed_hypothesis_and_n():
    a, oka = fr.sample_indices(5, np.arange(1000), 2000)
    b, _ = fr.sample_indices(5, np.arange(500, 1000), 2000)
    assert np.array_equal(a[500:], b) and oka.all()
    assert ((a >= 0) & (a < 2000)).all() and all(len(set(row)) == 7 for row in a)
    _, ok7 = fr.sample_indices(0, np.arange(4096), 7)
    assert 0 < (~ok7).sum() < 4096                                      # n = 7: 32 draws do not always find all seven


GOLDEN_SEED, GOLDEN_INLIERS, GOLDEN_HOMOGRAPHY_INLIERS = 0, 1791, 1714


def test_golden_pair():
    """the statement on the golden pair's 2 464 accepted matches, 1024 hypotheses, 1 px, seed 0: 1 791 inliers (recorded when
    written) -- more than the 1 714 the homography's statement finds on the same list at 3 px, refit included"""
    recs = golden_records()
    assert len(recs) == 2464
    r, mask = fr.find_fundamental(recs, 1024, 1.0, GOLDEN_SEED)
    assert r["inliers"] == GOLDEN_INLIERS == mask.sum()
    h, _ = hr.find_homography(recs, 1024, 3.0, GOLDEN_SEED, True)
    assert h["inliers"] == GOLDEN_HOMOGRAPHY_INLIERS
    assert r["inliers"] > h["inliers"]


def test_entry_points_exported(ah):
    out = subprocess.check_output(["nm", "-D", "--defined-only", ah.LIB_PATH], text=True)
    exported = set(re.findall(r" T (hak_[a-z0-9_]+)", out))
    assert {"hak_find_fundamental", "hak_find_fundamental_batch"} <= exported
    assert ah.FUNDAMENTAL_DTYPE == fr.FUNDAMENTAL_DTYPE and ah.FUNDAMENTAL_DTYPE.itemsize == 52
    cxx = subprocess.check_output(["nm", "-D", "-C", "--defined-only", os.path.join(os.path.dirname(ah.LIB_PATH), "libakaze_hip.so")],
                                  text=True)
    assert "akaze::cuFindFundamental(" in cxx
    assert callable(ah.findFundamental)


def test_refusals_need_no_device(ah):
    """every refusal of include/hipakaze.h returns non-zero with a message before a device is touched"""
    rec = np.zeros((), ah.FUNDAMENTAL_DTYPE)
    buf = np.zeros(64, ah.MATCH_PAIR_DTYPE)                             # an address to stand for a list: it is never read
    lst, out = buf.ctypes.data, rec.ctypes.data
    lib = ah.lib
    single = [
        (None, None, 0, 0, 1.0, 0, None, out),                          # iterations 0
        (None, None, 0, 65537, 1.0, 0, None, out),
        (None, None, 0, 10, float("nan"), 0, None, out),
        (None, None, 0, 10, float("inf"), 0, None, out),
        (None, None, 0, 10, 0.0, 0, None, out),
        (None, None, 0, 10, -1.0, 0, None, out),
        (None, None, -1, 10, 1.0, 0, None, out),                        # negative n
        (None, None, 5, 10, 1.0, 0, None, out),                         # no list
        (None, None, 0, 10, 1.0, 0, None, None),                        # no h_out
    ]
    for args in single:
        assert lib.hak_find_fundamental(*args) != 0, args
        assert lib.hak_last_error().decode() != ""
    ctx_less = (None, lst, 8, lst, 1, 10, 1.0, 0, out, None)
    assert lib.hak_find_fundamental_batch(*ctx_less) != 0               # no context
    assert lib.hak_last_error().decode() != ""
    if ah.device_count() == 0:
        assert lib.hak_find_fundamental(None, None, 0, 10, 1.0, 0, None, out) != 0
        assert "no HIP device" in lib.hak_last_error().decode()


# ---- the committed cases of test_gpu_fundamental.py::test_randomised_parity: drawn here so that what they reach can be asserted
# on the statement alone
PARITY_SEED, PARITY_CASES = 2027, 150
PARITY_SCENES = ("general", "planar", "translation", "lattice", "collinear")


def parity_case(k):
    """case k of the randomised parity run: dict(recs (n, 4) float32, iterations, threshold, seed, ctx, scene, group).  A pure
    function of k.  Cases 8 b .. 8 b + 3 of every third block b of eight share iterations / threshold / seed and also go through
    hak_find_fundamental_batch as one ragged group (`group` = b, else -1)."""
    from akaze_hip import synth
    rng = np.random.default_rng([PARITY_SEED, k])
    pick = lambda seq: seq[int(rng.integers(len(seq)))]
    n = int(pick((rng.integers(0, 7), 7, 8, rng.integers(9, 301), rng.integers(9, 301), rng.integers(300, 3001))))
    scene = pick(PARITY_SCENES)
    m = max(n, 8)
    s = int(rng.integers(1 << 30))
    if scene == "general":
        recs = synth.two_view_matches(m, 0, s, noise=float(pick((0.0, 0.3, 1.0))))[0].astype(np.float64)
    else:
        x1 = np.stack([rng.uniform(0, 1920, m), rng.uniform(0, 1080, m)], axis=1)
        if scene == "collinear":                                        # every point of both images on one line each
            t = rng.uniform(0, 1, m)
            x1 = np.stack([100 + 1500 * t, 200 + 700 * t], axis=1)
            x2 = np.stack([300 + 1200 * t ** 1.1, 900 - 650 * t], axis=1)
        elif scene == "planar":                                         # one homography: F is not determined, many models tie
            H = np.array([[1.02, 0.03, 15.0], [-0.02, 0.97, -8.0], [2e-5, -1e-5, 1.0]]) + rng.normal(0, [[0.02, 0.02, 5], [0.02, 0.02, 5], [1e-5, 1e-5, 0]])
            p = np.concatenate([x1, np.ones((m, 1))], axis=1) @ H.T
            x2 = p[:, :2] / p[:, 2:]
        elif scene == "translation":                                    # pure translation: parallax along lines through one epipole
            ep = np.array([rng.uniform(-2000, 4000), rng.uniform(-2000, 3000)])
            x2 = x1 + (x1 - ep) * rng.uniform(0.02, 0.2, (m, 1))
        else:                                                           # lattice: few distinct integer values, ties in the counts
            q = int(pick((2, 3, 5)))
            x1 = np.stack([rng.integers(0, q, m), rng.integers(0, q, m)], axis=1) * float(pick((1, 7, 100)))
            x2 = np.stack([rng.integers(0, q, m), rng.integers(0, q + 1, m)], axis=1) * float(pick((1, 7, 100)))
        recs = np.concatenate([x1, x2], axis=1)
        if scene != "lattice":
            recs += rng.normal(0, float(pick((0.0, 0.0, 0.3))), recs.shape)
    rate = float(rng.uniform(0.0, 0.9)) if rng.random() < 0.7 else 0.0
    out = rng.random(m) < rate
    lo, hi = recs[np.isfinite(recs).all(axis=1)].min(), recs.max()
    recs[out] = np.floor(rng.uniform(lo, hi + 1, (int(out.sum()), 4))) if scene == "lattice" else rng.uniform(lo, hi + 1, (int(out.sum()), 4))
    if rng.random() < 0.3:
        recs += float(pick((-16000.0, 16000.0))) * np.array([rng.integers(0, 2), rng.integers(0, 2), rng.integers(0, 2), 1.0])
    recs = (recs * 2.0 ** int(pick((0, 0, 0, -20, -8, 8, 20)))).astype(np.float32)[:n]
    if n and rng.random() < 0.3:                                        # NaN / inf rows
        bad = rng.random(n) < 0.15
        recs[bad, rng.integers(0, 4, int(bad.sum()))] = np.array([np.nan, np.inf, -np.inf], np.float32)[rng.integers(0, 3, int(bad.sum()))]
    if n and rng.random() < 0.25:                                       # exact duplicates, up to all-equal
        share = float(pick((0.25, 0.6, 1.0)))
        recs[rng.random(n) < share] = recs[int(rng.integers(n))]
    c = dict(recs=recs, iterations=int(pick((1, 7, 64, 100, 257))), threshold=float(np.float32(rng.uniform(0.2, 8.0))),
             seed=int(pick((0, 0xFFFFFFFF, int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 2 ** 32))))), ctx=bool(rng.integers(2)),
             scene=scene, group=-1)
    if (k // 8) % 3 == 0 and k % 8 < 4:
        g = np.random.default_rng([PARITY_SEED, k // 8, 5])
        c.update(iterations=int((1, 7, 64, 100, 257)[int(g.integers(5))]), threshold=float(np.float32(g.uniform(0.2, 8.0))),
                 seed=int((0, 0xFFFFFFFF, int(g.integers(0, 2 ** 32)))[int(g.integers(3))]), group=k // 8)
    return c


def test_parity_cases_reach_the_rare_branches():
    """what the statement alone says about the committed cases: winners on a later root, lists without a model, ties between
    different (h, root) on the winning inlier count (the smallest-h-then-smallest-root rule decides), and winners whose cubic gave
    exactly one model (the one-root branch) and exactly three (fundamental_ref.models' `valid` row of the winning hypothesis: a
    three-root cubic with a rejected model counts as neither)"""
    assert parity_case(5)["recs"].tobytes() == parity_case(5)["recs"].tobytes() and parity_case(5)["seed"] == parity_case(5)["seed"]
    later_root = no_model = ties = one_root = three_roots = 0
    scenes = set()
    for k in range(PARITY_CASES):
        c = parity_case(k)
        scenes.add(c["scene"])
        r, mask = fr.find_fundamental(c["recs"], c["iterations"], c["threshold"], c["seed"])
        later_root += r["root"] > 0
        no_model += r["hypothesis"] < 0
        if r["hypothesis"] < 0:
            continue
        rec = hr.records(c["recs"])
        F, valid = fr.models(rec, c["seed"], np.arange(c["iterations"]))
        nroots = int(valid[r["hypothesis"]].sum())                       # the models the winner's cubic gave
        one_root += nroots == 1
        three_roots += nroots == 3
        hh, rr = np.nonzero(valid)
        t2 = np.float32(c["threshold"]) * np.float32(c["threshold"])
        cnt = fr.inlier_mask(F[hh, rr], rec, t2).sum(axis=1)
        assert cnt.max() == r["inliers"] and (hh[np.argmax(cnt)], rr[np.argmax(cnt)]) == (r["hypothesis"], r["root"])
        ties += (cnt == cnt.max()).sum() >= 2
    assert scenes == set(PARITY_SCENES)
    assert later_root >= 10 and no_model >= 10 and ties >= 10 and one_root >= 5 and three_roots >= 5, \
        (later_root, no_model, ties, one_root, three_roots)
