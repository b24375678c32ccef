"""CPU suite: five-point RANSAC essential matrix (hak_find_essential).  The numpy statement of the contract (tests/essential_ref.py,
the checker of the GPU tests) is held against planted scenes: the family table of the five-point solver (R = I, planar, small and
large rotations), the 42 noise-free poses of the pose table through find_essential -> recover_pose beside the seven-point path, the
nine noisy scenes of the README and a planar family through both chains, and the committed randomised cases of the GPU parity run,
of which it is asserted on the statement alone what they reach; the entry points are exported and refuse bad arguments without a
device."""
import os
import re
import subprocess

import numpy as np
import pytest

import essential_ref as er
import fundamental_ref as fr
import fundamental_refit_ref as rr
import homography_ref as hr
import pose_ref as pr
import pose_refit_ref as pz
from conftest import ROOT
from test_pose_cpu import TABLE, dir_angle, rot_angle, table_case
from test_pose_refit_cpu import MAX_DEPTH, SCENES

FAMILIES = ("R = I, sideways t", "R = I, t = (1, 2, 0)", "R = I, forward t", "planar, R = I, sideways t", "planar, general", "general",
            "small rotation", "170 degree roll")
FAMILY_SAMPLES, FAMILY_GATE = 200, 0.95


@pytest.fixture(scope="module")
def synth(ah):
    from akaze_hip import synth
    return synth


def _skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0.0]])


def family_samples(synth, name, seed, count=FAMILY_SAMPLES):
    """count noise-free five-point samples of a family in float64 bearings: (points (count, 5, 4), E (count, 9) scaled to largest
    |entry| 1)"""
    rng = np.random.default_rng([77, seed])
    P, Es = np.zeros((count, 5, 4)), np.zeros((count, 9))
    for s in range(count):
        while True:
            if name in ("general", "planar, general"):
                R, t = synth.rotation_zyx(rng.uniform(-20, 20, 3)), rng.normal(size=3)
            elif name == "small rotation":
                R, t = synth.rotation_zyx(rng.uniform(-0.5, 0.5, 3)), rng.normal(size=3)
            elif name == "170 degree roll":
                R, t = synth.rotation_zyx((rng.uniform(-3, 3), rng.uniform(-3, 3), 170 + rng.uniform(-3, 3))), rng.normal(size=3)
            else:
                R = np.eye(3)
                t = np.array({"R = I, t = (1, 2, 0)": (1.0, 2.0, 0.0), "R = I, forward t": (0.0, 0.0, 1.0)}.get(name, (1.0, 0.0, 0.0)))
            t = t / np.linalg.norm(t)
            X = np.stack([rng.uniform(-2, 2, 5), rng.uniform(-2, 2, 5), rng.uniform(4, 10, 5)], axis=1)
            if name.startswith("planar"):
                nrm = rng.normal(size=3) * 0.3 + np.array([0, 0, 1.0])
                X[:, 2] = (6.0 - X[:, 0] * nrm[0] - X[:, 1] * nrm[1]) / nrm[2]
            X2 = X @ R.T + t
            if (X[:, 2] > 0.5).all() and (X2[:, 2] > 0.5).all():
                break
        P[s, :, 0:2], P[s, :, 2:4] = X[:, :2] / X[:, 2:], X2[:, :2] / X2[:, 2:]
        E = _skew(t) @ R
        Es[s] = (E / E.flat[np.argmax(np.abs(E))]).reshape(9)
    return P, Es


def planted_error(F, valid, Es):
    """per sample the smallest max-abs entry error of a valid model against the planted E, up to sign"""
    F64 = F.astype(np.float64)
    err = np.minimum(np.abs(F64 - Es[:, None, :]).max(axis=2), np.abs(F64 + Es[:, None, :]).max(axis=2))
    return np.where(valid, err, np.inf).min(axis=1)


def test_family_table(synth):
    """the planted E is among the statement's models to 1e-6 in at least 95 % of the noise-free samples of every family"""
    print("| scene family | planted E found to 1e-6 | to 1e-3 | real roots 2 / 4 / 6 / 8 / 10 |")
    shares = []
    for k, name in enumerate(FAMILIES):
        P, Es = family_samples(synth, name, k)
        F, valid = er.solve_five(P)
        e = planted_error(F, valid, Es)
        nv = np.bincount(valid.sum(axis=1), minlength=11)
        shares.append(float((e < 1e-6).mean()))
        print(f"| {name} | {100 * shares[-1]:.1f} % | {100 * (e < 1e-3).mean():.1f} % | {' / '.join(str(int(v)) for v in nv[2::2])} |")
    assert all(s >= FAMILY_GATE for s in shares), dict(zip(FAMILIES, shares))


def test_statement_is_pure_and_scaled(synth):
    recs, _, F, K, R, t, z = synth.two_view_scene(210, 90, 5, noise=0.3)
    keep = recs.copy()
    a = er.find_essential(recs, K, None, 64, 1.0, 3)
    b = er.find_essential(recs, (K[0, 0], K[1, 1], K[0, 2], K[1, 2]), K, 64, 1.0, 3, block=7)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and recs.tobytes() == keep.tobytes()
    rec, mask = a
    assert rec["hypothesis"] >= 0 and 16 <= rec["root"] <= 25 and rec["n"] == 300 and rec["inliers"] == mask.sum() >= 150
    assert np.abs(rec["F"]).max() == 1.0 and mask.dtype == np.uint8
    # E = K2^T F K1 has two equal singular values and a zero one
    s = np.linalg.svd(K.T @ rec["F"].astype(np.float64).reshape(3, 3) @ K, compute_uv=False)
    assert abs(s[0] - s[1]) <= 1e-5 * s[0] and s[2] <= 1e-5 * s[0]
    # fewer than five records, and none at all
    for n in (0, 4):
        r, m = er.find_essential(recs[:n], K, None, 16, 1.0, 0)
        assert r["hypothesis"] == -1 and r["inliers"] == 0 and r["root"] == 0 and r["n"] == n and not r["F"].any() and len(m) == n


def test_planted_poses_through_the_statements(synth):
    """find_essential -> recover_pose on the 42 noise-free poses from float32 matches, beside find_fundamental -> recover_pose on the
    same matches, gated PER POSE: rotation and baseline error within 10 x the seven-point path's on that pose, with a floor under
    the seven-point figure: the seven-point path's own median error over the table.

    Why the floor.  Every match of a pose is an inlier of every hypothesis at 1 px, so hypothesis 0 wins the tie on both paths and
    each error is the float32 rounding of the matches (up to 6e-5 px) times the conditioning of ONE minimal sample.  The seven-point
    path's own error spreads over ten orders of magnitude across the table for that reason alone (4.4e-14 degrees on pose 4, where
    the rounding happens to vanish, 1.5e-3 on pose 24), so far below its typical error the ratio on one pose compares two samples'
    luck, not two solvers.  The floor is taken from the reference (its median here: 2.5e-5 / 1.1e-4 degrees), never from the
    five-point figures.  Measured when written: without the floor two poses miss 10 x -- pose 41 with 1.80e-4 / 8.40e-4 against
    9.71e-6 / 5.18e-5 degrees (18.6 x / 16.2 x), pose 4 with 5.97e-13 against 4.68e-14 degrees of baseline (12.8 x) -- and the other
    40 stay below 7.6 x; the five-point medians are 1.7e-5 / 5.9e-5 degrees, below the seven-point ones.  Every figure is printed."""
    errs = {"E": [], "F": []}
    for k in range(len(TABLE)):
        recs, _, K, R, t, z = table_case(synth, k)
        for name, rec in (("E", er.find_essential(recs, K, None, 16, 1.0, k)[0]), ("F", fr.find_fundamental(recs, 16, 1.0, k)[0])):
            assert rec["hypothesis"] >= 0 and rec["inliers"] == len(recs), (name, k, rec)
            out = pr.recover_pose(recs, rec, K)[0]
            assert out["candidate"] >= 0 and out["in_front"] == len(recs), (name, k, out)
            errs[name].append((rot_angle(out["R"].reshape(3, 3), R), dir_angle(out["t"], t)))
    E, F = np.array(errs["E"]), np.array(errs["F"])
    floor = np.median(F, axis=0)
    for k in range(len(TABLE)):
        print(f"pose {k}: five-point {E[k, 0]:.2e} / {E[k, 1]:.2e} degrees, seven-point {F[k, 0]:.2e} / {F[k, 1]:.2e}")
    print(f"42 planted poses, rotation / baseline error in degrees: five-point worst {E[:, 0].max():.3e} / {E[:, 1].max():.3e}, median "
          f"{np.median(E[:, 0]):.3e} / {np.median(E[:, 1]):.3e}; seven-point worst {F[:, 0].max():.3e} / {F[:, 1].max():.3e}, median "
          f"{floor[0]:.3e} / {floor[1]:.3e}")
    bad = [(k, E[k].tolist(), F[k].tolist()) for k in range(len(TABLE)) if (E[k] > 10 * np.maximum(F[k], floor)).any()]
    assert not bad, bad
    assert (E.max(axis=0) <= 10 * F.max(axis=0)).all()


def _chains(recs, K, R, t, seed):
    """(errors and counts) of essential -> pose (-> pose refit) beside fundamental -> refit -> pose (-> pose refit), 256 x 1 px"""
    rows = []
    e0 = er.find_essential(recs, K, None, 256, 1.0, seed)[0]
    f0 = rr.refine_fundamental(recs, fr.find_fundamental(recs, 256, 1.0, seed)[0], 1.0, 3)[0]
    for rec in (e0, f0):
        pose = pr.recover_pose(recs, rec, K, None, 1.0, MAX_DEPTH)[0]
        ref = pz.refine_pose(recs, K, pose, None, 2.0, MAX_DEPTH, 8)[0]
        rows.append((int(rec["inliers"]), rot_angle(pose["R"].reshape(3, 3), R), dir_angle(pose["t"], t), int(pose["in_front"]),
                     rot_angle(ref["R"].reshape(3, 3), R), dir_angle(ref["t"], t), int(ref["in_front"])))
    return rows


def _row(label, rows, planted):
    cell = lambda r: f"{r[0]} | {r[1]:.3f} / {r[2]:.3f} ({r[3]}) | {r[4]:.3f} / {r[5]:.3f} ({r[6]})"
    return f"| {label} | {cell(rows[0])} | {cell(rows[1])} | {planted} |"


# (n, noise px, seed), 70 % planted: nine in ten of them on one slanted plane, the others at depths 4..12.  On an EXACTLY planar
# scene two essential matrices fit every point (the twin of the plane's homography decomposition) and an inlier count cannot tell
# them apart: the winner is then whichever comes first, and in_front / inliers is the caller's signal, as it is for F.
PLANAR = [(300, 0.3, 21), (300, 1.0, 22), (1000, 0.5, 23), (400, 0.0, 24)]
OFF_PLANE = 0.1


def planar_scene(synth, n, noise, seed):
    """a dominant plane under the default pose of two_view_scene: points of one slanted plane seen by both cameras, one planted
    point in ten off it, 30 % outliers"""
    rng = np.random.default_rng([91, seed])
    w, h, focal = 1920, 1080, 1500.0
    K = np.array([[focal, 0.0, w / 2.0], [0.0, focal, h / 2.0], [0.0, 0.0, 1.0]])
    R, t = synth.rotation_zyx((2.0, -5.0, 1.5)), np.array([-1.0, 0.05, 0.1])
    n_in = n * 7 // 10
    nrm, d = np.array([0.15, -0.1, 1.0]), 8.0
    p1 = np.zeros((0, 2))
    p2 = np.zeros((0, 2))
    while len(p1) < n_in:
        px = np.stack([rng.uniform(0, w, 2 * n_in), rng.uniform(0, h, 2 * n_in), np.ones(2 * n_in)], axis=1)
        ray = np.linalg.solve(K, px.T).T
        X = ray * (d / (ray @ nrm))[:, None]
        off = rng.random(len(X)) < OFF_PLANE
        X[off] = ray[off] * rng.uniform(4.0, 12.0, (int(off.sum()), 1))
        X2 = X @ R.T + t
        q = X2 @ K.T
        q = q[:, :2] / q[:, 2:]
        keep = (X[:, 2] > 0.5) & (X2[:, 2] > 0.5) & (q[:, 0] >= 0) & (q[:, 0] < w) & (q[:, 1] >= 0) & (q[:, 1] < h)
        p1, p2 = np.concatenate([p1, px[keep, :2]]), np.concatenate([p2, q[keep]])
    p1, p2 = p1[:n_in] + rng.normal(0, noise, (n_in, 2)), p2[:n_in] + rng.normal(0, noise, (n_in, 2))
    o = np.stack([rng.uniform(0, w, n - n_in), rng.uniform(0, h, n - n_in), rng.uniform(0, w, n - n_in), rng.uniform(0, h, n - n_in)], axis=1)
    recs = np.concatenate([np.concatenate([p1, p2], axis=1), o]).astype(np.float32)
    return recs[rng.permutation(n)], K, R, t / np.linalg.norm(t), n_in


def test_noisy_and_planar_scenes_beside_the_seven_point_chain(synth):
    """printed for the README, not gated, except that on the planar scenes the five-point winner's pose has at least 0.9 of its
    inliers in front"""
    print("| n, noise px, seed | five-point: inliers | pose (in front) | pose refit 2 px, 8 rounds | seven-point + refit: inliers | pose "
          "(in front) | pose refit | planted |")
    for n, noise, seed in SCENES:
        recs, flags, F, K, R, t, z = synth.two_view_scene(n * 7 // 10, n - n * 7 // 10, seed, noise=noise)
        print(_row(f"{n}, {noise}, {seed}", _chains(recs, K, R, t, seed), int(flags.sum())))
    for n, noise, seed in PLANAR:
        recs, K, R, t, n_in = planar_scene(synth, n, noise, seed)
        rows = _chains(recs, K, R, t, seed)
        print(_row(f"dominant plane {n}, {noise}, {seed}", rows, n_in))
        assert rows[0][3] >= 0.9 * rows[0][0], (n, noise, seed, rows[0])


# ---- the committed cases of test_gpu_essential.py::test_randomised_parity: drawn here so that what they reach can be asserted on
# the statement alone
PARITY_SEED, PARITY_CASES = 2031, 98
PARITY_SCENES = ("general", "planar", "sideways", "forward", "lattice", "collinear", "equal")


# two built members at the end of the family: a five-point sample whose polynomial has ten real roots (found by a search over 3e5
# random samples; about one in 1e5 has ten) plus three records that fit root 8 / root 9 alone, at a seed whose only hypothesis draws
# the five -- the one way a winner reaches the third virtual hypothesis of the scratch
_TEN = [[38.72488021850586, 0.7093283534049988, 301.7791442871094, 1094.1685791015625],
        [566.2244262695312, 380.4366149902344, -82.31266784667969, 1084.935546875],
        [522.032470703125, -49.563541412353516, 926.820068359375, 875.431640625],
        [905.84423828125, 603.7275390625, 289.17962646484375, 691.4124145507812],
        [544.9818725585938, 851.4674072265625, 388.89300537109375, 135.8022918701172]]
_TEN_EXTRA = {8: [[823.3292236328125, 645.4382934570312, 556.7413330078125, 307.1564636230469],
                  [615.9743041992188, 209.01068115234375, 477.6462707519531, 889.5046997070312],
                  [328.64569091796875, 403.0225524902344, 506.85321044921875, 144.72357177734375]],
              9: [[285.2052917480469, 272.4914855957031, 167.42333984375, 900.9522705078125],
                  [696.3502197265625, 604.0704345703125, 198.22735595703125, 668.32421875],
                  [429.13580322265625, 110.55984497070312, 468.9504699707031, 955.369873046875]]}


def parity_case(k):
    if k >= PARITY_CASES - 2:
        K = (1000.0, 1000.0, 500.0, 500.0)
        return dict(recs=np.array(_TEN + _TEN_EXTRA[8 + k - (PARITY_CASES - 2)], np.float32), K1=K, K2=K, iterations=1, threshold=0.5,
                    seed=17, ctx=bool(k % 2), scene="ten roots", group=-1)
    return _drawn_case(k)


def _drawn_case(k):
    """case k of the randomised parity run: dict(recs (n, 4) float32, K1, K2 (fx, fy, cx, cy), iterations, threshold, seed, ctx,
    scene, group).  A pure function of k.  Cases 8 b .. 8 b + 3 of every third block b of eight share K1 / K2 / iterations /
    threshold / seed and also go through hak_find_essential_batch as one ragged group (`group` = b, else -1)."""
    from akaze_hip import synth
    rng = np.random.default_rng([PARITY_SEED, k])
    pick = lambda seq: seq[int(rng.integers(len(seq)))]

    def calib(g):
        fx = float(np.float32(g.uniform(300, 3000)))
        return (fx, float(np.float32(fx * g.uniform(0.9, 1.1))), float(np.float32(g.uniform(300, 1600))), float(np.float32(g.uniform(200, 900))))

    K1, K2 = calib(rng), calib(rng)
    n = int(pick((rng.integers(0, 5), 5, 6, rng.integers(7, 301), rng.integers(7, 301), rng.integers(300, 3001))))
    scene = pick(PARITY_SCENES)
    m = max(n, 8)
    if scene in ("general", "planar", "sideways", "forward"):
        R = np.eye(3) if scene in ("sideways", "forward") else synth.rotation_zyx(rng.uniform(-15, 15, 3))
        t = {"sideways": np.array([1.0, 0.0, 0.0]), "forward": np.array([0.0, 0.0, 1.0])}.get(scene, rng.normal(size=3))
        b1 = np.stack([rng.uniform(-0.5, 0.5, 3 * m), rng.uniform(-0.3, 0.3, 3 * m), np.ones(3 * m)], axis=1)
        z = rng.uniform(4.0, 12.0, 3 * m)
        if scene == "planar":
            z = 8.0 / (b1 @ np.array([0.2, -0.1, 1.0]))
        X = b1 * z[:, None]
        X2 = X @ R.T + t
        keep = X2[:, 2] > 0.5
        b1, b2 = b1[keep][:m], (X2[keep] / X2[keep][:, 2:])[:m]
        while len(b1) < m:                                              # (never with these ranges; keeps n records whatever happens)
            b1, b2 = np.concatenate([b1, b1]), np.concatenate([b2, b2])
        recs = np.stack([b1[:m, 0] * K1[0] + K1[2], b1[:m, 1] * K1[1] + K1[3], b2[:m, 0] * K2[0] + K2[2], b2[:m, 1] * K2[1] + K2[3]], axis=1)
        recs += rng.normal(0, float(pick((0.0, 0.3, 1.0))), recs.shape)
    elif scene == "collinear":
        s = rng.uniform(0, 1, m)
        recs = np.stack([100 + 1500 * s, 200 + 700 * s, 300 + 1200 * s ** 1.1, 900 - 650 * s], axis=1)
    elif scene == "lattice":
        q = int(pick((2, 3, 5)))
        recs = np.concatenate([rng.integers(0, q, (m, 2)) * float(pick((1, 7, 100))), rng.integers(0, q + 1, (m, 2)) * float(pick((1, 7, 100)))],
                              axis=1).astype(np.float64)
    else:
        recs = np.tile(rng.uniform(0, 1000, (1, 4)), (m, 1))
    rate = float(rng.uniform(0.0, 0.9)) if rng.random() < 0.7 else 0.0
    out = rng.random(m) < rate
    if scene not in ("equal", "lattice"):
        recs[out] = rng.uniform(0, 2000, (int(out.sum()), 4))
    recs = recs.astype(np.float32)[:n]
    if n and rng.random() < 0.3:                                        # NaN / inf rows
        bad = rng.random(n) < 0.15
        recs[bad, rng.integers(0, 4, int(bad.sum()))] = np.array([np.nan, np.inf, -np.inf], np.float32)[rng.integers(0, 3, int(bad.sum()))]
    if n and rng.random() < 0.25:                                       # exact duplicates, up to all-equal
        share = float(pick((0.25, 0.6, 1.0)))
        recs[rng.random(n) < share] = recs[int(rng.integers(n))]
    its = (1, 5, 6, 7, 64, 100, 257)
    c = dict(recs=recs, K1=K1, K2=K2, iterations=int(pick(its)), threshold=float(np.float32(rng.uniform(0.2, 8.0))),
             seed=int(pick((0, 0xFFFFFFFF, int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 2 ** 32))))), ctx=bool(rng.integers(2)),
             scene=scene, group=-1)
    if (k // 8) % 3 == 0 and k % 8 < 4:
        g = np.random.default_rng([PARITY_SEED, k // 8, 5])
        c.update(K1=calib(g), K2=calib(g), iterations=int(its[int(g.integers(len(its)))]), threshold=float(np.float32(g.uniform(0.2, 8.0))),
                 seed=int((0, 0xFFFFFFFF, int(g.integers(0, 2 ** 32)))[int(g.integers(3))]), group=k // 8)
    return c


@pytest.fixture(scope="module")
def parity_runs():
    """(case, record, mask) of every committed case by the statement, computed once"""
    out = []
    for k in range(PARITY_CASES):
        c = parity_case(k)
        out.append((c,) + er.find_essential(c["recs"], c["K1"], c["K2"], c["iterations"], c["threshold"], c["seed"]))
    return out


def test_parity_cases_reach_the_rare_branches(parity_runs):
    """what the statement alone says about the committed cases: winners in every virtual group of the scratch (root - 16 in 0..3, 4..7
    and 8..9, the last by the two built members), hypotheses with 2, 4 and at least 6 real
    roots, lists without a model, and ties on the winning count between different (h, root), which the smallest-h-then-smallest-root
    rule decides"""
    assert parity_case(5)["recs"].tobytes() == parity_case(5)["recs"].tobytes() and parity_case(5)["K1"] == parity_case(5)["K1"]
    groups, nroots_seen = [0, 0, 0], set()
    no_model = ties = tie_by_root = 0
    scenes = set()
    for c, r, mask in parity_runs:
        scenes.add(c["scene"])
        no_model += r["hypothesis"] < 0
        rec = hr.records(c["recs"])
        F, valid, nroots = er.models(rec, c["K1"], c["K2"], c["seed"], np.arange(c["iterations"]), roots=True)
        nroots_seen |= set(int(v) for v in nroots)
        if r["hypothesis"] < 0:
            continue
        groups[(int(r["root"]) - 16) // 4] += 1
        hh, rr_ = np.nonzero(valid)
        t2 = np.float32(c["threshold"]) * np.float32(c["threshold"])
        cnt = fr.inlier_mask(F[hh, rr_], rec, t2).sum(axis=1)
        j = int(np.argmax(cnt))
        assert cnt.max() == r["inliers"] and (hh[j], 16 + rr_[j]) == (r["hypothesis"], r["root"])
        top = cnt == cnt.max()
        ties += top.sum() >= 2
        tie_by_root += (top & (hh == hh[j])).sum() >= 2
    print(f"winners per virtual group {groups}, real roots seen {sorted(nroots_seen)}, no model {no_model}, ties {ties}, "
          f"ties within the winning hypothesis {tie_by_root}")
    assert scenes == set(PARITY_SCENES) | {"ten roots"} and 10 in nroots_seen
    assert groups[0] >= 10 and groups[1] >= 3 and groups[2] >= 2 and {2, 4} <= nroots_seen and max(nroots_seen) >= 6 and -1 in nroots_seen
    assert no_model >= 5 and ties >= 5 and tie_by_root >= 1, (no_model, ties, tie_by_root)


def test_entry_points_exported(ah):
    out = subprocess.check_output(["nm", "-D", "--defined-only", ah.LIB_PATH], text=True)
    exported = set(re.findall(r" T (hak_[a-z0-9_]+)", out))
    assert {"hak_find_essential", "hak_find_essential_batch"} <= exported
    cxx = subprocess.check_output(["nm", "-D", "-C", "--defined-only", os.path.join(os.path.dirname(ah.LIB_PATH), "libakaze_hip.so")],
                                  text=True)
    assert "akaze::cuFindEssential(" in cxx
    assert callable(ah.findEssential)
    header = open(os.path.join(ROOT, "include", "akaze.h")).read()
    stub = open(os.path.join(ROOT, "cuda-akaze_amd", "host", "asan", "stub_hipakaze.cpp")).read()
    main = open(os.path.join(ROOT, "cuda-akaze_amd", "host", "asan", "asan_main.cpp")).read()
    assert "int cuFindEssential(" in header and "int hak_find_essential(" in stub and "cuFindEssential(" in main


def test_refusals_need_no_device(ah):
    """every refusal of include/hipakaze.h returns non-zero with a message before a device is touched"""
    rec = np.zeros((), ah.FUNDAMENTAL_DTYPE)
    buf = np.zeros(64, ah.MATCH_PAIR_DTYPE)                             # an address to stand for a list: it is never read
    lst, out = buf.ctypes.data, rec.ctypes.data
    K = ah.intrinsics((1500.0, 1500.0, 960.0, 540.0))
    k = K.ctypes.data
    bad_k = []
    for f, v in (("fx", 0.0), ("fy", 0.0), ("fx", np.nan), ("fy", np.inf), ("cx", np.nan), ("cy", -np.inf)):
        b = K.copy()
        b[f] = v
        bad_k.append(b)
    lib = ah.lib
    single = [
        (None, None, 0, k, k, 0, 1.0, 0, None, out),                    # iterations 0
        (None, None, 0, k, k, 65537, 1.0, 0, None, out),
        (None, None, 0, k, k, 10, float("nan"), 0, None, out),
        (None, None, 0, k, k, 10, float("inf"), 0, None, out),
        (None, None, 0, k, k, 10, 0.0, 0, None, out),
        (None, None, 0, k, k, 10, -1.0, 0, None, out),
        (None, None, -1, k, k, 10, 1.0, 0, None, out),                  # negative n
        (None, None, 5, k, k, 10, 1.0, 0, None, out),                   # no list
        (None, lst + 4, 5, k, k, 10, 1.0, 0, None, out),                # a misaligned list
        (None, None, 0, k, k, 10, 1.0, 0, None, None),                  # no h_out
        (None, None, 0, None, k, 10, 1.0, 0, None, out),                # no K1
        (None, None, 0, k, None, 10, 1.0, 0, None, out),                # no K2
    ]
    single += [(None, None, 0, b.ctypes.data, k, 10, 1.0, 0, None, out) for b in bad_k]
    single += [(None, None, 0, k, b.ctypes.data, 10, 1.0, 0, None, out) for b in bad_k]
    for args in single:
        assert lib.hak_find_essential(*args) != 0, args
        assert lib.hak_last_error().decode() != ""
    assert lib.hak_find_essential_batch(None, lst, 8, lst, 1, k, k, 10, 1.0, 0, out, None) != 0      # no context
    assert lib.hak_last_error().decode() != ""
    if ah.device_count() == 0:
        assert lib.hak_find_essential(None, None, 0, k, k, 10, 1.0, 0, None, out) != 0
        assert "no HIP device" in lib.hak_last_error().decode()
