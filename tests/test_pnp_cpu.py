"""CPU suite: track linking and RANSAC absolute pose (hak_link_tracks, hak_solve_pnp).  The numpy statements of the contracts
(tests/link_ref.py and tests/pnp_ref.py, the checkers of the GPU tests) are held against planted scenes: exact recovery over a
table of poses, points behind the camera, the noisy chain fundamental -> refit -> pose -> link -> PnP over three views, the
degenerate inputs and the link rule's corner cases; the entry points are exported and refuse bad arguments without a device."""
import ctypes as C

import numpy as np
import pytest

import fundamental_ref as fr
import fundamental_refit_ref as rr
import link_ref as lr
import pnp_ref as pn
import pose_ref as pr
from test_pose_cpu import dir_angle, rot_angle

# the pose table: 6 rotations (degrees about x, y, z; R = Rz Ry Rx) x 7 translations, Xc = R X + t.  It holds R = I, translations
# along the optical axis in both directions and rolls of 170 degrees and more
ROTATIONS = [(0, 0, 0), (2, -5, 1.5), (0, 0, 170), (10, 3, -20), (-4, 8, 90), (1, -2, -175)]
TRANSLATIONS = [(0, 0, 0), (0, 0, 2), (0, 0, -1.5), (1, 0, 0), (-0.9, -0.1, 0.25), (0.3, -1, 0.2), (-5, 4, 20)]
TABLE = [(a, b, 7 * i + j) for i, a in enumerate(ROTATIONS) for j, b in enumerate(TRANSLATIONS)]
BEHIND = 9                                                              # the table entry with a third of its points behind the camera
N_TABLE, ITER_TABLE, THR_TABLE = 60, 64, 0.5
FOCAL, W, H = 1500.0, 1920, 1080
K_TABLE = (FOCAL, FOCAL, W / 2.0, H / 2.0)
# the angle THR_TABLE px subtends at the focal length: a rotation error above it moves a point near the principal point by more
# than the threshold
ROT_BOUND_DEG = float(np.degrees(np.arctan(THR_TABLE / FOCAL)))
# (measured over the table with the statement: worst rotation error 3.9e-4 degrees, worst |t - t_true| 7.0e-5 scene units with
# the points 4 .. 12 units from the camera; the test prints both)
# the noisy legs: (points, noise px, seed) with 30 % wrong matches in each list
NOISY = [(400, 0.5, 1), (400, 1.0, 2), (400, 0.5, 3), (400, 1.0, 4)]


@pytest.fixture(scope="module")
def synth(ah):
    from akaze_hip import synth
    return synth


def corr_array(X, uv):
    c = np.zeros(len(X), pn.CORR3D_DTYPE)
    c["X"], c["Y"], c["Z"] = np.asarray(X, np.float64).T
    c["u"], c["v"] = np.asarray(uv, np.float64).T
    c["src3d"] = c["src2d"] = np.arange(len(X))
    return c


def table_case(synth, k):
    """entry k: (correspondences rounded to float32, R, t, in front flags).  The points are drawn in the NEW camera's frustum at
    depths 4 .. 12 and moved to the frame the pose maps from; in entry BEHIND every third point is mirrored through the camera
    centre: it projects onto the same pixel from behind the camera"""
    angles, t, seed = TABLE[k]
    rng = np.random.default_rng(1000 + seed)
    R, t = synth.rotation_zyx(angles), np.asarray(t, np.float64)
    z = rng.uniform(4.0, 12.0, N_TABLE)
    uv = np.stack([rng.uniform(0, W, N_TABLE), rng.uniform(0, H, N_TABLE)], axis=1)
    Xc = np.stack([(uv[:, 0] - W / 2.0) / FOCAL * z, (uv[:, 1] - H / 2.0) / FOCAL * z, z], axis=1)
    front = np.ones(N_TABLE, bool)
    if k == BEHIND:
        front[::3] = False
        Xc[~front] = -Xc[~front]
    return corr_array((Xc - t) @ R, uv), R, t, front


@pytest.fixture(scope="module")
def table_runs(synth):
    runs = []
    for k in range(len(TABLE)):
        corr, R, t, front = table_case(synth, k)
        runs.append((corr, R, t, front, pn.solve_pnp(corr, K_TABLE, ITER_TABLE, THR_TABLE, k)))
    return runs


def test_exact_recovery_over_the_pose_table(table_runs):
    assert len(TABLE) >= 40
    worst_rot = worst_t = 0.0
    solutions = set()
    for k, (corr, R, t, front, (out, mask)) in enumerate(table_runs):
        assert out["hypothesis"] >= 0 and out["n"] == N_TABLE, (k, out)               # every scene yields a model
        assert mask.dtype == np.uint8 and np.array_equal(mask.astype(bool), front), (k, out)
        assert out["inliers"] == front.sum()
        solutions.add(int(out["solution"]))
        a = rot_angle(out["R"].reshape(3, 3), R)
        assert a < ROT_BOUND_DEG, (k, a)
        worst_rot, worst_t = max(worst_rot, a), max(worst_t, float(np.linalg.norm(out["t"].astype(np.float64) - t)))
    print(f"pnp table: worst rotation {worst_rot:.3e} deg (bound {ROT_BOUND_DEG:.3e}), worst |t - t_true| {worst_t:.3e}, "
          f"winning solutions {sorted(solutions)}")
    assert len(solutions) > 1                                           # more than one root of the quartic wins somewhere
    # the table holds what the contract names
    assert (0, 0, 0) in ROTATIONS and (0, 0, 2) in TRANSLATIONS and any(abs(a[2]) >= 170 for a in ROTATIONS)
    front = table_runs[BEHIND][3]
    assert (~front).sum() == N_TABLE // 3 and not table_runs[BEHIND][4][1][~front].any()


def test_true_pose_is_among_the_solutions(synth):
    """the algebra of steps 2-5: on noise-free inputs (rounded to float32) the solutions of nearly every sample hold the planted
    pose"""
    worst = []
    for k in (1, 8, 16, 25, 33, 41):
        corr, R, t, front = table_case(synth, k)
        rec = pn.records(corr)
        M, valid = pn.models(rec, pr.intrinsics(K_TABLE), k, np.arange(32))
        for h in range(32):
            errs = [rot_angle(M[h, s, :9].reshape(3, 3), R) + float(np.linalg.norm(M[h, s, 9:].astype(np.float64) - t))
                    for s in range(4) if valid[h, s]]
            if k == BEHIND and not front[pn.sample_indices(k, [h], N_TABLE)[0][0]].all():
                continue                                                # a sample with a point behind the camera plants nothing
            if errs:
                worst.append(min(errs))
    assert len(worst) > 150                                             # nearly every sample gives a model
    print(f"best solution per sample: median {np.median(worst):.2e}, 95th percentile {np.percentile(worst, 95):.2e}")
    assert np.median(worst) < 1e-3 and np.percentile(worst, 95) < 0.1    # float32 inputs; ill-conditioned samples are the tail


def chain(synth, n, noise, seed):
    """the statement chain over one three_view_scene -> (corr, planted flags per correspondence, pnp record, mask, R02, t02)"""
    K, (R01, t01), (R12, t12), A, B, fa, fb, X0, pa, pb = synth.three_view_scene(seed, n, noise, 0.3)
    rec0, _ = fr.find_fundamental(A, 256, 1.0, seed)
    rec1, _ = rr.refine_fundamental(A, rec0, 1.0, 3)
    pose, pmask, xyz = pr.recover_pose(A, rec1, K, None, 1.0, 50.0)
    corr = lr.link_tracks(A, pmask, xyz, B, 2 * n)
    planted = fa[corr["src3d"]] & fb[corr["src2d"]] & (pa[corr["src3d"]] == pb[corr["src2d"]])
    out, mask = pn.solve_pnp(corr, K, 256, 2.0, seed)
    return corr, planted, pose, out, mask, R12 @ R01, R12 @ t01 + t12


def test_noisy_chain_over_three_views(synth):
    for n, noise, seed in NOISY:
        corr, planted, pose, out, mask, R02, t02 = chain(synth, n, noise, seed)
        assert pose["candidate"] >= 0 and out["hypothesis"] >= 0 and out["inliers"] == mask.sum() > 0
        share = planted[mask == 1].mean()
        a, b = rot_angle(out["R"].reshape(3, 3), R02), dir_angle(out["t"], t02)
        print(f"noisy n={n} noise={noise} seed={seed}: {len(corr)} linked, {planted.sum()} planted, {out['inliers']} inliers of which "
              f"planted {share:.3f}; rotation {a:.4f} deg, translation direction {b:.4f} deg, "
              f"|t| {np.linalg.norm(out['t']):.4f} (planted {np.linalg.norm(t02) / np.linalg.norm((-1.0, 0.05, 0.1)):.4f})")
        assert share > 0.7, (n, noise, seed, share)


def _no_model(out, mask, n):
    return (out["hypothesis"] == -1 and out["inliers"] == 0 and out["solution"] == 0 and out["n"] == n and not out["t"].any()
            and np.array_equal(out["R"], np.eye(3, dtype=np.float32).reshape(9)) and not mask.any() and len(mask) == n)


def test_degenerate_inputs(synth):
    corr, R, t, front = table_case(synth, 10)
    for n in (0, 1, 2):
        assert _no_model(*pn.solve_pnp(corr[:n], K_TABLE, 64, 0.5, 0), n)
    out, mask = pn.solve_pnp(corr[:3], K_TABLE, 64, 0.5, 0)              # three points: the sample itself fits
    assert out["hypothesis"] >= 0 and out["inliers"] == 3
    line = corr[:3].copy()
    for f in ("X", "Y", "Z"):
        line[f][2] = 0.5 * (line[f][0] + line[f][1])                    # three collinear points: no triad
    assert _no_model(*pn.solve_pnp(line, K_TABLE, 64, 0.5, 0), 3)
    same = corr.copy()
    for f in ("X", "Y", "Z", "u", "v"):
        same[f] = same[f][0]                                            # all points identical: b2 = 0
    assert _no_model(*pn.solve_pnp(same, K_TABLE, 64, 0.5, 0), N_TABLE)
    for f, bad in (("X", np.nan), ("Z", np.inf), ("u", -np.inf), ("v", np.nan)):
        allbad = corr.copy()
        allbad[f] = bad
        assert _no_model(*pn.solve_pnp(allbad, K_TABLE, 64, 0.5, 0), N_TABLE), f
        some = corr.copy()
        some[f][::2] = bad                                              # half the records: they are never inliers, the rest are
        out, mask = pn.solve_pnp(some, K_TABLE, 64, 0.5, 0)
        assert out["hypothesis"] >= 0 and not mask[::2].any() and mask[1::2].all(), f
    one, m1 = pn.solve_pnp(corr, K_TABLE, 1, 0.5, 3)                     # iterations = 1: hypothesis 0 or nothing
    assert one["hypothesis"] in (0, -1) and one["inliers"] == m1.sum()
    many = pn.solve_pnp(corr, K_TABLE, 64, 0.5, 3)[0]
    assert many["inliers"] >= one["inliers"]


# ---- the committed cases of test_gpu_pnp.py::test_randomised_parity and of the P3P leg of test_gpu_ransac_trace.py: drawn here so
# that what they reach can be asserted on the statement alone
PARITY_SEED, PARITY_CASES = 2045, 150
PARITY_SCENES = ("general", "coplanar", "collinear", "lattice", "near", "far")
PARITY_CAMERAS = ("table", "anisotropic", "outside", "long", "short")
PARITY_ITERATIONS = (1, 7, 64, 100, 257)


def parity_camera(rng, kind):
    """(fx, fy, cx, cy): K_TABLE, fx != fy, a principal point outside the image, the focal length scaled by 2^10 and by 2^-10"""
    if kind == "anisotropic":
        return (float(rng.uniform(800, 2000)), float(rng.uniform(800, 2000)), W / 2.0 + 13.0, H / 2.0 - 7.0)
    if kind == "outside":
        return (FOCAL, FOCAL, float((-700.0, W + 900.0)[int(rng.integers(2))]), float((-400.0, H + 300.0)[int(rng.integers(2))]))
    if kind == "long":
        return (FOCAL * 1024.0, FOCAL * 1024.0, W / 2.0, H / 2.0)
    if kind == "short":
        return (FOCAL / 1024.0, FOCAL / 1024.0, W / 2.0, H / 2.0)
    return K_TABLE


def parity_case(k):
    """case k of the randomised P3P family run: dict(corr (n,) CORR3D_DTYPE, K (fx, fy, cx, cy), iterations, threshold, seed, ctx,
    scene, camera, group).  A pure function of k.  Cases 8 b .. 8 b + 3 of every third block b of eight share K / iterations /
    threshold / seed and also go through hak_solve_pnp_batch as one ragged group (`group` = b, else -1).
    Scenes: a general planted pose; coplanar points (three quarters fronto-parallel: world Z constant under R = I; two of those three on a ring about the optical
    axis, where most samples have three or four solutions); collinear points (two
    thirds exactly: integer steps along an integer direction); an integer lattice of 2, 3 or 5 values per axis (isosceles and
    equilateral samples, a2 == c2, ties in the counts); points near or behind the centre of projection; far points at depths of
    1e3 .. 1e6.  Independent axes: the camera, the outlier rate 0 .. 0.9, NaN / +-inf rows, duplicates up to all-equal (two
    sample points at one place give c2 == 0, hence A4 == 0, or b2 == 0), the world scaled by 2^{-20, -8, 0, 8, 20} and offset by
    +-16000, observation noise, threshold, iterations, seeds 0, 0xFFFFFFFF and random."""
    from akaze_hip import synth
    rng = np.random.default_rng([PARITY_SEED, k])
    grp = np.random.default_rng([PARITY_SEED, k // 8, 5])
    pick = lambda seq: seq[int(rng.integers(len(seq)))]
    n = int(pick((rng.integers(0, 7), 7, 8, rng.integers(9, 301), rng.integers(9, 301), rng.integers(300, 3001),
                  pick((1023, 1024, 1025)))))
    scene = pick(PARITY_SCENES + ("coplanar",))                         # (coplanar twice: its ring scenes carry the three- and
    camera = pick(PARITY_CAMERAS)                                       # four-model hypotheses and the winners at solutions 2 and 3)
    K = parity_camera(rng, camera)
    group = k // 8 if (k // 8) % 3 == 0 and k % 8 < 4 else -1
    if group >= 0:                                                      # one K per batch call
        camera = PARITY_CAMERAS[int(grp.integers(len(PARITY_CAMERAS)))]
        K = parity_camera(grp, camera)
    fx, fy, cx, cy = K
    m = max(n, 8)
    R, t = synth.rotation_zyx(rng.uniform(-25, 25, 3)), rng.uniform(-1, 1, 3)
    uv = np.stack([rng.uniform(0, W, m), rng.uniform(0, H, m)], axis=1)
    ray = np.stack([(uv[:, 0] - cx) / fx, (uv[:, 1] - cy) / fy, np.ones(m)], axis=1)
    Xw = None
    if scene == "general":
        Xc = ray * rng.uniform(4.0, 12.0, (m, 1))
    elif scene == "far":
        Xc = ray * 10.0 ** rng.uniform(3.0, 6.0, (m, 1))
    elif scene == "near":                                               # around the centre of projection, a good share behind it
        Xc = np.stack([rng.uniform(-2, 2, m), rng.uniform(-2, 2, m), rng.uniform(-1, 2, m)], axis=1)
    elif scene == "coplanar":
        shape = rng.random()
        if shape < 3 / 4:
            R, t, nrm = np.eye(3), np.zeros(3), np.array([0.0, 0.0, 1.0])
        else:
            nrm = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), 1.0])
        if shape < 1 / 2:                                               # a ring about the optical axis, the camera above its centre:
            a = rng.uniform(0, 2 * np.pi, m)                            # most samples have three and four solutions
            ray = np.stack([np.cos(a), np.sin(a), np.ones(m)], axis=1) * \
                np.stack([rng.uniform(0.15, 0.9) * (1.0 + rng.uniform(-1, 1, m) * float(pick((0.0, 0.05, 0.3, 0.3))))] * 2 + [np.ones(m)], axis=1)
        Xc = ray * (float(pick((4.0, 8.0, 10.5))) / (ray @ nrm))[:, None]
    elif scene == "collinear":
        d = np.array(pick(((1, 0, 0), (0, 1, 0), (1, 1, 0), (1, -2, 1), (2, 3, -1), (0, 0, 1))), np.float64)
        steps = rng.integers(-20, 21, m).astype(np.float64)
        if rng.random() < 1 / 3:
            steps = steps + rng.uniform(-0.5, 0.5, m)                    # off the integers: collinear up to rounding only
        Xw = rng.integers(-5, 6, 3) + steps[:, None] * d * float(pick((1.0, 0.25, 3.0)))
    else:                                                               # lattice
        q, sp = int(pick((2, 3, 5))), float(pick((1, 7, 100)))
        Xw = rng.integers(0, q, (m, 3)).astype(np.float64) * sp
    if Xw is None:
        Xw = (Xc - t) @ R                                                # Xc = R Xw + t
    else:                                                               # the camera looks at the cloud from three extents away
        ext = max(float(np.ptp(Xw, axis=0).max()), 1.0)
        t = np.array([rng.uniform(-0.2, 0.2) * ext, rng.uniform(-0.2, 0.2) * ext, 3.0 * ext]) - R @ Xw.mean(axis=0)
        Xc = Xw @ R.T + t
    with np.errstate(all="ignore"):
        obs = np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], axis=1)
    if scene != "lattice":
        obs = obs + rng.normal(0, float(pick((0.0, 0.0, 0.3, 1.0))), obs.shape)
    rate = float(rng.uniform(0.0, 0.9)) if rng.random() < 0.7 else 0.0
    out = rng.random(m) < rate
    fin = obs[np.isfinite(obs).all(axis=1)]
    lo, hi = (float(np.clip(fin.min(), -4000, 0)), float(np.clip(fin.max(), 8, 4000))) if len(fin) else (0.0, float(W))
    draw = rng.uniform(lo, hi + 1, (int(out.sum()), 2))
    obs[out] = np.floor(draw) if scene == "lattice" else draw
    Xw = Xw * 2.0 ** int(pick((0, 0, 0, -20, -8, 8, 20)))
    if rng.random() < 0.3:
        Xw = Xw + float(pick((-16000.0, 16000.0))) * np.array([rng.integers(0, 2), rng.integers(0, 2), 1.0])
    with np.errstate(all="ignore"):
        corr = corr_array(Xw, obs)[:n]
    if n and rng.random() < 0.3:                                        # NaN / inf rows
        bad = np.nonzero(rng.random(n) < 0.15)[0]
        for i in bad:
            corr[("X", "Y", "Z", "u", "v")[int(rng.integers(5))]][i] = (np.nan, np.inf, -np.inf)[int(rng.integers(3))]
    if n and rng.random() < 0.3:                                        # exact duplicates, up to all-equal
        share = float(pick((0.25, 0.6, 1.0)))
        src = corr[int(rng.integers(n))].copy()
        sel = rng.random(n) < share
        for f in ("X", "Y", "Z", "u", "v"):
            corr[f][sel] = src[f]
    c = dict(corr=corr, K=K, iterations=int(pick(PARITY_ITERATIONS)), threshold=float(np.float32(rng.uniform(0.2, 8.0))),
             seed=int(pick((0, 0xFFFFFFFF, int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 2 ** 32))))), ctx=bool(rng.integers(2)),
             scene=scene, camera=camera, group=group)
    if group >= 0:
        c.update(iterations=int(PARITY_ITERATIONS[int(grp.integers(5))]), threshold=float(np.float32(grp.uniform(0.2, 8.0))),
                 seed=int((0, 0xFFFFFFFF, int(grp.integers(0, 2 ** 32)))[int(grp.integers(3))]))
    return c


def hypothesis_stages(rec, K, seed, iterations):
    """where the statement's steps 1-5 stop each hypothesis 0 .. iterations - 1, recomputed with pnp_ref's own functions:
    dict(stage (iterations,) of "sample" (no three distinct indices, or n < 3), "input" (b2 == 0 or a non-finite a2, b2, c2 or
    cosine), "A4" (A4 == 0), "quartic" (a non-finite coefficient or bound, or a failed cubic), "triad" (the world points' triad)
    and "solved"; critical (iterations,) the cubic's real-root count where it was solved, else 0; roots (iterations,) the quartic's
    bracketed roots; models (iterations,) the solutions that gave a model; rejected (iterations,) the roots that did not)"""
    hs = np.arange(iterations)
    stage = np.full(iterations, "sample", dtype=object)
    zero = np.zeros(iterations, np.int64)
    out = dict(stage=stage, critical=zero.copy(), roots=zero.copy(), models=zero.copy(), rejected=zero.copy())
    if len(rec) < 3:
        return out
    idx, ok = pn.sample_indices(seed, hs, len(rec))
    pt = rec[np.where(idx < 0, 0, idx)].astype(np.float64)
    fx, fy, cx, cy = (np.float64(K[f]) for f in ("fx", "fy", "cx", "cy"))
    with np.errstate(all="ignore"):
        X, b = [], []
        for q in range(3):
            X.append([pt[:, q, 0], pt[:, q, 1], pt[:, q, 2]])
            x, y = (pt[:, q, 3] - cx) / fx, (pt[:, q, 4] - cy) / fy
            nrm = np.sqrt((x * x + y * y) + 1.0)
            b.append([x / nrm, y / nrm, 1.0 / nrm])
        da, db, dc = pn._sub(X[1], X[2]), pn._sub(X[0], X[2]), pn._sub(X[0], X[1])
        a2, b2, c2 = pn._dot(da, da), pn._dot(db, db), pn._dot(dc, dc)
        ca, cb, cg = pn._dot(b[1], b[2]), pn._dot(b[0], b[2]), pn._dot(b[0], b[1])
        ok_in = b2 != 0.0
        for v in (a2, b2, c2, ca, cb, cg):
            ok_in = ok_in & np.isfinite(v)
        A4, A3, A2, A1, A0, _ = pn.quartic(a2, b2, c2, ca, cb, cg)
        roots, count, okr = pn.positive_roots(A4, A3, A2, A1, A0)
        _, ccount, _ = fr.real_roots(np.ones(iterations), 0.75 * (A3 / A4), 0.5 * (A2 / A4), 0.25 * (A1 / A4))
        okf = pn._triad(X[0], X[1], X[2])[3]
    left = ok.copy()
    for name, passed in (("input", ok_in), ("A4", A4 != 0.0), ("quartic", okr), ("triad", okf)):
        stage[left & ~passed] = name
        left = left & passed
    stage[left] = "solved"
    _, valid = pn.models(rec, K, seed, hs)
    assert not valid[~left].any()
    out["critical"] = np.where(left, ccount, 0)
    out["roots"] = np.where(left, count, 0)
    out["models"] = valid.sum(axis=1)
    out["rejected"] = out["roots"] - out["models"]
    return out


@pytest.fixture(scope="module")
def parity_runs():
    """(case, records, intrinsics, stages, statement record) of every parity case, computed once"""
    runs = []
    for k in range(PARITY_CASES):
        c = parity_case(k)
        rec, K = pn.records(c["corr"]), pr.intrinsics(c["K"])
        runs.append((c, rec, K, hypothesis_stages(rec, K, c["seed"], c["iterations"]),
                     pn.solve_pnp(c["corr"], c["K"], c["iterations"], c["threshold"], c["seed"])[0]))
    return runs


def test_parity_cases_are_pure_and_cover_the_axes(parity_runs):
    a, b = parity_case(5), parity_case(5)
    assert a["corr"].tobytes() == b["corr"].tobytes() and {f: a[f] for f in a if f != "corr"} == {f: b[f] for f in b if f != "corr"}
    cases = [r[0] for r in parity_runs]
    assert {c["scene"] for c in cases} == set(PARITY_SCENES) and {c["camera"] for c in cases} == set(PARITY_CAMERAS)
    assert {c["iterations"] for c in cases} == set(PARITY_ITERATIONS) and {0, 0xFFFFFFFF} <= {c["seed"] for c in cases}
    sizes = {len(c["corr"]) for c in cases}
    assert {0, 1, 2, 3, 4, 5, 6, 7, 8} <= sizes and sizes & {1023, 1024, 1025} and max(sizes) > 1025
    groups = sorted({c["group"] for c in cases if c["group"] >= 0})
    assert len(groups) >= 5
    for g in groups:
        ks = [c for c in cases if c["group"] == g]
        assert len(ks) == 4 and len({(c["K"], c["iterations"], c["threshold"], c["seed"]) for c in ks}) == 1
    assert sum(not np.isfinite(pn.records(c["corr"])[:, 0]).all() for c in cases) >= 10          # lists with NaN / inf rows
    assert sum(len(c["corr"]) > 3 and len(np.unique(c["corr"][["X", "Y", "Z", "u", "v"]])) < 0.8 * len(c["corr"]) for c in cases) >= 10


def test_parity_cases_reach_the_rare_branches(parity_runs):
    """what the statement alone says about the committed cases; conditions on the inputs, not measurements of the kernel.  Counted
    when written, over the 13 906 hypotheses of the 150 cases: stopped at the sample 281, at b2 == 0 or a non-finite input 3 759,
    at A4 == 0 537, at the world triad 1 391, solved 7 938 (none stops at a non-finite quartic coefficient or in the cubic); cubics
    with one critical point 4 150, with three 3 788; hypotheses with 0 / 1 / 2 / 3 / 4 bracketed roots 6 990 / 2 738 / 3 841 / 165 /
    172 and with as many models 7 752 / 3 171 / 2 756 / 89 / 138; 1 981 hypotheses with a root that den, w, s1 .. s3 or the second
    triad rejects; winners at solution >= 1 in 38 cases, >= 2 in 10; ties on the winning count in 66; 59 lists without a model.
    Three- and four-model hypotheses and winners at solutions 2 and 3 come almost only from the ring scenes, and few seeds give five
    such winners: PARITY_SEED is the one of 2031 .. 2046 with the most (the others: 2 .. 8)."""
    stage, critical, roots, models = {}, {}, {}, {}
    rejected = later1 = later2 = ties = no_model = 0
    for c, rec, K, st, r in parity_runs:
        for name, into in (("stage", stage), ("critical", critical), ("roots", roots), ("models", models)):
            for v, cnt in zip(*np.unique(st[name], return_counts=True)):
                into[v] = into.get(v, 0) + int(cnt)
        rejected += int((st["rejected"] > 0).sum())
        later1 += r["hypothesis"] >= 0 and r["solution"] >= 1
        later2 += r["hypothesis"] >= 0 and r["solution"] >= 2
        no_model += r["hypothesis"] < 0
        if r["hypothesis"] >= 0:
            M, valid = pn.models(rec, K, c["seed"], np.arange(c["iterations"]))
            hh, rr = np.nonzero(valid)
            t2 = np.float32(c["threshold"]) * np.float32(c["threshold"])
            cnt = pn.inlier_mask(M[hh, rr], rec, K, t2).sum(axis=1)
            assert cnt.max() == r["inliers"] and (hh[np.argmax(cnt)], rr[np.argmax(cnt)]) == (r["hypothesis"], r["solution"])
            ties += (cnt == cnt.max()).sum() >= 2
    got = dict(stage=stage, critical=critical, roots=roots, models=models, rejected=rejected, later1=int(later1), later2=int(later2),
               ties=int(ties), no_model=int(no_model))
    print("p3p parity cases:", got)
    assert all(models.get(s, 0) >= 50 for s in range(5)), models        # hypotheses with 0, 1, 2, 3 and 4 models
    assert all(roots.get(s, 0) >= 50 for s in range(5)), roots          # ... and with 0 .. 4 bracketed roots
    assert critical.get(1, 0) >= 50 and critical.get(3, 0) >= 50, critical
    assert all(stage.get(s, 0) >= 20 for s in ("sample", "input", "A4", "triad")), stage
    assert rejected >= 20                                               # a root rejected by den, w, s1 .. s3 or the second triad
    assert later1 >= 10 and later2 >= 5 and ties >= 10 and no_model >= 10, got


def pairs(query, train, x2=None):
    m = np.zeros(len(query), np.dtype([("query", "<i4"), ("train", "<i4"), ("distance", "<i4"), ("second", "<i4"),
                                       ("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4")]))
    m["query"], m["train"] = query, train
    m["x2"] = np.arange(len(query)) + 0.5 if x2 is None else x2
    m["y2"] = -m["x2"]
    return m


def test_link_rule():
    A = pairs([0, 1, 2, 3, 4, 5, 6], [5, 9, 5, 2, 9, 40, -1])
    xyz = np.arange(21, dtype=np.float32).reshape(7, 3) + 100
    B = pairs([9, 5, 7, 2, 40, 5, -1, 41], [1, 2, 3, 4, 5, 6, 7, 8])
    got = lr.link_tracks(A, None, xyz, B, 40)
    # duplicate trains: the smallest a wins (9 -> a = 1, 5 -> a = 0); query 7 has no match in A; 40 and -1 are out of range
    assert got["src2d"].tolist() == [0, 1, 3, 5] and got["src3d"].tolist() == [1, 0, 3, 0]
    assert np.array_equal(got["X"], xyz[[1, 0, 3, 0], 0]) and np.array_equal(got["Z"], xyz[[1, 0, 3, 0], 2])
    assert np.array_equal(got["u"], B["x2"][[0, 1, 3, 5]]) and np.array_equal(got["v"], B["y2"][[0, 1, 3, 5]]) and not got["pad"].any()
    wide = lr.link_tracks(A, None, xyz, B, 41)                          # max_index = 41 admits train 40
    assert wide["src2d"].tolist() == [0, 1, 3, 4, 5] and wide["src3d"][3] == 5
    mask = np.array([0, 1, 1, 1, 1, 1, 1], np.uint8)                    # a = 0 masked: train 5 falls to a = 2
    masked = lr.link_tracks(A, mask, xyz, B, 40)
    assert masked["src3d"].tolist() == [1, 2, 3, 2]
    mask[[1, 4]] = 0                                                    # every a of train 9 masked: the match is not linked
    assert lr.link_tracks(A, mask, xyz, B, 40)["src2d"].tolist() == [1, 3, 5]
    assert len(lr.link_tracks(A[:0], None, xyz[:0], B, 41)) == 0 and len(lr.link_tracks(A, None, xyz, B[:0], 41)) == 0
    nonfinite = xyz.copy()
    nonfinite[1] = np.nan                                               # still linked: the estimator rejects it
    got = lr.link_tracks(A, None, nonfinite, B, 40)
    assert got["src3d"].tolist() == [1, 0, 3, 0] and np.isnan(got["X"][0])
    assert got.dtype == pn.CORR3D_DTYPE and pn.CORR3D_DTYPE.itemsize == 32


def refusals(ah, ctx, p, cntp):
    """every refused call of the four entry points as (function, arguments): p a valid 16-byte aligned pointer (device memory on a
    machine with one), cntp a valid int pointer; ctx a context or None (then the batch forms are refused for that alone)"""
    lib = ah.lib
    K = ah.intrinsics(K_TABLE)
    keep = [K]

    def k_with(**kw):
        b = K.copy()
        for f, v in kw.items():
            b[f] = v
        keep.append(b)
        return b.ctypes.data

    inf, nan = float("inf"), float("nan")
    kp = K.ctypes.data
    rec = np.zeros((), ah.ABS_POSE_DTYPE)
    cnt = C.c_int(-7)
    keep += [rec, cnt]
    op, cp = rec.ctypes.data, C.byref(cnt)
    pnp, pnpb, link, linkb = lib.hak_solve_pnp, lib.hak_solve_pnp_batch, lib.hak_link_tracks, lib.hak_link_tracks_batch
    bad_k = [k_with(fx=0.0), k_with(fy=0.0), k_with(fx=nan), k_with(fy=inf), k_with(cx=nan), k_with(cy=-inf)]
    out = [(pnp, (None, p, 8, kp, it, 1.0, 0, None, op)) for it in (0, -1, 65537)]
    out += [(pnp, (None, p, 8, kp, 64, thr, 0, None, op)) for thr in (0.0, -1.0, nan, inf)]
    out += [(pnp, (None, p, 8, b, 64, 1.0, 0, None, op)) for b in bad_k]
    out += [(pnp, (None, p, 8, None, 64, 1.0, 0, None, op)), (pnp, (None, p, 8, kp, 64, 1.0, 0, None, None)),
            (pnp, (None, p, -1, kp, 64, 1.0, 0, None, op)), (pnp, (None, None, 8, kp, 64, 1.0, 0, None, op)),
            (pnp, (None, p + 4, 8, kp, 64, 1.0, 0, None, op))]
    out += [(pnpb, (None, p, 64, cntp, 1, kp, 64, 1.0, 0, p, None))]                                   # no context
    if ctx is not None:
        out += [(pnpb, (ctx, None, 64, cntp, 1, kp, 64, 1.0, 0, p, None)), (pnpb, (ctx, p, 64, None, 1, kp, 64, 1.0, 0, p, None)),
                (pnpb, (ctx, p, 64, cntp, 1, kp, 64, 1.0, 0, None, None)), (pnpb, (ctx, p, 64, cntp, 0, kp, 64, 1.0, 0, p, None)),
                (pnpb, (ctx, p, 0, cntp, 1, kp, 64, 1.0, 0, p, None)), (pnpb, (ctx, p + 8, 64, cntp, 1, kp, 64, 1.0, 0, p, None)),
                (pnpb, (ctx, p, 64, cntp, 1, None, 64, 1.0, 0, p, None)), (pnpb, (ctx, p, 64, cntp, 1, kp, 0, 1.0, 0, p, None)),
                (pnpb, (ctx, p, 64, cntp, 1, kp, 64, nan, 0, p, None)), (pnpb, (ctx, p, 64, cntp, 1, bad_k[0], 64, 1.0, 0, p, None)),
                (pnpb, (ctx, p, 64, cntp, 1, bad_k[4], 64, 1.0, 0, p, None))]
    out += [(link, (None, p, 4, None, p, p, 4, 0, p, cp, None)), (link, (None, p, 4, None, p, p, 4, -3, p, cp, None)),    # max_index
            (link, (None, p, -1, None, p, p, 4, 16, p, cp, None)), (link, (None, p, 4, None, p, p, -1, 16, p, cp, None)),
            (link, (None, p, 1 << 30, None, p, p, 4, 16, p, cp, None)), (link, (None, p, 4, None, p, p, 1 << 30, 16, p, cp, None)),
            (link, (None, None, 4, None, p, p, 4, 16, p, cp, None)), (link, (None, p, 4, None, None, p, 4, 16, p, cp, None)),
            (link, (None, p, 4, None, p, None, 4, 16, p, cp, None)), (link, (None, p, 4, None, p, p, 4, 16, None, cp, None)),
            (link, (None, p, 4, None, p, p, 4, 16, p, None, None)),
            (link, (None, p + 4, 4, None, p, p, 4, 16, p, cp, None)), (link, (None, p, 4, None, p, p + 8, 4, 16, p, cp, None)),
            (link, (None, p, 4, None, p, p, 4, 16, p + 4, cp, None))]
    out += [(linkb, (None, p, 64, cntp, 1, None, p, p, 64, cntp, 1, 1, p, 64, cntp))]                  # no context
    if ctx is not None:
        good = [ctx, p, 64, cntp, 1, None, p, p, 64, cntp, 1, 1, p, 64, cntp]
        for pos, val in ((1, None), (3, None), (6, None), (7, None), (9, None), (12, None), (14, None),       # NULL lists, counts, xyz
                         (2, 0), (8, 0), (13, 0), (4, 0), (10, 0), (11, 0),                                 # strides, steps, npairs
                         (1, p + 4), (7, p + 8), (12, p + 4)):                                               # misaligned
            args = list(good)
            args[pos] = val
            out.append((linkb, tuple(args)))
    return out, keep, rec, cnt


def test_entry_points_refuse_bad_arguments_without_a_device(ah):
    """the refusals come before any device is touched, so they hold on a machine without one: the pointers are never followed"""
    assert ah.CORR3D_DTYPE == pn.CORR3D_DTYPE and ah.ABS_POSE_DTYPE == pn.ABS_POSE_DTYPE
    calls, keep, rec, cnt = refusals(ah, None, 4096, 4096)
    assert len(calls) >= 30
    for k, (fn, args) in enumerate(calls):
        assert fn(*args) != 0, (k, args)
        assert ah.lib.hak_last_error().decode() != "", (k, args)
    assert not rec.tobytes().strip(b"\0") and cnt.value == -7            # nothing was written through a refused call's pointers
