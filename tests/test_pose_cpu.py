"""CPU suite: relative pose from the fundamental matrix (hak_recover_pose).  The numpy statement of the contract
(tests/pose_ref.py, the checker of the GPU tests) is held against planted poses: exact recovery over a table of rotations and
baselines in which every one of the four decompositions wins, proper rotations, the noisy chain RANSAC -> refit -> pose, the depth
limit and the degenerate inputs; the entry points are exported and refuse bad arguments without a device."""
import ctypes as C

import numpy as np
import pytest

import fundamental_ref as fr
import fundamental_refit_ref as rr
import pose_ref as pr

# the pose table: 6 rotations (degrees about x, y, z; R = Rz Ry Rx) x 7 baselines.  It holds R = I, a baseline along the optical
# axis in both directions and rolls near 170 degrees; entry k has the image order swapped when (i + j) % 5 == 0
ROTATIONS = [(0, 0, 0), (2, -5, 1.5), (0, 0, 170), (10, 3, -20), (-4, 8, 90), (1, -2, -175)]
BASELINES = [(-1, .05, .1), (1, 0, 0), (0, 0, 1), (0, 0, -1), (0, 1, 0), (.3, -1, .2), (-.5, .5, 2)]
TABLE = [(a, b, 7 * i + j, (i + j) % 5 == 0) for i, a in enumerate(ROTATIONS) for j, b in enumerate(BASELINES)]
N_TABLE = 200
# measured over the table with the statement (float64 pose, R and t rounded to float32; noise-free matches rounded to float32, the
# true F scaled to largest entry 1 and rounded to float32): the worst rotation error, the worst baseline-direction error (degrees),
# the worst relative depth error of a point, the worst |R^T R - I| entry and |det R - 1| of the float32 R
WORST_ROT_DEG, WORST_DIR_DEG, WORST_DEPTH_REL = 3.4e-6, 2.6e-6, 1.4e-5
WORST_ORTHO, WORST_DET = 6.0e-8, 6.0e-8
WINS = [9, 9, 14, 10]                                                   # how often each candidate wins over the table

# the noisy legs: (n, noise px, seed), 70 % planted inliers at the default pose; RANSAC 256 x 1 px and three refit rounds by the
# statements, then the pose at 1 px.  Measured worst over these seeds: rotation and baseline error in degrees (both from
# (300, 1.0, 2), where 1 px of noise at a 1 px threshold leaves 109 inliers; the other five stay below 0.15 and 0.94 degrees)
NOISY = [(300, 0.3, 1), (300, 1.0, 2), (300, 0.6, 3), (1000, 0.3, 4), (1000, 1.0, 5), (1000, 0.6, 6)]
NOISY_WORST_ROT_DEG, NOISY_WORST_DIR_DEG = 0.585, 4.23


def rot_angle(Rg, R):
    """degrees between two rotations, from the chord |Rg - R|_F = 2 sqrt(2) sin(angle / 2) (accurate near 0, unlike arccos)"""
    return float(np.degrees(2.0 * np.arcsin(min(1.0, np.linalg.norm(np.asarray(Rg, np.float64) - R) / (2.0 * np.sqrt(2.0))))))


def dir_angle(tg, t):
    tg, t = np.asarray(tg, np.float64), np.asarray(t, np.float64)
    return float(np.degrees(np.arctan2(np.linalg.norm(np.cross(tg, t)), tg @ t)))


def f32_model(F):
    """the true F scaled to largest entry 1 and rounded to float32, as a hak_fundamental holds it"""
    return (F / F.flat[np.argmax(np.abs(F))]).astype(np.float32).reshape(9)


def table_case(synth, k):
    a, b, seed, swap = TABLE[k]
    recs, _, F, K, R, t, z = synth.two_view_scene(N_TABLE, 0, seed, a, b, swap=swap)
    return recs, f32_model(F), K, R, t, z


@pytest.fixture(scope="module")
def synth(ah):
    from akaze_hip import synth
    return synth


@pytest.fixture(scope="module")
def table_runs(synth):
    """(records, F, K, R, t, z, statement output) of every table entry, computed once"""
    runs = []
    for k in range(len(TABLE)):
        recs, F, K, R, t, z = table_case(synth, k)
        runs.append((recs, F, K, R, t, z, pr.recover_pose(recs, F, K)))
    return runs


def first_winners(runs):
    """candidate -> the first table entry it wins (the GPU suite's one case per candidate)"""
    first = {}
    for k, run in enumerate(runs):
        first.setdefault(int(run[6][0]["candidate"]), k)
    return first


def test_exact_recovery_over_the_pose_table(table_runs):
    wins = [0] * 4
    worst_rot = worst_dir = worst_depth = 0.0
    for k, (recs, F, K, R, t, z, (out, mask, xyz)) in enumerate(table_runs):
        assert out["candidate"] >= 0 and out["n"] == N_TABLE, (k, out)
        assert out["in_front"] == out["inliers"] == N_TABLE, (k, out)
        assert mask.all() and mask.dtype == np.uint8 and xyz.dtype == np.float32 and xyz.shape == (N_TABLE, 3)
        wins[int(out["candidate"])] += 1
        worst_rot = max(worst_rot, rot_angle(out["R"].reshape(3, 3), R))
        worst_dir = max(worst_dir, dir_angle(out["t"], t))
        worst_depth = max(worst_depth, float(np.max(np.abs(xyz[:, 2] - z) / z)))
    print(f"pose table: wins {wins}, worst rotation {worst_rot:.3e} deg, baseline {worst_dir:.3e} deg, depth {worst_depth:.3e}")
    assert all(w > 0 for w in wins) and wins == WINS, wins
    assert worst_rot <= 10 * WORST_ROT_DEG and worst_dir <= 10 * WORST_DIR_DEG and worst_depth <= 10 * WORST_DEPTH_REL
    # the table holds what the contract names
    assert (0, 0, 0) in ROTATIONS and (0, 0, 1) in BASELINES and (0, 0, -1) in BASELINES
    assert any(abs(a[2]) >= 170 for a in ROTATIONS) and any(c[3] for c in TABLE)


def test_points_reproject_and_are_in_camera_one_frame(table_runs):
    """xyz is the planted point in the first camera's frame in baseline units: K X projects onto (x1, y1), K (R X + t) onto
    (x2, y2)"""
    for k, (recs, F, K, R, t, z, (out, mask, xyz)) in enumerate(table_runs):
        X = xyz.astype(np.float64)
        p1 = X @ K.T
        p2 = (X @ out["R"].astype(np.float64).reshape(3, 3).T + out["t"].astype(np.float64)) @ K.T
        e1 = np.abs(p1[:, :2] / p1[:, 2:] - recs[:, :2]).max()
        e2 = np.abs(p2[:, :2] / p2[:, 2:] - recs[:, 2:]).max()
        assert e1 < 1e-3 and e2 < 1e-2, (k, e1, e2)                      # pixels; float32 coordinates near 2000 carry 1.2e-4


def test_rotations_are_proper(table_runs):
    worst_o = worst_d = 0.0
    for recs, F, K, R, t, z, (out, _, _) in table_runs:
        Rg = out["R"].astype(np.float64).reshape(3, 3)
        worst_o = max(worst_o, float(np.abs(Rg.T @ Rg - np.eye(3)).max()))
        worst_d = max(worst_d, abs(float(np.linalg.det(Rg)) - 1.0))
        assert abs(float(np.linalg.norm(out["t"].astype(np.float64))) - 1.0) <= 2e-7
        # before the rounding to float32 both candidates are orthonormal to float64 accuracy
        for Rc, _ in pr.candidates(F, pr.intrinsics(K), pr.intrinsics(K))[::2]:
            Rc = np.array(Rc, np.float64).reshape(3, 3)
            assert np.abs(Rc.T @ Rc - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(Rc) - 1.0) <= 1e-14
    print(f"float32 R: worst |R^T R - I| {worst_o:.3e}, worst |det R - 1| {worst_d:.3e}")
    assert worst_o <= 10 * WORST_ORTHO and worst_d <= 10 * WORST_DET


def noisy_case(synth, n, noise, seed):
    n_in = n * 7 // 10
    recs, flags, F, K, R, t, z = synth.two_view_scene(n_in, n - n_in, seed, noise=noise)
    rec0, _ = fr.find_fundamental(recs, 256, 1.0, seed)
    rec1, _ = rr.refine_fundamental(recs, rec0, 1.0, 3)
    return recs, flags, rec1, K, R, t


def test_noisy_chain_ransac_refit_pose(synth):
    worst_rot = worst_dir = 0.0
    for n, noise, seed in NOISY:
        recs, flags, rec1, K, R, t = noisy_case(synth, n, noise, seed)
        out, mask, xyz = pr.recover_pose(recs, rec1, K)
        assert out["candidate"] >= 0 and out["inliers"] == rec1["inliers"] and out["in_front"] == mask.sum()
        assert out["in_front"] >= 0.95 * out["inliers"] and out["inliers"] >= 0.5 * flags.sum(), (n, noise, seed, out)
        a, b = rot_angle(out["R"].reshape(3, 3), R), dir_angle(out["t"], t)
        print(f"noisy n={n} noise={noise} seed={seed}: rotation {a:.4f} deg, baseline {b:.4f} deg, in front {out['in_front']} of "
              f"{out['inliers']}")
        worst_rot, worst_dir = max(worst_rot, a), max(worst_dir, b)
    assert worst_rot <= 2 * NOISY_WORST_ROT_DEG and worst_dir <= 2 * NOISY_WORST_DIR_DEG, (worst_rot, worst_dir)


def test_max_depth_removes_the_far_points(synth):
    """a finite max_depth removes exactly the matches whose planted depth in baseline units, in either camera, exceeds it -- up to
    the margin the recorded depth error leaves around the limit"""
    recs, _, F, K, R, t, z1 = synth.two_view_scene(400, 0, 11, baseline=(-0.5, 0.025, 0.05))     # depths 4..12 -> 8..24 baselines
    X1 = (np.linalg.solve(K, np.concatenate([recs[:, :2].astype(np.float64), np.ones((400, 1))], axis=1).T) * z1).T
    z2 = (X1 @ R.T + t)[:, 2]
    full, fmask, _ = pr.recover_pose(recs, f32_model(F), K)
    assert full["in_front"] == 400
    margin = 10 * WORST_DEPTH_REL
    for md in (16.0, 10.5, 30.0, 8.0):
        out, mask, xyz = pr.recover_pose(recs, f32_model(F), K, max_depth=md)
        near = (z1 < md) & (z2 < md)
        sure = (np.abs(z1 - md) > margin * md) & (np.abs(z2 - md) > margin * md)
        assert sure.sum() >= 398
        assert np.array_equal(mask[sure].astype(bool), near[sure]), md
        assert out["inliers"] == 400 and out["in_front"] == mask.sum() and out["candidate"] == full["candidate"]
        assert not xyz[mask == 0].any() and (xyz[mask == 1, 2] < md).all()
    assert 0 < pr.recover_pose(recs, f32_model(F), K, max_depth=16.0)[0]["in_front"] < 400


def _no_pose(out, mask, xyz, n):
    return (out["candidate"] == -1 and out["inliers"] == 0 and out["in_front"] == 0 and out["n"] == n and not out["t"].any()
            and np.array_equal(out["R"], np.eye(3, dtype=np.float32).reshape(9)) and not mask.any() and not xyz.any()
            and len(mask) == n and xyz.shape == (n, 3))


def test_degenerate_inputs(synth):
    recs, F, K, R, t, z = table_case(synth, 8)
    rec = np.zeros((), fr.FUNDAMENTAL_DTYPE)
    rec["F"], rec["hypothesis"] = F, -1
    assert _no_pose(*pr.recover_pose(recs, rec, K), 200)                # a no-model record with a usable F
    rec["hypothesis"] = 5
    assert pr.recover_pose(recs, rec, K)[0]["candidate"] >= 0
    bad = F.copy()
    bad[4] = np.nan
    assert _no_pose(*pr.recover_pose(recs, bad, K), 200)                # a NaN in F
    bad[4] = np.inf
    assert _no_pose(*pr.recover_pose(recs, bad, K), 200)
    assert _no_pose(*pr.recover_pose(recs, np.zeros(9, np.float32), K), 200)     # an all-zero F: E's largest entry is 0
    rank1 = np.zeros(9, np.float32)
    rank1[0] = 1.0                                                      # a rank-1 E: the second singular value is 0
    assert _no_pose(*pr.recover_pose(recs, rank1, (1.0, 1.0, 0.0, 0.0)), 200)
    nonfinite = recs.copy()
    nonfinite[:, 2] = np.nan
    out, mask, xyz = pr.recover_pose(nonfinite, F, K)                   # only non-finite records: a pose without support
    assert out["candidate"] == 0 and out["inliers"] == 0 and out["in_front"] == 0 and not mask.any() and not xyz.any()
    out, mask, xyz = pr.recover_pose(recs[:0], F, K)
    assert out["candidate"] == 0 and out["n"] == 0 and len(mask) == 0
    # two cameras: the second image scaled by 2 about its principal point is the same pose under K2 = (2 fx, 2 fy, cx, cy)
    two = recs.copy()
    cx, cy = K[0, 2], K[1, 2]
    two[:, 2], two[:, 3] = (recs[:, 2] - cx) * 2 + cx, (recs[:, 3] - cy) * 2 + cy
    S = np.array([[0.5, 0, cx / 2], [0, 0.5, cy / 2], [0, 0, 1.0]])     # image 2' -> image 2
    F2 = S.T @ F.astype(np.float64).reshape(3, 3)
    K2 = (2 * K[0, 0], 2 * K[1, 1], cx, cy)
    o2 = pr.recover_pose(two, f32_model(F2), K, K2)[0]
    assert o2["in_front"] == 200 and rot_angle(o2["R"].reshape(3, 3), R) <= 10 * WORST_ROT_DEG


# ---- the committed cases of test_gpu_pose.py::test_randomised_parity: drawn here so that what they reach can be asserted on the
# statement alone
PARITY_SEED, PARITY_CASES = 2064, 150
PARITY_SCENES = ("general", "sideways", "forward", "rotation", "planar", "lattice")
PARITY_MODELS = ("planted", "ransac", "refit", "random", "rank1", "zero")
PARITY_CAMERAS = ("table", "anisotropic", "outside", "long", "short")
PARITY_DEPTHS = ("inf", "8", "1e-3", "flt_max", "own")
FLT_MAX = float(np.finfo(np.float32).max)
PW, PH, PFOCAL = 1920, 1080, 1500.0


def parity_camera(rng, kind):
    """(fx, fy, cx, cy): the table's camera, fx != fy, a principal point outside the image, the focal length scaled by 2^10 and by
    2^-10"""
    if kind == "anisotropic":
        return (float(rng.uniform(800, 2000)), float(rng.uniform(800, 2000)), PW / 2.0 + 13.0, PH / 2.0 - 7.0)
    if kind == "outside":
        return (PFOCAL, PFOCAL, float((-700.0, PW + 900.0)[int(rng.integers(2))]), float((-400.0, PH + 300.0)[int(rng.integers(2))]))
    if kind == "long":
        return (PFOCAL * 1024.0, PFOCAL * 1024.0, PW / 2.0, PH / 2.0)
    if kind == "short":
        return (PFOCAL / 1024.0, PFOCAL / 1024.0, PW / 2.0, PH / 2.0)
    return (PFOCAL, PFOCAL, PW / 2.0, PH / 2.0)


def _kmat(K):
    return np.array([[K[0], 0.0, K[2]], [0.0, K[1], K[3]], [0.0, 0.0, 1.0]])


def _own_depth(recs, F, K1, K2, threshold, rng):
    """the float32 of one match's own statement depth under the pose the statement takes without a limit (8 when there is none),
    of a depth that the rounding leaves unchanged where the list has one"""
    out, mask, _ = pr.recover_pose(recs, F, K1, K2, threshold, np.inf)
    if out["candidate"] < 0 or not mask.any():
        return 8.0
    R, t = pr.candidates(np.asarray(F, np.float32).reshape(9), pr.intrinsics(K1), pr.intrinsics(K2))[int(out["candidate"])]
    _, z1, z2, _, _ = pr.depths(pr.records(recs), pr.intrinsics(K1), pr.intrinsics(K2), R, t)
    i, which = int(rng.integers(int(mask.sum()))), int(rng.integers(2))
    z = (z1, z2)[which][mask.astype(bool)]
    exact = z[z == z.astype(np.float32)]                                # a depth that IS a float32 (lattice scenes): the limit equals it
    return float(np.float32(exact[i % len(exact)] if len(exact) else z[i]))


def parity_case(k):
    """case k of the randomised pose family run: dict(recs (n, 4) float32, record (FUNDAMENTAL_DTYPE: the model and, for the
    batch call, its hypothesis), K1, K2 (fx, fy, cx, cy), threshold, max_depth, ctx, scene, model, depth, group).  A pure function
    of k.  Cases 8 b .. 8 b + 3 of every third block b of eight share K1 / K2 / threshold / max_depth and also go through
    hak_recover_pose_batch as one ragged group with their records on the device (`group` = b, else -1); a single call takes the
    nine floats and cannot see `hypothesis`.
    Scenes: a general two-view scene; a pure translation sideways (along x or y) and forward (the epipole inside the image), every scene but the lattice with a seventh of its matches at infinity (parallel rays: det == 0 up to
    rounding; under R = I the same pixel in both images, and in the forward scene half of them on the epipole); a nearly pure rotation (a baseline of 1e-4 ..
    1e-7 depths); a planar scene (every scene, four times in ten, with every other point behind both cameras: it is in front under -t);
    integer lattice points seen by K = (1, 1, 0, 0) under integer translations (exact depths, ties).
    Models: the planted F; the statement's own RANSAC record and refit record of the list (hypothesis -1 where it finds none); a
    random full-rank 3 x 3; rank 1; all zero.  Independent axes: F negated, F scaled by 2^{-100, -20, 0, 20, 100}, a NaN / inf entry
    in F, hypothesis set to -1 on a usable F, K1 = K2 or not, the camera variety, max_depth from {inf, 8, 1e-3, FLT_MAX, the
    float32 of one match's own statement depth}, the image order swapped, outliers, NaN rows, duplicates, coordinates (and the
    principal points with them) offset by +-16000."""
    from akaze_hip import synth
    rng = np.random.default_rng([PARITY_SEED, k])
    grp = np.random.default_rng([PARITY_SEED, k // 8, 5])
    pick = lambda seq: seq[int(rng.integers(len(seq)))]
    group = k // 8 if (k // 8) % 3 == 0 and k % 8 < 4 else -1
    n = int(pick((rng.integers(0, 7), 7, 8, rng.integers(9, 301), rng.integers(9, 301), rng.integers(300, 3001),
                  pick((511, 512, 513)), pick((1023, 1024, 1025)))))
    scene = pick(PARITY_SCENES)
    model = pick(PARITY_MODELS[:3] * 3 + PARITY_MODELS[3:])             # the three fitted kinds three times as often
    src = grp if group >= 0 else rng                                    # one pair of cameras, threshold and limit per batch call
    pk = lambda seq: seq[int(src.integers(len(seq)))]
    K1 = parity_camera(src, pk(PARITY_CAMERAS))
    K2 = K1 if src.random() < 0.5 else parity_camera(src, pk(PARITY_CAMERAS))
    threshold = float(np.float32(src.uniform(0.2, 8.0)))
    depth = pk(PARITY_DEPTHS[:2] * 2 + PARITY_DEPTHS[2:] + PARITY_DEPTHS[4:])       # (inf, 8 and the own depth twice as often)
    if scene == "lattice" and group < 0:
        K1 = K2 = (1.0, 1.0, 0.0, 0.0)
        if np.random.default_rng([PARITY_SEED, k, 7]).random() < 0.6:   # exact depths: the limit EQUALS the depth of several matches,
            depth = "own"                                               # which decides both `<` comparisons at equality
    if rng.random() < 0.3 and scene != "lattice" and group < 0:         # both images moved with their principal points
        off = float(pick((-16000.0, 16000.0)))
        K1 = (K1[0], K1[1], K1[2] + off * int(rng.integers(2)), K1[3] + off)
        K2 = (K2[0], K2[1], K2[2] + off, K2[3] + off * int(rng.integers(2)))
    m = max(n, 8)
    if scene == "lattice":                                              # X = (i, j, z) with z a power of two, t an integer vector
        z = 2.0 ** rng.integers(0, 3, m)
        X1 = np.concatenate([rng.integers(-4, 5, (m, 2)) * 1.0, z[:, None]], axis=1)
        R, t = np.eye(3), np.array(pick(((1, 0, 0), (0, 1, 0), (-1, 1, 0), (1, 0, 1), (0, 0, -1))), np.float64)
    else:
        uv = np.stack([rng.uniform(0, PW, m), rng.uniform(0, PH, m)], axis=1)
        ray = np.stack([(uv[:, 0] - PW / 2.0) / PFOCAL, (uv[:, 1] - PH / 2.0) / PFOCAL, np.ones(m)], axis=1)
        X1 = ray * rng.uniform(4.0, 12.0, (m, 1))
        R = synth.rotation_zyx(rng.uniform(-10, 10, 3))
        t = rng.normal(size=3)
        if scene == "sideways":
            R, t = np.eye(3), np.roll(np.array([float(pick((-1.0, 1.0))), rng.uniform(-0.05, 0.05), 0.0]), int(rng.integers(2)))
        elif scene == "forward":
            R, t = np.eye(3), np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.15, 0.15), float(pick((-1.0, 1.0)))])
        elif scene == "rotation":
            t = t / np.linalg.norm(t) * 10.0 ** rng.uniform(-7, -4) * 8.0
        elif scene == "planar":
            nrm = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), 1.0])
            X1 = ray * (8.0 / (ray @ nrm))[:, None]
        if scene in ("general", "planar"):
            t = t / np.linalg.norm(t)
    mirrored = rng.random() < 0.4
    if mirrored:                                                        # every other point behind both cameras: in front under -t at
        X1[1::2] = -X1[0:2 * (m // 2):2]                                # its partner's depths, so two candidates tie at even lengths
    X2 = X1 @ R.T + t
    Km1, Km2 = _kmat(K1), _kmat(K2)
    with np.errstate(all="ignore"):
        p1, p2 = X1 @ Km1.T, X2 @ Km2.T
        recs = np.concatenate([p1[:, :2] / p1[:, 2:], p2[:, :2] / p2[:, 2:]], axis=1)
    tx = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
    Ft = np.linalg.inv(Km2).T @ tx @ R @ np.linalg.inv(Km1)
    if scene != "lattice":
        recs = recs + rng.normal(0, float(pick((0.0, 0.0, 0.3, 1.0))), recs.shape)
    rate = float(rng.uniform(0.0, 0.9)) if rng.random() < 0.6 else 0.0
    out = rng.random(m) < rate
    if mirrored:
        out[1::2] = out[0:2 * (m // 2):2]                               # (partners leave together)
    fin = recs[np.isfinite(recs).all(axis=1)]
    lo, hi = (float(fin.min()), float(fin.max())) if len(fin) else (0.0, 1.0)
    draw = rng.uniform(lo, hi + 1, (int(out.sum()), 4))
    recs[out] = np.floor(draw) if scene == "lattice" else draw
    if scene != "lattice":                       # matches at infinity (under R = I also: on the epipole):
        same = rng.random(m) < 0.15                                     # parallel rays, det == 0 up to rounding
        if scene == "forward":
            ep = (Km1 @ (t / t[2]))[:2]
            recs[same & (rng.random(m) < 0.5), :2] = ep
        far = np.concatenate([(recs[same, :2] - [K1[2], K1[3]]) / [K1[0], K1[1]], np.ones((int(same.sum()), 1))], axis=1) @ R.T @ Km2.T
        with np.errstate(all="ignore"):
            recs[same, 2:] = far[:, :2] / far[:, 2:]
    if rng.random() < 0.3 and group < 0:                                # the image order swapped (a batch has one K1 and one K2)
        recs, Ft, K1, K2 = recs[:, [2, 3, 0, 1]], Ft.T, K2, K1
    recs = np.ascontiguousarray(recs.astype(np.float32)[:n])
    if n and rng.random() < 0.3:                                        # NaN / inf rows
        bad = rng.random(n) < 0.15
        if mirrored:
            bad[1::2] = bad[0:2 * (n // 2):2]
        recs[bad, rng.integers(0, 4, int(bad.sum()))] = np.array([np.nan, np.inf, -np.inf], np.float32)[rng.integers(0, 3, int(bad.sum()))]
    if n and rng.random() < 0.25:                                       # exact duplicates, up to all-equal
        recs[rng.random(n) < float(pick((0.25, 0.6, 1.0)))] = recs[int(rng.integers(n))]
    record = np.zeros((), fr.FUNDAMENTAL_DTYPE)
    record["hypothesis"], record["n"] = 3, n
    if model in ("ransac", "refit"):
        record = fr.find_fundamental(recs, 64, threshold, int(rng.integers(1 << 30)))[0]
        if model == "refit":
            record = rr.refine_fundamental(recs, record, threshold, 2)[0]
    elif model == "planted":
        record["F"] = f32_model(Ft) if np.isfinite(Ft).all() and Ft.any() else 0.0
    elif model == "random":
        record["F"] = f32_model(rng.normal(size=(3, 3)))
    elif model == "rank1":
        record["F"] = np.outer(rng.integers(-2, 3, 3), rng.integers(-2, 3, 3)).reshape(9)
        if rng.random() < 0.5 and group < 0:
            K1 = K2 = (1.0, 1.0, 0.0, 0.0)
    F = record["F"].astype(np.float64)
    if rng.random() < 0.5:                                              # (-E swaps Ra and Rb: candidates 0, 1 <-> 2, 3)
        F = -F
    with np.errstate(all="ignore"):
        F = (F * 2.0 ** int(pick((0,) * 8 + (-100, -20, 20, 100)))).astype(np.float32)
    if rng.random() < 0.06:
        F[int(rng.integers(9))] = (np.nan, np.inf, -np.inf)[int(rng.integers(3))]
    record["F"] = F
    if rng.random() < 0.2:
        record["hypothesis"] = -1                                       # a no-model record with whatever F it holds
    max_depth = {"inf": float("inf"), "8": 8.0, "1e-3": 1e-3, "flt_max": FLT_MAX}.get(depth)
    if max_depth is None and group >= 0 and k % 8:                      # a batch has one limit: its first list's
        max_depth = parity_case(k - k % 8)["max_depth"]
    elif max_depth is None:
        max_depth = _own_depth(recs, F, K1, K2, threshold, np.random.default_rng([PARITY_SEED, k, 6]))
    return dict(recs=recs, record=record, K1=K1, K2=K2, threshold=threshold, max_depth=max_depth, ctx=bool(rng.integers(2)),
                scene=scene, model=model, depth=depth, group=group)


def parity_trace(c, batch=False):
    """what the statement does on case c, step by step with pose_ref's own functions.  batch: with the record (hypothesis seen), as
    hak_recover_pose_batch takes it; else with the nine floats.  dict(cause in {"pose", "hypothesis", "non-finite", "d == 0",
    "l1 / l2"}, candidate, j3, counts (the four candidates' in-front counts), inliers, in_front, by_det, by_depth (inliers of F that
    det <= 0, and the depth limit alone, keep out of the winner's mask), at_limit (of the latter, those with z1 or z2 EQUAL to the
    limit))"""
    F = c["record"]["F"]
    out, mask, xyz = pr.recover_pose(c["recs"], c["record"] if batch else F, c["K1"], c["K2"], c["threshold"], c["max_depth"])
    tr = dict(cause="pose", candidate=int(out["candidate"]), j3=-1, counts=None, inliers=int(out["inliers"]),
              in_front=int(out["in_front"]), by_det=0, by_depth=0, at_limit=0)
    K1, K2 = pr.intrinsics(c["K1"]), pr.intrinsics(c["K2"])
    if batch and c["record"]["hypothesis"] < 0:
        tr["cause"] = "hypothesis"
    elif not np.isfinite(F).all():
        tr["cause"] = "non-finite"
    else:
        E, ok = pr.essential(F, K1, K2)
        if not ok:
            tr["cause"] = "d == 0"
        elif not pr.decompose(E)[3]:
            tr["cause"] = "l1 / l2"
    assert (tr["cause"] == "pose") == (out["candidate"] >= 0)
    if tr["cause"] != "pose":
        return tr
    with np.errstate(all="ignore"):
        G = np.array([[(E[i] * E[j] + E[3 + i] * E[3 + j]) + E[6 + i] * E[6 + j] for j in range(3)] for i in range(3)])
        A = rr.jacobi(G, 3, rr.SWEEPS3)[1]
    tr["j3"] = int(np.argmin([A[0, 0], A[1, 1], A[2, 2]]))              # (the first of equal minima, as the rule's strict <)
    rec = pr.records(c["recs"])
    inl = pr.inlier_mask(F, rec, np.float32(c["threshold"]) * np.float32(c["threshold"]))[0]
    cands = pr.candidates(F, K1, K2)
    tr["counts"] = [int((inl & pr.front_mask(rec, K1, K2, R, t, c["max_depth"])).sum()) for R, t in cands]
    assert tr["counts"][tr["candidate"]] == max(tr["counts"]) == tr["in_front"] and inl.sum() == tr["inliers"]
    R, t = cands[tr["candidate"]]
    det, z1, z2, _, _ = pr.depths(rec, K1, K2, R, t)
    with np.errstate(all="ignore"):
        tr["by_det"] = int((inl & ~(det > 0.0)).sum())
        cut = inl & pr.front_mask(rec, K1, K2, R, t, np.inf) & ~mask.astype(bool)
        md = np.float64(np.float32(c["max_depth"]))
        tr["by_depth"], tr["at_limit"] = int(cut.sum()), int((cut & ((z1 == md) | (z2 == md))).sum())
    return tr


@pytest.fixture(scope="module")
def parity_traces():
    cases = [parity_case(k) for k in range(PARITY_CASES)]
    return cases, [parity_trace(c) for c in cases], [parity_trace(c, True) for c in cases if c["group"] >= 0]


def test_parity_cases_are_pure_and_cover_the_axes(parity_traces):
    a, b = parity_case(5), parity_case(5)
    assert a["recs"].tobytes() == b["recs"].tobytes() and a["record"].tobytes() == b["record"].tobytes()
    assert {f: a[f] for f in a if f not in ("recs", "record")} == {f: b[f] for f in b if f not in ("recs", "record")}
    cases = parity_traces[0]
    assert {c["scene"] for c in cases} == set(PARITY_SCENES) and {c["model"] for c in cases} == set(PARITY_MODELS)
    assert {c["depth"] for c in cases} == set(PARITY_DEPTHS)
    sizes = {len(c["recs"]) for c in cases}
    assert {0, 1, 2, 3, 4, 5, 6, 7, 8} <= sizes and sizes & {511, 512, 513} and sizes & {1023, 1024, 1025} and max(sizes) > 1025
    assert sum(c["K1"] != c["K2"] for c in cases) >= 20 and sum(c["K1"] == c["K2"] for c in cases) >= 20
    assert sum(c["K1"] == (1.0, 1.0, 0.0, 0.0) for c in cases) >= 5
    assert sum(abs(c["K1"][3]) > 10000 for c in cases) >= 10             # coordinates offset by +-16000
    expo = {int(np.round(np.log2(np.abs(c["record"]["F"][np.isfinite(c["record"]["F"])]).max()))) // 10 for c in cases
            if np.isfinite(c["record"]["F"]).any() and c["record"]["F"][np.isfinite(c["record"]["F"])].any() and c["model"] == "planted"}
    assert {-10, -2, 0, 2, 10} <= expo, expo                            # the planted F (largest entry 1) scaled by 2^-100 .. 2^100
    groups = sorted({c["group"] for c in cases if c["group"] >= 0})
    assert len(groups) >= 5
    for g in groups:
        ks = [c for c in cases if c["group"] == g]
        assert len(ks) == 4 and len({(c["K1"], c["K2"], c["threshold"], c["depth"]) for c in ks}) == 1
        assert len({c["max_depth"] for c in ks}) == 1
    assert sum(not np.isfinite(c["recs"]).all() for c in cases) >= 10


def test_parity_cases_reach_the_rare_branches(parity_traces):
    """what the statement alone says about the committed cases; conditions on the inputs, not measurements of the kernel.  Counted
    when written (150 single calls, 28 of them again with their records in a batch): candidates 0 .. 3 win 58 / 14 / 14 / 15 cases
    (34 of candidate 0's with nothing in front of any candidate); two candidates tie on a largest count above zero in 7; j3 = 0 / 1
    / 2 in 38 / 29 / 34; no pose for a non-finite F 18 times, d == 0 30, the l1 / l2 test 5, hypothesis < 0 8 (batch only: a single
    call cannot see it); 0 < in_front < inliers in 55 cases, a pose with in_front == 0 in 34 (7 of them with inliers); det <= 0
    removes an inlier in 12, the depth limit in 28, in 5 of them at a depth EQUAL to the limit.  Positive ties are rare -- they
    come from the lists whose points are mirrored pairwise -- and PARITY_SEED is one of the two seeds of 2061 .. 2074 that were found to meet
    every bound at once."""
    cases, single, batch = parity_traces
    posed = [t for t in single if t["cause"] == "pose"]
    wins = [sum(t["candidate"] == c for t in posed) for c in range(4)]
    ties = sum(sorted(t["counts"])[-1] == sorted(t["counts"])[-2] > 0 for t in posed)
    ties0 = sum(max(t["counts"]) == 0 for t in posed)
    j3 = [sum(t["j3"] == j for t in posed) for j in range(3)]
    causes = {}
    for t in single + batch:
        causes[t["cause"]] = causes.get(t["cause"], 0) + 1
    got = dict(wins=wins, ties=ties, ties_at_zero=ties0, j3=j3, causes=causes,
               partly_front=sum(0 < t["in_front"] < t["inliers"] for t in posed),
               none_front=sum(t["in_front"] == 0 for t in posed), none_front_with_inliers=sum(t["in_front"] == 0 < t["inliers"] for t in posed),
               by_det=sum(t["by_det"] > 0 for t in posed), by_depth=sum(t["by_depth"] > 0 for t in posed),
               at_limit=sum(t["at_limit"] > 0 for t in posed))
    print("pose parity cases:", got)
    assert min(wins) >= 10 and ties >= 5 and min(j3) >= 5, got
    assert all(causes.get(c, 0) >= 3 for c in ("non-finite", "d == 0", "l1 / l2", "hypothesis")), got
    assert got["partly_front"] >= 10 and got["none_front"] >= 5 and got["by_det"] >= 10 and got["by_depth"] >= 10, got
    assert got["at_limit"] >= 3, got                                    # a depth equal to the limit is out: `<`, not `<=`


def test_entry_points_refuse_bad_arguments_without_a_device(ah):
    """the refusals come before any device is touched, so they hold on a machine without one"""
    lib = ah.lib
    assert ah.POSE_DTYPE.itemsize == 64 and ah.INTRINSICS_DTYPE.itemsize == 16
    assert ah.POSE_DTYPE == pr.POSE_DTYPE and ah.INTRINSICS_DTYPE == pr.INTRINSICS_DTYPE
    out = np.zeros((), ah.POSE_DTYPE)
    F = np.zeros(9, np.float32)
    F[5], F[7] = -1.0, 1.0
    K = ah.intrinsics((1500.0, 1500.0, 960.0, 540.0))
    fp, kp, op = F.ctypes.data_as(C.POINTER(C.c_float)), K.ctypes.data, out.ctypes.data
    inf, nan = float("inf"), float("nan")

    def k_with(**kw):
        b = K.copy()
        for f, v in kw.items():
            b[f] = v
        return b

    bad_k = [k_with(fx=0.0), k_with(fy=0.0), k_with(fx=nan), k_with(fy=inf), k_with(cx=nan), k_with(cy=-inf)]
    one = lib.hak_recover_pose
    refused = [(None, 16, 4, fp, kp, kp, thr, inf, None, None, op) for thr in (0.0, -1.0, nan, inf)]
    refused += [(None, 16, 4, fp, kp, kp, 1.0, md, None, None, op) for md in (0.0, -2.0, nan)]
    refused += [(None, 16, 4, fp, b.ctypes.data, kp, 1.0, inf, None, None, op) for b in bad_k]
    refused += [(None, 16, 4, fp, kp, b.ctypes.data, 1.0, inf, None, None, op) for b in bad_k]
    refused += [(None, 16, 4, None, kp, kp, 1.0, inf, None, None, op), (None, 16, 4, fp, None, kp, 1.0, inf, None, None, op),
                (None, 16, 4, fp, kp, None, 1.0, inf, None, None, op), (None, 16, 4, fp, kp, kp, 1.0, inf, None, None, None),
                (None, 16, -1, fp, kp, kp, 1.0, inf, None, None, op), (None, None, 4, fp, kp, kp, 1.0, inf, None, None, op),
                (None, 20, 4, fp, kp, kp, 1.0, inf, None, None, op)]
    for args in refused:
        assert one(*args) != 0, args
        assert lib.hak_last_error().decode() != ""
    batch = lib.hak_recover_pose_batch
    assert batch(None, 16, 64, 16, 1, 16, kp, kp, 1.0, inf, 16, None, None) != 0      # no context
    assert "argument" in lib.hak_last_error().decode()
    assert not out.tobytes().strip(b"\0")                               # nothing was written through a refused call's pointer
