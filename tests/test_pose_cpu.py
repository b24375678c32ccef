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
