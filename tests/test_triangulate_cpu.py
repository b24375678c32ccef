"""CPU suite: triangulation under two known views (hak_triangulate).  The numpy statement of the contract
(tests/triangulate_ref.py, the checker of the GPU tests) is held against planted scenes: exact recovery over the pose table of
test_pnp_cpu.py, every gate and every no-model case from the record's counts, and the noisy chain fundamental -> refit -> pose ->
link -> PnP -> refit -> triangulation -> link -> PnP -> refit over four views; the entry points are exported and refuse bad
arguments without a device."""
import ctypes as C

import numpy as np
import pytest

import fundamental_ref as fr
import fundamental_refit_ref as rr
import link_ref as lr
import pnp_ref as pn
import pnp_refit_ref as pf
import pose_ref as pr
import triangulate_ref as tr
from test_pnp_cpu import BEHIND, FOCAL, H, K_TABLE, TABLE, W
from test_pose_cpu import dir_angle, rot_angle

N_EXACT, THR_EXACT = 200, 0.5
# the four-view legs of the accuracy table: (points, noise px, seed), 30 % wrong matches in each list; the last only prints
LEGS = [(400, 0.3, 1), (400, 0.5, 2), (400, 0.5, 3), (1000, 0.5, 5), (400, 1.0, 4)]
ASSERTED_LEGS = 4


@pytest.fixture(scope="module")
def synth(ah):
    from akaze_hip import synth
    return synth


def match_array(p1, p2):
    m = np.zeros(len(p1), np.dtype([("query", "<i4"), ("train", "<i4"), ("distance", "<i4"), ("second", "<i4"),
                                    ("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4")]))
    m["query"] = m["train"] = np.arange(len(p1))
    m["distance"], m["second"] = 20, 60
    with np.errstate(all="ignore"):
        (m["x1"], m["y1"]), (m["x2"], m["y2"]) = np.asarray(p1, np.float64).T, np.asarray(p2, np.float64).T
    return m


def rt12(R, t):
    """twelve float32 {R row-major, t}"""
    return np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)]).astype(np.float32)


def project(X, R, t):
    """(pixels (n, 2), depth (n,)) of world points under the view Xc = R X + t and K_TABLE, float64"""
    Xc = X @ np.asarray(R, np.float64).T + t
    with np.errstate(all="ignore"):
        return np.stack([FOCAL * Xc[:, 0] / Xc[:, 2] + W / 2.0, FOCAL * Xc[:, 1] / Xc[:, 2] + H / 2.0], axis=1), Xc[:, 2]


def exact_case(synth, kb, ka):
    """table entry kb as view B, entry ka (None: the identity) as view A -> (matches rounded to float32, MA, MB, world points X,
    depths zA, zB, pixels pA, pB).  The points are drawn in B's frustum at depths 4 .. 12, as test_pnp_cpu.table_case draws them;
    with kb == BEHIND every third is mirrored through B's centre: it projects onto the same pixel from behind the camera.  The
    views are the table's rounded to float32, and the points are projected under those, so nothing but the pixels' rounding
    separates the matches from the planted scene"""
    rng = np.random.default_rng(5000 + 100 * kb + (0 if ka is None else ka + 1))
    MB = rt12(synth.rotation_zyx(TABLE[kb][0]), TABLE[kb][1])
    MA = rt12(np.eye(3), np.zeros(3)) if ka is None else rt12(synth.rotation_zyx(TABLE[ka][0]), TABLE[ka][1])
    RA, tA, RB, tB = (M.astype(np.float64) for M in (MA[:9].reshape(3, 3), MA[9:], MB[:9].reshape(3, 3), MB[9:]))
    z = rng.uniform(4.0, 12.0, N_EXACT)
    uv = np.stack([rng.uniform(0, W, N_EXACT), rng.uniform(0, H, N_EXACT)], axis=1)
    Xc = np.stack([(uv[:, 0] - W / 2.0) / FOCAL * z, (uv[:, 1] - H / 2.0) / FOCAL * z, z], axis=1)
    if kb == BEHIND:
        Xc[::3] = -Xc[::3]
    X = np.linalg.solve(RB, (Xc - tB).T).T
    (pA, zA), (pB, zB) = project(X, RA, tA), project(X, RB, tB)
    return match_array(pA, pB), MA, MB, X, zA, zB, pA, pB


def point_bound(X, MA, MB, zA, zB, pA, pB):
    """|P - X| allowed per point, from the rounding of the pixels to float32 alone.
    A pixel coordinate p is stored with an error of at most ulp32(p) / 2, so a pixel moves by at most
    d = sqrt(ulp(x)^2 + ulp(y)^2) / 2.  The bearing (x, y, 1) then moves by at most d / f in its plane; seen from the camera
    centre that turns the ray by an angle of at most (d / f) / |(x, y, 1)|, and at the point, which lies |(x, y, 1)| z from the
    centre, the ray passes within e = z d / f of it.  Two lines with unit directions u, v at an angle th that pass within eA and eB
    of X: with qA, qB their points closest to X and g = qB - qA (|g| <= eA + eB), the ends of the common perpendicular are
    qA + s u and qB + t v with s = g . (u - v cos th) / sin^2 th, and |u - v cos th| = sin th, so |s|, |t| <= |g| / sin th.  Either
    end is therefore within (eA + eB) (1 + 1 / sin th) <= 2 (eA + eB) / sin th of X, and so is their midpoint.  The angle between
    the rounded rays differs from th by at most (eA / rA + eB / rB), under 1e-6 of it for the points the bound is used on
    (sin th >= 1e-3); the factor 2.02 covers it.  Rounding P to float32 adds at most sqrt(3) ulp32(max |P_j|) / 2.  The float64
    solve itself adds errors of the order of 2^-52 / sin^2 th of the depth, which the last term (1e-9 of the depth) covers for
    sin th >= 1e-3."""
    cA = -MA[:9].reshape(3, 3).astype(np.float64).T @ MA[9:].astype(np.float64)
    cB = -MB[:9].reshape(3, 3).astype(np.float64).T @ MB[9:].astype(np.float64)
    u, v = X - cA, X - cB
    ru, rv = np.linalg.norm(u, axis=1), np.linalg.norm(v, axis=1)
    sin_th = np.linalg.norm(np.cross(u, v), axis=1) / (ru * rv)

    def e(p, z):
        ulp = np.spacing(np.abs(p).astype(np.float32)).astype(np.float64)
        return np.abs(z) * 0.5 * np.sqrt((ulp ** 2).sum(axis=1)) / FOCAL

    rounding = np.sqrt(3.0) * 0.5 * np.spacing(np.abs(X).max(axis=1).astype(np.float32) * np.float32(1.01)).astype(np.float64)
    return 2.02 * (e(pA, zA) + e(pB, zB)) / sin_th + rounding + 1e-9 * np.maximum(ru, rv), sin_th


def test_exact_recovery_over_the_pose_table(synth):
    assert len(TABLE) == 42
    worst = worst_ratio = 0.0
    kept_total = zero_baseline = both_front = 0
    for kb in range(len(TABLE)):
        for ka in (None, (kb + 17) % len(TABLE)):
            m, MA, MB, X, zA, zB, pA, pB = exact_case(synth, kb, ka)
            out, mask, xyz = tr.triangulate(m, MA, MB, K_TABLE, None, THR_EXACT)
            _, gate, _ = tr.gates(m, MA, MB, K_TABLE, None, THR_EXACT)
            assert out["model"] == 1 and out["n"] == N_EXACT and out["kept"] == mask.sum() and out["kept"] + out["rejected"].sum() == N_EXACT
            front = (zA > 0) & (zB > 0)
            _, cA = tr.centre(MA)
            _, cB = tr.centre(MB)
            if cA == cB:                                                # no baseline: every ray pair meets at the shared centre,
                zero_baseline += 1                                      # depth 0, or is parallel
                assert out["kept"] == 0 and out["rejected"][2] == 0, (kb, ka, out)
                continue
            # every point in front of both cameras is kept, every other is rejected, by the depth gate
            assert np.array_equal(mask.astype(bool), front), (kb, ka, int((mask.astype(bool) != front).sum()))
            assert (gate[~front] == 1).all() and out["rejected"][1] == (~front).sum() and out["rejected"][0] == out["rejected"][2] == 0
            if kb == BEHIND:
                assert not front[::3].any() and (gate[::3] == 1).all()  # the mirrored points
            both_front += int(front.any())
            kept_total += int(front.sum())
            bound, sin_th = point_bound(X, MA, MB, zA, zB, pA, pB)
            err = np.linalg.norm(xyz.astype(np.float64) - X, axis=1)
            use = front & (sin_th >= 1e-3)
            assert (err[use] <= bound[use]).all(), (kb, ka, float((err[use] / bound[use]).max()))
            assert not (xyz[~front] != 0).any()
            if use.any():
                worst, worst_ratio = max(worst, float(err[use].max())), max(worst_ratio, float((err[use] / bound[use]).max()))
    print(f"triangulation table: {kept_total} points kept over {both_front} view pairs with points in front of both, worst |P - X| "
          f"{worst:.3e} scene units, at most {worst_ratio:.3f} of the pixel-rounding bound; {zero_baseline} pairs without a baseline")
    assert kept_total > 3000 and both_front >= 20 and zero_baseline >= 1


# ---- the gate and no-model family, shared with test_gpu_triangulate.py: (name, matches, view A, view B, parameters, expected)
B_SIDE = rt12(np.eye(3), (-1.0, 0.0, 0.0))                              # the second camera one unit to the right of the first


def _pose_record(M, candidate=0):
    r = np.zeros((), pr.POSE_DTYPE)
    r["R"], r["t"], r["candidate"], r["inliers"], r["in_front"], r["n"] = M[:9], M[9:], candidate, 5, 4, 9
    return r


def _abs_record(M, hypothesis=0):
    r = np.zeros((), pn.ABS_POSE_DTYPE)
    r["R"], r["t"], r["hypothesis"], r["inliers"], r["solution"], r["n"] = M[:9], M[9:], hypothesis, 5, 4, 9
    return r


def side_matches(X):
    """world points seen by the identity view and by B_SIDE"""
    X = np.asarray(X, np.float64).reshape(-1, 3)
    return match_array(project(X, np.eye(3), np.zeros(3))[0], project(X, np.eye(3), B_SIDE[9:].astype(np.float64))[0])


def gate_cases():
    """every case as dict(name, matches, A, B, par = (threshold, max_depth, min_sin), kept, rejected, model); a pure function"""
    rng = np.random.default_rng(77)
    cloud = np.stack([rng.uniform(-3, 3, 40), rng.uniform(-2, 2, 40), rng.uniform(4, 12, 40)], axis=1)
    good = side_matches(cloud)
    cases = []

    def add(name, m, A, B, par, kept, rejected, model=1):
        cases.append(dict(name=name, matches=m, A=A, B=B, par=par, kept=kept, rejected=None if rejected is None else list(rejected),
                          model=model))

    add("planted", good, None, B_SIDE, (0.5, np.inf, 0.0), 40, (0, 0, 0))
    par = good.copy()
    par["x2"], par["y2"] = par["x1"], par["y1"]                          # the same bearing under R = I: det == 0 exactly
    add("parallel rays", par, None, B_SIDE, (0.5, np.inf, 0.0), 0, (40, 0, 0))
    # the rays to (0.5, 0, Z) from centres one unit apart meet at an angle of 2 atan(0.5 / Z): its sine at Z = 10.05 separates
    # Z = 10 (kept) from Z = 10.1 (below min_sin) with a margin of 5e-3 of it
    min_sin = float(np.sin(2.0 * np.arctan(0.5 / 10.05)))
    add("min_sin", side_matches([(0.5, 0, 10.0), (0.5, 0, 10.1)]), None, B_SIDE, (0.5, np.inf, min_sin), 1, (1, 0, 0))
    # (0, 0, 4): x1 = cx, x2 = cx - 1500 / 4 = 585 exactly, so a = (0, 0, 1), b = (-0.25, 0, 1), det = 0.0625 and z1 = z2 = 4 exactly
    on_axis = side_matches([(0.0, 0.0, 4.0)])
    add("depth == max_depth", on_axis, None, B_SIDE, (0.5, 4.0, 0.0), 0, (0, 1, 0))
    add("depth just below max_depth", on_axis, None, B_SIDE, (0.5, float(np.nextafter(np.float32(4.0), np.float32(5.0))), 0.0), 1, (0, 0, 0))
    wrong = good.copy()
    wrong["y2"][::2] += 50.0                                            # skew rays: in front, 25 px from either observation
    add("wrong matches", wrong, None, B_SIDE, (2.0, np.inf, 0.0), 20, (0, 0, 20))
    for f, bad in (("x1", np.nan), ("y1", np.inf), ("x2", -np.inf), ("y2", np.nan)):
        nf = good.copy()
        nf[f][::4] = bad
        add("non-finite " + f, nf, None, B_SIDE, (0.5, np.inf, 0.0), 30, (10, 0, 0))
    add("two identity views", good, None, None, (0.5, np.inf, 0.0), 0, None)
    add("n = 0", good[:0], None, B_SIDE, (0.5, np.inf, 0.0), 0, (0, 0, 0))
    add("pose record", good, None, _pose_record(B_SIDE, 2), (0.5, np.inf, 0.0), 40, (0, 0, 0))
    add("abs record", good, _abs_record(rt12(np.eye(3), np.zeros(3))), _abs_record(B_SIDE), (0.5, np.inf, 0.0), 40, (0, 0, 0))
    add("no pose, B", good, None, _pose_record(B_SIDE, -1), (0.5, np.inf, 0.0), 0, (0, 0, 0), 0)
    add("no pose, A", good, _pose_record(B_SIDE, -1), None, (0.5, np.inf, 0.0), 0, (0, 0, 0), 0)
    add("no abs pose, B", good, None, _abs_record(B_SIDE, -1), (0.5, np.inf, 0.0), 0, (0, 0, 0), 0)
    add("no abs pose, A", good, _abs_record(B_SIDE, -1), B_SIDE, (0.5, np.inf, 0.0), 0, (0, 0, 0), 0)
    for k, bad in ((4, np.nan), (0, np.inf), (10, -np.inf)):
        M = B_SIDE.copy()
        M[k] = bad
        add(f"non-finite view entry {k}", good, None, _abs_record(M), (0.5, np.inf, 0.0), 0, (0, 0, 0), 0)
        add(f"non-finite pose entry {k}", good, _pose_record(M), B_SIDE, (0.5, np.inf, 0.0), 0, (0, 0, 0), 0)
    return cases


def test_every_gate_from_the_counts():
    names = set()
    for c in gate_cases():
        out, mask, xyz = tr.triangulate(c["matches"], c["A"], c["B"], K_TABLE, None, *c["par"])
        n = len(c["matches"])
        names.add(c["name"])
        assert out["n"] == n and out["model"] == c["model"] and out["kept"] == c["kept"] == mask.sum() and not out["pad"].any(), (c["name"], out)
        assert len(mask) == n and xyz.shape == (n, 3) and xyz.dtype == np.float32 and mask.dtype == np.uint8
        if c["rejected"] is not None:
            assert out["rejected"].tolist() == c["rejected"], (c["name"], out)
        if c["model"]:
            assert out["kept"] + out["rejected"].sum() == n
        else:
            assert not mask.any() and not xyz.any() and not out["rejected"].any()
        assert not xyz[mask == 0].any() and np.isfinite(xyz).all()
    assert {"parallel rays", "min_sin", "depth == max_depth", "wrong matches", "two identity views", "n = 0", "no pose, B"} <= names
    by = {c["name"]: c for c in gate_cases()}
    out, mask, _ = tr.triangulate(by["min_sin"]["matches"], None, B_SIDE, K_TABLE, None, *by["min_sin"]["par"])
    assert mask.tolist() == [1, 0]                                      # the nearer point has the larger angle
    out, mask, _ = tr.triangulate(by["wrong matches"]["matches"], None, B_SIDE, K_TABLE, None, 2.0)
    assert not mask[::2].any() and mask[1::2].all()
    for f in ("x1", "y1", "x2", "y2"):
        _, mask, _ = tr.triangulate(by["non-finite " + f]["matches"], None, B_SIDE, K_TABLE, None, 0.5)
        assert not mask[::4].any() and mask[np.arange(40) % 4 != 0].all()
    out, _, _ = tr.triangulate(by["planted"]["matches"], None, None, K_TABLE)
    assert out["rejected"][2] == 0 and out["rejected"][:2].sum() == 40   # w = 0: parallel or at depth 0, never a point


def test_purity_and_symmetry(synth):
    m, MA, MB, *_ = exact_case(synth, 11, 30)
    rng = np.random.default_rng(4)
    m["y2"][::5] += rng.uniform(-3, 3, len(m["y2"][::5])).astype(np.float32)       # some matches near the reprojection gate
    a = tr.triangulate(m, MA, MB, K_TABLE, None, 1.0, 40.0, 0.01)
    b = tr.triangulate(m.copy(), MA.copy(), MB.copy(), K_TABLE, None, 1.0, 40.0, 0.01)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    sw = m.copy()
    sw["x1"], sw["y1"], sw["x2"], sw["y2"] = m["x2"], m["y2"], m["x1"], m["y1"]
    c = tr.triangulate(sw, MB, MA, K_TABLE, None, 1.0, 40.0, 0.01)
    assert np.array_equal(a[1], c[1]) and 0 < a[0]["kept"] < len(m) and a[0]["rejected"][2] > 0


def chain(synth, n, noise, seed, ransac_seed=None, max_index=None):
    """the statement chain over one four_view_scene -> dict of every stage's outputs (the RANSAC stages take the scene's seed
    and the links 2 n keypoints per image unless told otherwise)"""
    sc = synth.four_view_scene(seed, n, noise, 0.3)
    K, A, B, Cl = sc[0], sc[3], sc[4], sc[11]
    seed = seed if ransac_seed is None else ransac_seed
    max_index = 2 * n if max_index is None else max_index
    rec0, _ = fr.find_fundamental(A, 256, 1.0, seed)
    rec1, _ = rr.refine_fundamental(A, rec0, 1.0, 3)
    pose, pmask, xyz = pr.recover_pose(A, rec1, K, None, 1.0, 50.0)
    corr2 = lr.link_tracks(A, pmask, xyz, B, max_index)
    abs2, _ = pn.solve_pnp(corr2, K, 256, 2.0, seed)
    ref2, mask2 = pf.refine_pnp(corr2, K, abs2, 2.0, 3)
    tri, tmask, txyz = tr.triangulate(B, pose, ref2, K, None, 2.0, 50.0, 0.01)
    corr3 = lr.link_tracks(B, tmask, txyz, Cl, max_index)
    abs3, _ = pn.solve_pnp(corr3, K, 256, 2.0, seed)
    ref3, mask3 = pf.refine_pnp(corr3, K, abs3, 2.0, 3)
    return dict(scene=sc, fund=rec1, pose=pose, pmask=pmask, xyz=xyz, corr2=corr2, abs2=abs2, ref2=ref2, mask2=mask2, tri=tri, tmask=tmask,
                txyz=txyz, corr3=corr3, abs3=abs3, ref3=ref3, mask3=mask3)


def test_noisy_chain_over_four_views(synth):
    """the chain of the accuracy table (README.md) on every leg; a line per leg is printed.  The statement's figures when written,
    legs in LEGS' order -- kept / planted-correct matches of list B, wrong kept, |t3| got / planted: 280 / 280, 0, 2.719 / 2.722;
    280 / 280, 0, 2.730 / 2.722; 280 / 280, 0, 2.716 / 2.722; 702 / 700, 2, 2.724 / 2.722; and on the 1 px leg, which only prints,
    176 / 280, 0, 2.713 / 2.722.  The conditions below are the feature's, not these measurements: a statement that misses them is
    wrong"""
    for leg, (n, noise, seed) in enumerate(LEGS):
        c = chain(synth, n, noise, seed)
        (R01, t01), (R12, t12), fb, (R23, t23) = c["scene"][1], c["scene"][2], c["scene"][6], c["scene"][10]
        scale = np.linalg.norm(t01)                                     # the chain's unit is the first pair's baseline
        R02, t02 = R12 @ R01, R12 @ t01 + t12
        R03, t03 = R23 @ R02, R23 @ t02 + t23
        kept = c["tmask"] == 1
        t3 = float(np.linalg.norm(c["ref3"]["t"]))
        want_t3 = float(np.linalg.norm(t03) / scale)
        print(f"four views n={n} noise={noise} seed={seed}: kept {kept.sum()} / {fb.sum()} planted-correct in B, wrong kept "
              f"{(kept & ~fb).sum()}, rejected {c['tri']['rejected'].tolist()}, linked {len(c['corr3'])}, inliers for I3 "
              f"{c['ref3']['inliers']} (I2: {c['ref2']['inliers']}); I2 rot / t-dir "
              f"{rot_angle(c['ref2']['R'].reshape(3, 3), R02):.3f} / {dir_angle(c['ref2']['t'], t02):.3f} deg, I3 "
              f"{rot_angle(c['ref3']['R'].reshape(3, 3), R03):.3f} / {dir_angle(c['ref3']['t'], t03):.3f} deg, "
              f"|t3| {t3:.3f} / {want_t3:.3f}")
        if leg >= ASSERTED_LEGS:
            continue
        assert c["tri"]["model"] == 1 and c["ref3"]["hypothesis"] >= 0, (n, noise, seed)
        assert fb[kept].mean() >= 0.95, (n, noise, seed, float(fb[kept].mean()))
        assert (kept & fb).sum() >= 0.9 * fb.sum(), (n, noise, seed, int((kept & fb).sum()), int(fb.sum()))
        assert abs(t3 - want_t3) <= 0.02 * want_t3, (n, noise, seed, t3, want_t3)


# ------------------------------------------------------------------------------------------------------------- host side
def refusals(ah, ctx, p, cntp):
    """every refused call of the two entry points as (function, arguments, a word of the message): p a valid 16-byte aligned
    pointer (device memory on a machine with one), cntp a valid int pointer; ctx a context or None.  The batch form looks at its
    context last, so without one every other refusal still shows by its own message"""
    lib = ah.lib
    K = ah.intrinsics(K_TABLE)
    keep = [K]

    def k_with(**kw):
        b = K.copy()
        for f, v in kw.items():
            b[f] = v
        keep.append(b)
        return b.ctypes.data

    def view(k=None, v=0.0):
        m = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, -1, 0, 0], np.float32)
        if k is not None:
            m[k] = v
        keep.append(m)
        return m.ctypes.data_as(C.POINTER(C.c_float))

    inf, nan = float("inf"), float("nan")
    kp = K.ctypes.data
    rec = np.zeros((), ah.TRIANGULATION_DTYPE)
    keep.append(rec)
    op = rec.ctypes.data
    one, bat = lib.hak_triangulate, lib.hak_triangulate_batch
    bad_k = [k_with(fx=0.0), k_with(fy=0.0), k_with(fx=nan), k_with(fy=inf), k_with(cx=nan), k_with(cy=-inf)]
    good1 = [None, p, 8, None, view(), kp, kp, 1.0, 50.0, 0.0, None, None, op]
    good2 = [ctx, p, 64, cntp, 1, 1, None, 0, 0, p, 2, 1, kp, kp, 1.0, 50.0, 0.0, p, None, None]

    def vary(fn, good, changes):
        out = []
        for pos, val, word in changes:
            args = list(good)
            args[pos] = val
            out.append((fn, tuple(args), word))
        return out

    out = vary(one, good1, [(7, 0.0, "threshold"), (7, -1.0, "threshold"), (7, nan, "threshold"), (7, inf, "threshold"),
                            (8, 0.0, "max_depth"), (8, -2.0, "max_depth"), (8, nan, "max_depth"),
                            (9, -0.1, "min_sin"), (9, 1.0, "min_sin"), (9, 1.5, "min_sin"), (9, nan, "min_sin"),
                            (5, None, "intrinsics"), (6, None, "intrinsics"), (12, None, "null"),
                            (2, -1, "n < 0"), (1, None, "null"), (1, p + 4, "aligned"),
                            (3, view(3, nan), "non-finite"), (4, view(11, inf), "non-finite"), (4, view(0, -inf), "non-finite")])
    out += vary(one, good1, [(5, b, "f") for b in bad_k[:4]] + [(6, b, "c") for b in bad_k[4:]])
    out += vary(bat, good2, [(14, 0.0, "threshold"), (14, nan, "threshold"), (15, 0.0, "max_depth"), (15, nan, "max_depth"),
                             (16, -0.5, "min_sin"), (16, 1.0, "min_sin"), (16, nan, "min_sin"),
                             (7, 3, "kind"), (7, -1, "kind"), (10, 3, "kind"), (10, -1, "kind"),
                             (9, None, "null view"), (7, 1, "null view"), (7, 2, "null view"),
                             (8, -1, "view step"), (11, -1, "view step"), (4, 0, "count step"), (4, -2, "count step"),
                             (12, None, "intrinsics"), (13, None, "intrinsics"), (12, bad_k[0], "fx"), (13, bad_k[5], "cy"),
                             (17, None, "null"), (3, None, "null"), (1, None, "null"), (1, p + 8, "aligned"),
                             (5, 0, "npairs"), (2, 0, "stride")])
    out.append((bat, tuple([None] + good2[1:]), "context"))
    return out, keep, rec


def test_entry_points_refuse_bad_arguments_without_a_device(ah):
    """the refusals come before any device is touched, so they hold on a machine without one: the pointers are never followed"""
    assert {"hak_triangulate", "hak_triangulate_batch"} <= set(ah.SYMBOLS)
    assert ah.TRIANGULATION_DTYPE == tr.TRIANGULATION_DTYPE and ah.TRIANGULATION_DTYPE.itemsize == 32
    assert (ah.VIEW_IDENTITY, ah.VIEW_RELATIVE, ah.VIEW_ABSOLUTE) == (0, 1, 2)
    calls, keep, rec = refusals(ah, None, 4096, 4096)
    assert len(calls) >= 50
    for k, (fn, args, word) in enumerate(calls):
        assert fn(*args) != 0, (k, args)
        msg = ah.lib.hak_last_error().decode()
        assert word in msg, (k, word, msg)                              # refused for the reason the case is about
    assert not rec.tobytes().strip(b"\0")                               # nothing was written through a refused call's pointers


def test_four_view_scene_extends_the_three_view_recipe(synth):
    sc = synth.four_view_scene(6, 120, 0.0, 0.25)
    assert len(sc) == 14
    K, (R01, t01), (R12, t12), A, B, fa, fb, X0, pa, pb, (R23, t23), Cl, fc, pc = sc
    assert np.allclose(R23, synth.rotation_zyx((1.0, -3.0, -1.0))) and np.allclose(t23, (-0.8, 0.1, 0.15))
    assert len(A) == len(B) == len(Cl) == 120 and fa.sum() == fb.sum() == fc.sum() == 90
    assert (np.diff(Cl["query"]) > 0).all() and A.dtype == Cl.dtype
    # the lists chain: a correct match of B and the correct match of C for the same point share the keypoint of image 2
    Xb = np.zeros((120, 3))
    Xb[pa] = X0
    for i in np.nonzero(fb)[0][:40]:
        j = int(np.nonzero(pc == pb[i])[0][0])
        assert Cl["query"][j] == B["train"][i] and Cl["x1"][j] == B["x2"][i]
        X3 = R23 @ (R12 @ (R01 @ Xb[pb[i]] + t01) + t12) + t23
        if fc[j]:
            assert abs(FOCAL * X3[0] / X3[2] + W / 2.0 - Cl["x2"][j]) < 1e-3
    again = synth.four_view_scene(6, 120, 0.0, 0.25)
    assert all(np.array_equal(x, y) for x, y in zip((A, B, Cl, fa, fb, fc), (again[3], again[4], again[11], again[5], again[6], again[12])))
