"""CPU suite: Gauss-Newton refit of the absolute pose (hak_refine_pnp).  The numpy statement of the contract
(tests/pnp_refit_ref.py, the checker of the GPU tests) is held against planted scenes: the noisy pose table, the noisy three-view
chains, the degenerate inputs, and the randomised family of test_pnp_cpu.parity_case, of which it is asserted on the statement
alone that it reaches every exit of the rule; the entry points are exported and refuse bad arguments without a device."""
import os
import re
import subprocess

import numpy as np
import pytest

import pnp_ref as pn
import pnp_refit_ref as pf
import pose_ref as pr
from test_pnp_cpu import K_TABLE, N_TABLE, NOISY, PARITY_CASES, TABLE, chain, parity_case, synth, table_case  # noqa: F401 (fixture)
from test_pose_cpu import dir_angle, rot_angle

TABLE_NOISE, TABLE_ITERATIONS, TABLE_THRESHOLD, TABLE_ROUNDS = 0.5, 64, 2.0, 3


def _t2(threshold):
    return np.float32(threshold) * np.float32(threshold)


def _count(record, corr, K, threshold):
    M = np.concatenate([record["R"], record["t"]])
    return int(pn.inlier_mask(M, pn.records(corr), pr.intrinsics(K), _t2(threshold))[0].sum())


def _no_model(out, mask, n):
    return (out["hypothesis"] == -1 and out["inliers"] == 0 and out["solution"] == 0 and out["n"] == n and not out["t"].any()
            and np.array_equal(out["R"], np.eye(3, dtype=np.float32).reshape(9)) and not mask.any() and len(mask) == n)


def _check_output(corr, K, rec0, out, mask, threshold, trace):
    """what holds for every input"""
    n = len(corr)
    cur0 = np.concatenate([rec0["R"], rec0["t"]])
    if rec0["hypothesis"] < 0 or not np.isfinite(cur0).all():
        assert _no_model(out, mask, n) and trace == (0, pf.NO_MODEL)
        return
    assert out["hypothesis"] == rec0["hypothesis"] and out["n"] == n and len(mask) == n
    assert out["inliers"] >= _count(rec0, corr, K, threshold)
    assert out["inliers"] == mask.sum() == _count(out, corr, K, threshold)
    assert not mask[~np.isfinite(pn.records(corr)).all(axis=1)].any()   # NaN / inf records are never inliers
    if trace[0] > 0:
        assert out["solution"] == pf.REFINED_SOLUTION
    else:
        assert out["solution"] == rec0["solution"] and out["R"].tobytes() == rec0["R"].tobytes() and out["t"].tobytes() == rec0["t"].tobytes()


def refine(corr, K, rec0, threshold, rounds):
    """(record, mask, (accepted rounds, where the call stopped)) with the checks that hold for every input"""
    tr = []
    out, mask = pf.refine_pnp(corr, K, rec0, threshold, rounds, trace=tr)
    _check_output(corr, K, rec0, out, mask, threshold, tr[0])
    return out, mask, tr[0]


def noisy_table_case(synth, k):
    corr, R, t, front = table_case(synth, k)
    rng = np.random.default_rng(5000 + k)
    u = corr["u"].astype(np.float64) + rng.normal(0, TABLE_NOISE, N_TABLE)
    v = corr["v"].astype(np.float64) + rng.normal(0, TABLE_NOISE, N_TABLE)
    corr["u"], corr["v"] = u, v                                         # rounded to float32
    return corr, R, t


def test_noisy_pose_table(synth):
    """the 42 poses of test_pnp_cpu with 0.5 px of noise: the three-point winner of 64 hypotheses at 2 px against three rounds of the
    refit.  When written: the rotation error falls in 40 of 42 and |t - t_true| in 42 of 42, to a median of 0.29 / 0.28 of the
    winner's (the two rotation losers are scenes where the winner was already within 0.02 degrees)"""
    assert len(TABLE) == 42
    rot_lower = t_lower = 0
    rot_ratio, t_ratio = [], []
    for k in range(len(TABLE)):
        corr, R, t = noisy_table_case(synth, k)
        rec0, _ = pn.solve_pnp(corr, K_TABLE, TABLE_ITERATIONS, TABLE_THRESHOLD, k)
        out, mask, (accepted, why) = refine(corr, K_TABLE, rec0, TABLE_THRESHOLD, TABLE_ROUNDS)
        assert rec0["hypothesis"] >= 0 and out["inliers"] >= rec0["inliers"], (k, rec0, out)
        assert (out["solution"] == pf.REFINED_SOLUTION) == (accepted > 0), (k, out, accepted, why)
        a0, a1 = rot_angle(rec0["R"].reshape(3, 3), R), rot_angle(out["R"].reshape(3, 3), R)
        t0, t1 = (float(np.linalg.norm(r["t"].astype(np.float64) - t)) for r in (rec0, out))
        rot_lower, t_lower = rot_lower + (a1 < a0), t_lower + (t1 < t0)
        rot_ratio.append(a1 / a0)
        t_ratio.append(t1 / t0)
        if k == 0:
            print(f"entry 0: rotation {a0:.4f} -> {a1:.4f} deg, |t - t_true| {t0:.2e} -> {t1:.2e}, inliers {rec0['inliers']} -> "
                  f"{out['inliers']}")
    print(f"noisy pose table: rotation error lower in {rot_lower} of 42, |t - t_true| lower in {t_lower} of 42, median ratios "
          f"{np.median(rot_ratio):.3f} / {np.median(t_ratio):.3f}")
    assert rot_lower >= 36 and t_lower >= 38
    assert np.median(rot_ratio) < 0.5 and np.median(t_ratio) < 0.5


def test_noisy_chains(synth):
    for n, noise, seed in NOISY:
        corr, planted, pose, rec0, mask0, R02, t02 = chain(synth, n, noise, seed)
        K = synth.three_view_scene(seed, n, noise, 0.3)[0]
        out, mask, (accepted, why) = refine(corr, K, rec0, 2.0, 3)
        share = planted[mask == 1].mean()
        a0, a1 = rot_angle(rec0["R"].reshape(3, 3), R02), rot_angle(out["R"].reshape(3, 3), R02)
        b0, b1 = dir_angle(rec0["t"], t02), dir_angle(out["t"], t02)
        print(f"noisy chain n={n} noise={noise} seed={seed}: {len(corr)} linked, inliers {rec0['inliers']} -> {out['inliers']} "
              f"({accepted} rounds accepted, then {why}), planted share {share:.3f}; rotation {a0:.4f} -> {a1:.4f} deg, translation "
              f"direction {b0:.4f} -> {b1:.4f} deg")
        assert out["inliers"] >= rec0["inliers"] == mask0.sum(), (n, noise, seed)
        assert share > 0.7, (n, noise, seed, share)


def test_corner_cases(synth):
    corr, R, t = noisy_table_case(synth, 10)
    rec0, _ = pn.solve_pnp(corr, K_TABLE, 64, 2.0, 10)
    assert rec0["hypothesis"] >= 0 and rec0["inliers"] > 50
    # lists too short for RANSAC to find a model, and any list with a record that has none: the no-model record
    for n in (0, 1, 2):
        short, _ = pn.solve_pnp(corr[:n], K_TABLE, 64, 2.0, 0)
        out, mask, tr = refine(corr[:n], K_TABLE, short, 2.0, 3)
        assert _no_model(out, mask, n) and tr == (0, pf.NO_MODEL)
    gone = rec0.copy()
    gone["hypothesis"] = -1                                             # hypothesis = -1 with a usable R: still no model
    nan_r = rec0.copy()
    nan_r["R"][4] = np.nan
    inf_t = rec0.copy()
    inf_t["t"][1] = np.inf
    for n in (0, 3, N_TABLE):
        for broken in (gone, nan_r, inf_t):
            out, mask, tr = refine(corr[:n], K_TABLE, broken, 2.0, 3)
            assert _no_model(out, mask, n) and tr == (0, pf.NO_MODEL)
    # fewer than four inliers: no round runs, the record comes back with the count at this call's threshold.  (Three points give
    # hak_solve_pnp a model that fits them; three correspondences cannot be refitted.)
    three, _ = pn.solve_pnp(corr[:3], K_TABLE, 64, 2.0, 0)
    assert three["hypothesis"] >= 0 and three["inliers"] == 3
    for lst, rec in ((corr[:3], three), (corr[:0], rec0), (corr[:3], rec0)):
        out, mask, tr = refine(lst, K_TABLE, rec, 2.0, 8)
        assert tr == (0, pf.FEW) and out["R"].tobytes() == rec["R"].tobytes() and out["solution"] == rec["solution"]
        assert out["inliers"] == mask.sum() <= 3 and out["n"] == len(lst)
    # exactly four inliers run a round
    inl = corr[pn.inlier_mask(np.concatenate([rec0["R"], rec0["t"]]), pn.records(corr), pr.intrinsics(K_TABLE), _t2(2.0))[0]]
    out, mask, tr = refine(inl[:4], K_TABLE, rec0, 2.0, 1)
    assert tr[1] in (pf.ROUNDS, pf.REJECTED) and tr != (0, pf.FEW)
    d, why = pf.solve(pf.normal_equations(pn.records(inl[:4]), pr.intrinsics(K_TABLE), np.concatenate([rec0["R"], rec0["t"]]),
                                          np.ones(4, bool)))
    assert d is not None and np.isfinite(d).all()
    # all-identical points (N has rank 2) and collinear points (rank 5): whatever the elimination makes of them, the inliers do not
    # fall and a record that is not accepted comes back unchanged (_check_output)
    same = inl.copy()
    for f in ("X", "Y", "Z", "u", "v"):
        same[f] = same[f][0]
    out, mask, tr = refine(same, K_TABLE, rec0, 2.0, 3)
    assert out["inliers"] == len(same)
    line = inl.copy()
    s = np.linspace(-1.0, 1.0, len(line))
    M = rec0["R"].astype(np.float64).reshape(3, 3)
    Xw = np.array([0.3, -0.2, 8.0]) + s[:, None] * np.array([1.0, 0.5, 0.25])         # camera frame, then to the world and projected
    Xo = (Xw - rec0["t"].astype(np.float64)) @ M
    line["X"], line["Y"], line["Z"] = Xo.T
    line["u"], line["v"] = 1500.0 * Xw[:, 0] / Xw[:, 2] + 960.0, 1500.0 * Xw[:, 1] / Xw[:, 2] + 540.0
    out, mask, tr = refine(line, K_TABLE, rec0, 2.0, 3)
    assert out["inliers"] >= len(line) - 1
    # non-finite fields in half the records: they enter no sum -- the refit equals the refit of the finite half
    for f, bad in (("X", np.nan), ("Z", np.inf), ("u", -np.inf), ("v", np.nan)):
        some = corr.copy()
        some[f][::2] = bad
        a, am, atr = refine(some, K_TABLE, rec0, 2.0, 3)
        b, bm, btr = refine(corr[1::2], K_TABLE, rec0, 2.0, 3)
        assert not am[::2].any() and np.array_equal(am[1::2], bm) and atr == btr, f
        # (the lanes differ, so the sums agree to rounding only: the poses are compared, not their bits)
        assert np.abs(a["R"] - b["R"]).max() < 1e-5 and np.abs(a["t"] - b["t"]).max() < 1e-4, f
        S = pf.normal_equations(pn.records(some), pr.intrinsics(K_TABLE), np.concatenate([rec0["R"], rec0["t"]]),
                                pn.inlier_mask(np.concatenate([rec0["R"], rec0["t"]]), pn.records(some), pr.intrinsics(K_TABLE), _t2(2.0))[0])
        assert np.isfinite(S).all(), f
    # a refined record goes in again, and at another threshold the count is this call's
    a, am, atr = refine(corr, K_TABLE, rec0, 2.0, 1)
    assert atr == (1, pf.ROUNDS) and a["solution"] == 4
    b, bm, btr = refine(corr, K_TABLE, a, 2.0, 2)
    assert b["inliers"] >= a["inliers"] and b["solution"] == 4
    c, cm, ctr = refine(corr, K_TABLE, b, 0.7, 1)
    assert c["inliers"] == cm.sum() >= _count(b, corr, K_TABLE, 0.7) and c["inliers"] < b["inliers"]
    # rounds = 8 ends at the first round that is not accepted (at 0.6 px the sixth): the later rounds change nothing
    full, _, ftr = refine(corr, K_TABLE, rec0, 0.6, 8)
    assert ftr[1] == pf.REJECTED and 0 < ftr[0] < 7, ftr
    assert pf.refine_pnp(corr, K_TABLE, rec0, 0.6, ftr[0] + 1)[0].tobytes() == full.tobytes()
    assert pf.refine_pnp(corr, K_TABLE, rec0, 0.6, ftr[0])[0].tobytes() == full.tobytes()
    assert pf.refine_pnp(corr, K_TABLE, rec0, 0.6, ftr[0] - 1)[0].tobytes() != full.tobytes()


# ---- the committed cases of test_gpu_pnp_refit.py::test_randomised_parity: drawn here so that what they reach can be asserted on the
# statement alone
FAMILY_ROUNDS = (1, 2, 3, 8)
FAMILY_AXIS = 12
FAMILY_CASES = 2 * PARITY_CASES + FAMILY_AXIS


def family_case(j, solved=None):
    """member j of the randomised refit family: dict(corr, K, record, threshold, rounds, ctx, group, kind).  A pure function of j.
    Members 0 .. 149 ("own"): test_pnp_cpu.parity_case(j) -- its scenes, cameras, sizes, NaN rows, duplicates, scales -- with the
    statement's hak_solve_pnp record at the case's threshold, rounds FAMILY_ROUNDS[j % 4]; its `group` is the case's, for the ragged
    batch calls.  Members 150 .. 299 ("tight"): the same lists and records refined with 8 rounds at 0.3 of the threshold RANSAC
    ran at, where the first rounds move the pose most and a later round is often the first to lose an inlier.
    Members 300 .. 311 ("axis"): no record of hak_solve_pnp reaches the singular exit -- a pivot of step 4 is exactly 0 only when a
    column of N is, that is when every inlier has xc = yc = 0 exactly, points on the optical axis, and collinear points give the
    three-point solve no model -- so these members are built: the camera of parity_case(j), 4 .. 320 points at X = Y = 0 under the
    record R = I, t = 0, observed at (cx, cy), with off-axis non-inliers and NaN rows among them.  Columns 2 and 5 of N are 0 and
    the round fails at the pivot of column 2.  `solved` may pass the parity cases' records in, to spare the RANSAC."""
    from test_pnp_cpu import corr_array, parity_camera, PARITY_CAMERAS
    if j < 2 * PARITY_CASES:
        k = j % PARITY_CASES
        c = parity_case(k)
        rec0 = solved[k] if solved is not None else pn.solve_pnp(c["corr"], c["K"], c["iterations"], c["threshold"], c["seed"])[0]
        own = j < PARITY_CASES
        return dict(corr=c["corr"], K=c["K"], record=rec0, threshold=c["threshold"] if own else float(np.float32(0.3 * c["threshold"])),
                    rounds=FAMILY_ROUNDS[k % 4] if own else 8, ctx=c["ctx"] != own, group=c["group"] if own else -1,
                    kind="own" if own else "tight")
    rng = np.random.default_rng([PARITY_SEED_AXIS, j])
    K = parity_camera(rng, PARITY_CAMERAS[j % len(PARITY_CAMERAS)])
    n = int((4, 5, 63, 64, 65, 320)[j % 6])
    cx, cy = np.float32(K[2]), np.float32(K[3])
    X = np.zeros((n, 3))
    X[:, 2] = rng.uniform(1.0, 50.0, n)
    uv = np.stack([np.full(n, cx, np.float64), np.full(n, cy, np.float64)], axis=1)
    extra = int(rng.integers(0, 40))                                    # off the axis and far from where they project
    Xe = np.stack([rng.uniform(1, 3, extra), rng.uniform(1, 3, extra), rng.uniform(1, 50, extra)], axis=1)
    order = rng.permutation(n + extra)
    corr = corr_array(np.concatenate([X, Xe])[order], np.concatenate([uv, np.full((extra, 2), -1e6)])[order])
    if j % 2:
        corr["Z"][order == 0] = np.nan                                  # one of the axis points is not finite
    rec = np.zeros((), pn.ABS_POSE_DTYPE)
    rec["R"], rec["inliers"], rec["n"] = np.eye(3, dtype=np.float32).reshape(9), n, n + extra
    return dict(corr=corr, K=K, record=rec, threshold=float(np.float32(rng.uniform(0.5, 4.0))), rounds=FAMILY_ROUNDS[j % 4],
                ctx=bool(j % 2), group=-1, kind="axis")


PARITY_SEED_AXIS = 5077


@pytest.fixture(scope="module")
def family():
    """every family member, computed once"""
    solved = [pn.solve_pnp(c["corr"], c["K"], c["iterations"], c["threshold"], c["seed"])[0]
              for c in (parity_case(k) for k in range(PARITY_CASES))]
    return [family_case(j, solved) for j in range(FAMILY_CASES)]


def test_family_is_pure_and_reaches_every_exit(family):
    """what the statement alone says about the cases test_gpu_pnp_refit.py runs: conditions on the inputs, not measurements of the
    kernel.  Counted when written, own / tight / axis: no model 59 / 59 / 0, m < 4 23 / 29 / 0, singular 0 / 0 / 12, rejected
    7 / 11 / 0 (after 0 .. 6 accepted rounds), every round used 61 / 51 / 0; accepted rounds 0 / 1 / 2 / 3 or more:
    87 / 18 / 14 / 31 own and 92 / 1 / 1 / 56 tight"""
    assert len(family) >= 100
    a, b = family_case(7), family_case(7)
    assert a["corr"].tobytes() == b["corr"].tobytes() and a["record"].tobytes() == b["record"].tobytes()
    assert a["corr"].tobytes() == family[7]["corr"].tobytes() and a["record"].tobytes() == family[7]["record"].tobytes()
    a, b = family_case(FAMILY_CASES - 1), family[FAMILY_CASES - 1]
    assert a["corr"].tobytes() == b["corr"].tobytes() and a["K"] == b["K"] and a["threshold"] == b["threshold"]
    exits, accepted, rejected_after = {}, {}, set()
    for j, m in enumerate(family):
        out, mask, (acc, why) = refine(m["corr"], m["K"], m["record"], m["threshold"], m["rounds"])
        exits[(m["kind"], why)] = exits.get((m["kind"], why), 0) + 1
        accepted[(m["kind"], min(acc, 3))] = accepted.get((m["kind"], min(acc, 3)), 0) + 1
        if why == pf.REJECTED:
            rejected_after.add(acc)
        if m["kind"] == "axis":
            assert (acc, why) == (0, pf.SINGULAR) and out["inliers"] in (m["record"]["inliers"], m["record"]["inliers"] - 1), (j, out)
    print("pnp refit family: exits", exits, "accepted rounds (3 = three or more)", accepted, "rejected after", sorted(rejected_after))
    total = lambda d, key: sum(v for (kind, k), v in d.items() if k == key)
    for why in (pf.NO_MODEL, pf.FEW, pf.SINGULAR, pf.REJECTED, pf.ROUNDS):
        assert total(exits, why) >= 5, (why, exits)
    assert all(total(accepted, acc) >= 5 for acc in (0, 1, 2, 3)), accepted
    assert {0, 1} <= rejected_after and max(rejected_after) >= 3        # rejected at the first round, and after accepted ones
    groups = sorted({m["group"] for m in family if m["group"] >= 0})
    assert len(groups) >= 5


def refusals(ah, ctx, p, cntp):
    """every refused call of the two entry points as (function, arguments): p a valid 16-byte aligned pointer (device memory on a
    machine with one), cntp a valid int pointer; ctx a context or None (then the batch form is refused for that alone)"""
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
    keep.append(rec)
    io = rec.ctypes.data
    one, batch = lib.hak_refine_pnp, lib.hak_refine_pnp_batch
    bad_k = [k_with(fx=0.0), k_with(fy=0.0), k_with(fx=nan), k_with(fy=inf), k_with(cx=nan), k_with(cy=-inf)]
    out = [(one, (None, p, 8, kp, 1.0, r, None, io)) for r in (0, -1, 9)]
    out += [(one, (None, p, 8, kp, thr, 3, None, io)) for thr in (0.0, -1.0, nan, inf)]
    out += [(one, (None, p, 8, b, 1.0, 3, None, io)) for b in bad_k]
    out += [(one, (None, p, 8, None, 1.0, 3, None, io)), (one, (None, p, 8, kp, 1.0, 3, None, None)),
            (one, (None, p, -1, kp, 1.0, 3, None, io)), (one, (None, None, 8, kp, 1.0, 3, None, io)),
            (one, (None, p + 4, 8, kp, 1.0, 3, None, io))]
    out += [(batch, (None, p, 64, cntp, 1, kp, 1.0, 3, p, None))]                                      # no context
    if ctx is not None:
        out += [(one, (ctx, p, 8, kp, 1.0, 0, None, io)), (one, (ctx, p + 8, 8, kp, 1.0, 3, None, io)),
                (batch, (ctx, None, 64, cntp, 1, kp, 1.0, 3, p, None)), (batch, (ctx, p, 64, None, 1, kp, 1.0, 3, p, None)),
                (batch, (ctx, p, 64, cntp, 1, kp, 1.0, 3, None, None)), (batch, (ctx, p, 64, cntp, 0, kp, 1.0, 3, p, None)),
                (batch, (ctx, p, 0, cntp, 1, kp, 1.0, 3, p, None)), (batch, (ctx, p + 8, 64, cntp, 1, kp, 1.0, 3, p, None)),
                (batch, (ctx, p, 64, cntp, 1, None, 1.0, 3, p, None)), (batch, (ctx, p, 64, cntp, 1, kp, 1.0, 0, p, None)),
                (batch, (ctx, p, 64, cntp, 1, kp, 1.0, 9, p, None)), (batch, (ctx, p, 64, cntp, 1, kp, nan, 3, p, None)),
                (batch, (ctx, p, 64, cntp, 1, kp, 0.0, 3, p, None)), (batch, (ctx, p, 64, cntp, 1, bad_k[0], 1.0, 3, p, None)),
                (batch, (ctx, p, 64, cntp, 1, bad_k[4], 1.0, 3, p, None))]
    return out, keep, rec


def test_entry_points_exported(ah):
    out = subprocess.check_output(["nm", "-D", "--defined-only", ah.LIB_PATH], text=True)
    exported = set(re.findall(r" T (hak_[a-z0-9_]+)", out))
    assert {"hak_refine_pnp", "hak_refine_pnp_batch"} <= exported
    cxx = subprocess.check_output(["nm", "-D", "-C", "--defined-only", os.path.join(os.path.dirname(ah.LIB_PATH), "libakaze_hip.so")],
                                  text=True)
    assert "akaze::cuRefinePnP(" in cxx
    assert callable(ah.refinePnP)
    header = open(os.path.join(os.path.dirname(ah.LIB_PATH), "..", "include", "hipakaze.h")).read()
    assert "hak_refine_pnp_batch" in header and "4 = refitted by hak_refine_pnp" in header


def test_entry_points_refuse_bad_arguments_without_a_device(ah):
    """the refusals come before any device is touched, so they hold on a machine without one: the pointers are never followed"""
    calls, keep, rec = refusals(ah, None, 4096, 4096)
    assert len(calls) >= 19
    for k, (fn, args) in enumerate(calls):
        assert fn(*args) != 0, (k, args)
        assert ah.lib.hak_last_error().decode() != "", (k, args)
    assert not rec.tobytes().strip(b"\0")                               # nothing was written through a refused call's pointers
    if ah.device_count() == 0:
        K = ah.intrinsics(K_TABLE)
        assert ah.lib.hak_refine_pnp(None, None, 0, K.ctypes.data, 1.0, 3, None, rec.ctypes.data) != 0
        assert "no HIP device" in ah.lib.hak_last_error().decode()
