"""CPU suite: calibrated Gauss-Newton refit of the relative pose (hak_refine_pose).  The numpy statement of the contract
(tests/pose_refit_ref.py, the checker of the GPU tests) is held against planted scenes: the exact pose table, the nine noisy scenes
of the accuracy table (README.md), the three- and four-view chains with the refit inserted, and the randomised family of
test_pose_cpu.parity_case with built members for the rare exits, of which it is asserted on the statement alone that it reaches
the exits of the rule; the entry points are exported and refuse bad arguments without a device."""
import os
import re
import subprocess

import numpy as np
import pytest

import fundamental_ref as fr
import fundamental_refit_ref as rr
import link_ref as lr
import pnp_ref as pn
import pnp_refit_ref as pf
import pose_ref as pr
import pose_refit_ref as pz
import triangulate_ref as tr
from test_pnp_cpu import NOISY as CHAIN3
from test_pose_cpu import (N_TABLE, PARITY_CASES, TABLE, WORST_DIR_DEG, WORST_ROT_DEG, dir_angle, noisy_case, parity_case, rot_angle,
                           synth, table_case)  # noqa: F401 (fixture)
from test_triangulate_cpu import LEGS as CHAIN4

# the nine scenes of the accuracy table: (n, noise px, seed), 70 % planted; the input pose is the statements' chain
# find_fundamental 256 x 1 px -> refine_fundamental 3 rounds -> recover_pose at 1 px, depth < 50
SCENES = [(300, 0.3, 1), (300, 1.0, 2), (300, 0.6, 3), (1000, 0.3, 4), (1000, 1.0, 5), (1000, 0.6, 6), (400, 0.5, 7), (400, 1.0, 8),
          (2500, 0.5, 9)]
SETTINGS = [(1.0, 3), (2.0, 8)]                                         # (threshold px, rounds)
MAX_DEPTH = 50.0
# measured with the statement when written, per scene: (rotation, baseline-direction error in degrees) of the input pose and of
# the refit at each setting, and the matches in front (input: hak_recover_pose's field; refit: in_front)
MEASURED_INPUT = [(0.046, 0.103, 210), (0.584, 4.222, 108), (0.042, 0.180, 192), (0.016, 0.090, 700), (0.142, 0.930, 417),
                  (0.035, 0.240, 634), (0.029, 0.718, 268), (0.111, 3.171, 170), (0.019, 0.057, 1678)]
MEASURED = {(1.0, 3): [(0.044, 0.053, 210), (0.228, 2.780, 45), (0.013, 0.070, 189), (0.014, 0.024, 700), (0.054, 0.706, 388),
                       (0.039, 0.103, 642), (0.028, 0.077, 271), (0.395, 1.586, 122), (0.007, 0.032, 1678)],
            (2.0, 8): [(0.044, 0.053, 210), (0.114, 0.383, 197), (0.022, 0.143, 210), (0.014, 0.026, 701), (0.068, 0.093, 666),
                       (0.008, 0.045, 700), (0.014, 0.067, 280), (0.036, 0.208, 264), (0.011, 0.006, 1751)]}


def _no_pose(out, mask, xyz, n):
    return (out["candidate"] == -1 and out["inliers"] == 0 and out["in_front"] == 0 and out["n"] == n and not out["t"].any()
            and np.array_equal(out["R"], np.eye(3, dtype=np.float32).reshape(9)) and not mask.any() and not xyz.any()
            and len(mask) == n and xyz.shape == (n, 3))


def refine(recs, K1, rec0, K2, threshold, max_depth, rounds):
    """(record, mask, xyz, (accepted rounds, where the call stopped)) with the checks that hold for every input"""
    trace = []
    out, mask, xyz = pz.refine_pose(recs, K1, rec0, K2, threshold, max_depth, rounds, trace=trace)
    acc, why = trace[0]
    n = len(recs)
    if why == pz.NO_MODEL:
        assert _no_pose(out, mask, xyz, n) and acc == 0
        return out, mask, xyz, trace[0]
    assert out["n"] == n and len(mask) == n and xyz.shape == (n, 3)
    assert out["in_front"] == mask.sum() >= pz.count_under(recs, rec0, K1, K2, threshold, max_depth)       # monotone
    assert out["in_front"] == pz.count_under(recs, out, K1, K2, threshold, max_depth) <= out["inliers"]
    assert (out["candidate"] == pz.REFINED_CANDIDATE) == (acc > 0 or rec0["candidate"] == pz.REFINED_CANDIDATE)
    assert not xyz[mask == 0].any() and (xyz[mask == 1, 2] > 0).all()
    assert not mask[~np.isfinite(pr.records(recs)).all(axis=1)].any()
    if acc == 0:
        assert out["candidate"] == rec0["candidate"] and out["R"].tobytes() == np.array(rec0["R"], np.float32).tobytes()
        assert out["t"].tobytes() == np.array(rec0["t"], np.float32).tobytes()
    return out, mask, xyz, trace[0]


@pytest.fixture(scope="module")
def scenes(synth):
    """(recs, planted flags, K, R, t, the input pose record) of every scene, computed once"""
    out = []
    for n, noise, seed in SCENES:
        recs, flags, rec1, K, R, t = noisy_case(synth, n, noise, seed)
        out.append((recs, flags, K, R, t, pr.recover_pose(recs, rec1, K, None, 1.0, MAX_DEPTH)[0]))
    return out


def test_statement_is_pure(scenes):
    recs, flags, K, R, t, p0 = scenes[1]
    keep = (recs.copy(), p0.copy())
    a = pz.refine_pose(recs, K, p0, None, 2.0, MAX_DEPTH, 8)
    b = pz.refine_pose(recs, K, p0, None, 2.0, MAX_DEPTH, 8)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert recs.tobytes() == keep[0].tobytes() and p0.tobytes() == keep[1].tobytes()          # the inputs are left alone
    assert a[0]["candidate"] == pz.REFINED_CANDIDATE and a[1].dtype == np.uint8 and a[2].dtype == np.float32
    # K2 = None is K2 = K1, and a 3 x 3 K is the four numbers
    c = pz.refine_pose(recs, (K[0, 0], K[1, 1], K[0, 2], K[1, 2]), p0, K, 2.0, MAX_DEPTH, 8)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, c))


def test_exact_inputs_stay_exact(synth):
    """the 42 noise-free entries of the pose table: the refit leaves the errors within the table's own bounds and every match in
    front"""
    worst_rot = worst_dir = 0.0
    accepted = 0
    for k in range(len(TABLE)):
        recs, F, K, R, t, z = table_case(synth, k)
        p0 = pr.recover_pose(recs, F, K)[0]
        out, mask, xyz, (acc, why) = refine(recs, K, p0, None, 1.0, np.inf, 3)
        assert out["in_front"] == N_TABLE and mask.all(), (k, out, acc, why)
        accepted += acc > 0
        worst_rot = max(worst_rot, rot_angle(out["R"].reshape(3, 3), R))
        worst_dir = max(worst_dir, dir_angle(out["t"], t))
    print(f"exact pose table behind the refit: worst rotation {worst_rot:.3e} deg, baseline {worst_dir:.3e} deg, a round accepted in "
          f"{accepted} of {len(TABLE)}")
    assert worst_rot <= 10 * WORST_ROT_DEG and worst_dir <= 10 * WORST_DIR_DEG


def test_what_the_refit_buys(scenes):
    """the accuracy table of README.md.  The conditions are the feature's: the input pose alone meets them with equality"""
    base = [(rot_angle(p0["R"].reshape(3, 3), R), dir_angle(p0["t"], t), int(p0["in_front"])) for _, _, _, R, t, p0 in scenes]
    rows = {}
    for thr, rounds in SETTINGS:
        rows[(thr, rounds)] = []
        for recs, flags, K, R, t, p0 in scenes:
            out, mask, xyz, trace = refine(recs, K, p0, None, thr, MAX_DEPTH, rounds)
            rows[(thr, rounds)].append((rot_angle(out["R"].reshape(3, 3), R), dir_angle(out["t"], t), int(out["in_front"]), trace))
    print("n, noise, seed | recover_pose | refit 1 px x 3 | refit 2 px x 8 | planted   (rotation / baseline deg (in front))")
    for k, (n, noise, seed) in enumerate(SCENES):
        cells = [f"{a:.3f} / {b:.3f} ({c})" for a, b, c in [base[k]] + [rows[s][k][:3] for s in SETTINGS]]
        print(f"{n}, {noise}, {seed} | " + " | ".join(cells) + f" | {int(scenes[k][1].sum())}   {[rows[s][k][3] for s in SETTINGS]}")
    for k in range(len(SCENES)):
        assert base[k][0] <= 2 * MEASURED_INPUT[k][0] and base[k][1] <= 2 * MEASURED_INPUT[k][1], (k, base[k])
    for s in SETTINGS:
        dirs = [r[1] for r in rows[s]]
        assert np.median(dirs) <= np.median([b[1] for b in base]) and max(dirs) <= max(b[1] for b in base), (s, dirs)
        for k, (a, b, c, _) in enumerate(rows[s]):
            assert a <= 2 * MEASURED[s][k][0] and b <= 2 * MEASURED[s][k][1], (s, k, a, b)
    assert all(r[2] >= b[2] for r, b in zip(rows[(2.0, 8)], base)), rows[(2.0, 8)]
    lower = sum(r[1] < b[1] for r, b in zip(rows[(2.0, 8)], base))
    print(f"baseline-direction error lower in {lower} of {len(SCENES)} scenes at 2 px x 8")


def chain3(synth, n, noise, seed, refit):
    """the statements' three-view chain of test_pnp_cpu.chain, with the refit (threshold px, rounds) behind recover_pose or None"""
    K, (R01, t01), (R12, t12), A, B = synth.three_view_scene(seed, n, noise, 0.3)[:5]
    rec1 = rr.refine_fundamental(A, fr.find_fundamental(A, 256, 1.0, seed)[0], 1.0, 3)[0]
    pose, pmask, xyz = pr.recover_pose(A, rec1, K, None, 1.0, MAX_DEPTH)
    if refit:
        pose, pmask, xyz = pz.refine_pose(A, K, pose, None, refit[0], MAX_DEPTH, refit[1])
    corr = lr.link_tracks(A, pmask, xyz, B, 2 * n)
    out = pn.solve_pnp(corr, K, 256, 2.0, seed)[0]
    return pose, out, (R01, t01), (R12 @ R01, R12 @ t01 + t12)


def chain4(synth, n, noise, seed, refit):
    """the statements' four-view chain of test_triangulate_cpu.chain, with the refit behind recover_pose or None"""
    sc = synth.four_view_scene(seed, n, noise, 0.3)
    K, (R01, t01), (R12, t12), A, B, (R23, t23), Cl = sc[0], sc[1], sc[2], sc[3], sc[4], sc[10], sc[11]
    rec1 = rr.refine_fundamental(A, fr.find_fundamental(A, 256, 1.0, seed)[0], 1.0, 3)[0]
    pose, pmask, xyz = pr.recover_pose(A, rec1, K, None, 1.0, MAX_DEPTH)
    if refit:
        pose, pmask, xyz = pz.refine_pose(A, K, pose, None, refit[0], MAX_DEPTH, refit[1])
    corr2 = lr.link_tracks(A, pmask, xyz, B, 2 * n)
    ref2 = pf.refine_pnp(corr2, K, pn.solve_pnp(corr2, K, 256, 2.0, seed)[0], 2.0, 3)[0]
    tri, tmask, txyz = tr.triangulate(B, pose, ref2, K, None, 2.0, MAX_DEPTH, 0.01)
    corr3 = lr.link_tracks(B, tmask, txyz, Cl, 2 * n)
    ref3 = pf.refine_pnp(corr3, K, pn.solve_pnp(corr3, K, 256, 2.0, seed)[0], 2.0, 3)[0]
    R02, t02 = R12 @ R01, R12 @ t01 + t12
    return pose, ref2, ref3, (R01, t01), (R02, t02), (R23 @ R02, R23 @ t02 + t23)


def test_chain_effect(synth):
    """the refit at 2 px x 8 inserted into the three- and four-view chains: what the later views inherit.  Reported (README.md), not
    gated: only that every stage still finds a model is asserted"""
    err = lambda rec, Rt: f"{rot_angle(rec['R'].reshape(3, 3), Rt[0]):.3f} / {dir_angle(rec['t'], Rt[1]):.3f}"
    for n, noise, seed in CHAIN3:
        line = f"three views n={n} noise={noise} seed={seed}:"
        for refit in (None, (2.0, 8)):
            pose, out, Rt1, Rt2 = chain3(synth, n, noise, seed, refit)
            assert pose["candidate"] >= 0 and out["hypothesis"] >= 0
            line += f"  [{'refit' if refit else 'plain'}] I1 {err(pose, Rt1)} deg ({pose['in_front']} in front), I2 {err(out, Rt2)} deg, " \
                    f"{out['inliers']} PnP inliers of {out['n']}"
        print(line)
    for n, noise, seed in CHAIN4:
        line = f"four views n={n} noise={noise} seed={seed}:"
        for refit in (None, (2.0, 8)):
            pose, ref2, ref3, Rt1, Rt2, Rt3 = chain4(synth, n, noise, seed, refit)
            assert pose["candidate"] >= 0 and ref2["hypothesis"] >= 0 and ref3["hypothesis"] >= 0
            line += f"  [{'refit' if refit else 'plain'}] I1 {err(pose, Rt1)} deg, I2 {err(ref2, Rt2)} deg ({ref2['inliers']} of " \
                    f"{ref2['n']}), I3 {err(ref3, Rt3)} deg ({ref3['inliers']} of {ref3['n']})"
        print(line)


# ---- the committed cases of test_gpu_pose_refit.py::test_randomised_parity: drawn here so that what they reach can be asserted on
# the statement alone
FAMILY_SEED = 2071
BUILT = ("axis x", "axis y", "axis z", "four", "five", "row", "rotation", "gone", "nan", "inf", "again", "again tight")
FAMILY_CASES = 2 * PARITY_CASES + len(BUILT)


def _record(R, t, candidate=0):
    rec = np.zeros((), pr.POSE_DTYPE)
    rec["R"], rec["t"], rec["candidate"] = np.asarray(R, np.float64).reshape(9), t, candidate
    return rec


def family_case(j, posed=None):
    """member j of the randomised refit family: dict(recs, K1, K2, record, threshold, max_depth, rounds, ctx, group, kind).  A pure
    function of j.  Members 0 .. 149 ("own"): test_pose_cpu.parity_case(j) -- its scenes, models, cameras, depth limits, NaN rows,
    duplicates -- with the statement's hak_recover_pose record of the case (the record form: `hypothesis` is seen), at the case's
    threshold; rounds drawn from 1 .. 8, one draw per batch group (its `group` is the case's, for the ragged batch calls).
    Members 150 .. 299 ("tight"): the same lists and records at 0.3 of that threshold.  Then the built members, for the exits no
    drawn record reaches reliably:
      axis x / y / z  a noise-free scene whose record has t snapped onto a coordinate axis: two |t_k| are 0 and the basis tie
                      goes to the smaller index
      four, five      the first 4 and 5 matches that count under a noisy scene's pose: no round, and the first usable count
      row             R = I, t = (0, 0, 1) and matches on the image row through the principal point: columns 1 and 4 of N are
                      exactly 0 and the round fails at a zero pivot.  (A pure rotation cannot serve: where q and b coincide exactly
                      the two-ray determinant is exactly 0 and nothing counts, elsewhere the columns are tiny but not 0.)
      rotation        that pure rotation, with the planted R and an arbitrary t: whatever the rule makes of it
      gone, nan, inf  a usable R with candidate = -1; a NaN in R; an inf in t
      again           an already refitted record, at the same threshold and at 0.4 of it
    `posed` may pass the parity cases' pose records in, to spare the decompositions."""
    from akaze_hip import synth
    if j < 2 * PARITY_CASES:
        k = j % PARITY_CASES
        c = parity_case(k)
        rec0 = posed[k] if posed is not None else pr.recover_pose(c["recs"], c["record"], c["K1"], c["K2"], c["threshold"],
                                                                  c["max_depth"])[0]
        own = j < PARITY_CASES
        key = [FAMILY_SEED, c["group"], 1] if own and c["group"] >= 0 else [FAMILY_SEED, j]
        return dict(recs=c["recs"], K1=c["K1"], K2=c["K2"], record=rec0,
                    threshold=c["threshold"] if own else float(np.float32(0.3 * c["threshold"])), max_depth=c["max_depth"],
                    rounds=int(np.random.default_rng(key).integers(1, 9)), ctx=c["ctx"] != own, group=c["group"] if own else -1,
                    kind="own" if own else "tight")
    kind = BUILT[j - 2 * PARITY_CASES]
    base = dict(K2=None, threshold=1.0, max_depth=float("inf"), rounds=1 + j % 8, ctx=bool(j % 2), group=-1, kind=kind)
    if kind.startswith("axis"):
        axis = "xyz".index(kind[-1])
        k = {0: 1, 1: 4, 2: 2}[axis]                                    # table entries with R = I and the baseline along x, y, z
        recs, F, K, R, t, z = table_case(synth, k)
        rec0 = pr.recover_pose(recs, F, K)[0]
        snapped = np.zeros(3, np.float32)
        snapped[axis] = np.sign(rec0["t"][axis])
        assert np.abs(rec0["t"] - snapped).max() < 1e-5
        rec0["t"] = snapped
        return dict(base, recs=recs, K1=tuple(float(v) for v in (K[0, 0], K[1, 1], K[0, 2], K[1, 2])), record=rec0)
    if kind in ("four", "five", "again", "again tight", "gone", "nan", "inf"):
        recs, flags, rec1, K, R, t = noisy_case(synth, 300, 0.6, 3)
        K1 = tuple(float(v) for v in (K[0, 0], K[1, 1], K[0, 2], K[1, 2]))
        rec0 = pr.recover_pose(recs, rec1, K, None, 1.0, MAX_DEPTH)[0]
        base = dict(base, K1=K1, max_depth=MAX_DEPTH)
        if kind in ("four", "five"):
            cur = np.concatenate([rec0["R"], rec0["t"], pz.pose_F(rec0["R"], rec0["t"], pr.intrinsics(K1), pr.intrinsics(K1))[0]])
            counts = pz.counting(pr.records(recs), pr.intrinsics(K1), pr.intrinsics(K1), cur, np.float32(1.0), MAX_DEPTH)[1]
            few = recs[counts][:4 if kind == "four" else 5]
            others = recs[~counts][:3]
            return dict(base, recs=np.ascontiguousarray(np.concatenate([few[:2], others, few[2:]])), record=rec0, rounds=3)
        if kind.startswith("again"):
            once = pz.refine_pose(recs, K1, rec0, None, 1.0, MAX_DEPTH, 2)[0]
            assert once["candidate"] == pz.REFINED_CANDIDATE
            return dict(base, recs=recs, record=once, threshold=1.0 if kind == "again" else 0.4, rounds=8)
        bad = rec0.copy()
        if kind == "gone":
            bad["candidate"] = -1
        elif kind == "nan":
            bad["R"][4] = np.nan
        else:
            bad["t"][1] = np.inf
        return dict(base, recs=recs, record=bad)
    K1 = (1024.0, 1024.0, 512.0, 512.0)
    rng = np.random.default_rng([FAMILY_SEED, j])
    if kind == "row":
        x1 = 512.0 + 16.0 * rng.permutation(np.arange(2, 26))[:12]       # normalised x a multiple of 1 / 64, y = 0: exact
        recs = np.stack([x1, np.full(12, 512.0), 512.0 + (x1 - 512.0) / 2.0, np.full(12, 512.0)], axis=1).astype(np.float32)
        recs[5] = (100.0, 900.0, 700.0, 30.0)                           # and one match that is no inlier
        return dict(base, recs=recs, K1=K1, record=_record(np.eye(3), (0.0, 0.0, 1.0)), rounds=3)
    R = synth.rotation_zyx((3.0, -4.0, 2.0))                            # (rotation)
    uv = np.stack([rng.uniform(100, 900, 40), rng.uniform(100, 900, 40)], axis=1)
    ray = np.concatenate([(uv - 512.0) / 1024.0, np.ones((40, 1))], axis=1) @ R.T
    recs = np.concatenate([uv, 512.0 + 1024.0 * ray[:, :2] / ray[:, 2:]], axis=1).astype(np.float32)
    return dict(base, recs=recs, K1=K1, record=_record(R, (0.6, 0.0, 0.8)), rounds=3)


@pytest.fixture(scope="module")
def family():
    """every family member, computed once"""
    posed = []
    for k in range(PARITY_CASES):
        c = parity_case(k)
        posed.append(pr.recover_pose(c["recs"], c["record"], c["K1"], c["K2"], c["threshold"], c["max_depth"])[0])
    return [family_case(j, posed) for j in range(FAMILY_CASES)]


def test_family_is_pure_monotone_and_reaches_every_exit(family):
    """what the statement alone says about the cases test_gpu_pose_refit.py runs: conditions on the inputs, not measurements of the
    kernel.  The exit "non-finite" (finite pivots, then a non-finite solution, length or update) is a guard: the rule is invariant
    to the scale of a row, so no finite input was found that reaches it, and the family is not asked to"""
    a, b = family_case(7), family_case(7)
    assert a["recs"].tobytes() == b["recs"].tobytes() and a["record"].tobytes() == b["record"].tobytes()
    assert a["recs"].tobytes() == family[7]["recs"].tobytes() and a["record"].tobytes() == family[7]["record"].tobytes()
    assert a["rounds"] == family[7]["rounds"]
    exits, accepted, rejected_after, ties = {}, {}, set(), 0
    by_kind = {}
    for j, m in enumerate(family):
        out, mask, xyz, (acc, why) = refine(m["recs"], m["K1"], m["record"], m["K2"], m["threshold"], m["max_depth"], m["rounds"])
        exits[why] = exits.get(why, 0) + 1
        accepted[min(acc, 3)] = accepted.get(min(acc, 3), 0) + 1
        by_kind[m["kind"]] = (acc, why, int(out["in_front"]))
        if why == pz.REJECTED:
            rejected_after.add(acc)
        if why != pz.NO_MODEL:
            t = np.abs(m["record"]["t"].astype(np.float64))
            ties += int((t == t.min()).sum() > 1)
    print("pose refit family: exits", exits, "accepted rounds (3 = three or more)", accepted, "rejected after", sorted(rejected_after),
          "basis ties", ties, "built", {k: v for k, v in by_kind.items() if k not in ("own", "tight")})
    for why in (pz.NO_MODEL, pz.FEW, pz.SINGULAR, pz.REJECTED, pz.ROUNDS):
        assert exits.get(why, 0) >= (1 if why == pz.SINGULAR else 5), (why, exits)
    assert all(accepted.get(acc, 0) >= 5 for acc in (0, 1, 2, 3)), accepted
    assert 0 in rejected_after and max(rejected_after) >= 2
    assert ties >= 3
    for kind in ("axis x", "axis y", "axis z"):
        assert by_kind[kind][1] in (pz.ROUNDS, pz.REJECTED) and by_kind[kind][2] == N_TABLE, (kind, by_kind[kind])
    assert by_kind["four"] == (0, pz.FEW, 4) and by_kind["five"][1] != pz.FEW and by_kind["five"][2] >= 5, by_kind
    assert by_kind["row"] == (0, pz.SINGULAR, 11), by_kind["row"]
    assert by_kind["rotation"][1] not in (pz.NO_MODEL, pz.SINGULAR, pz.NON_FINITE), by_kind["rotation"]      # tiny columns, not 0
    assert all(by_kind[k][1] == pz.NO_MODEL for k in ("gone", "nan", "inf"))
    assert by_kind["again"][2] >= family[2 * PARITY_CASES + BUILT.index("again")]["record"]["in_front"]
    assert by_kind["again tight"][2] < by_kind["again"][2]
    assert len(sorted({m["group"] for m in family if m["group"] >= 0})) >= 5


def refusals(ah, ctx, p, cntp):
    """every refused call of the two entry points as (function, arguments): p a valid 16-byte aligned pointer (device memory on a
    machine with one), cntp a valid int pointer; ctx a context or None (then the batch form is refused for that alone)"""
    lib = ah.lib
    K = ah.intrinsics((1500.0, 1500.0, 960.0, 540.0))
    keep = [K]

    def k_with(**kw):
        b = K.copy()
        for f, v in kw.items():
            b[f] = v
        keep.append(b)
        return b.ctypes.data

    inf, nan = float("inf"), float("nan")
    kp = K.ctypes.data
    rec = np.zeros((), ah.POSE_DTYPE)
    keep.append(rec)
    io = rec.ctypes.data
    one, batch = lib.hak_refine_pose, lib.hak_refine_pose_batch
    bad_k = [k_with(fx=0.0), k_with(fy=0.0), k_with(fx=nan), k_with(fy=inf), k_with(cx=nan), k_with(cy=-inf)]
    out = [(one, (None, p, 8, kp, kp, 1.0, inf, r, None, None, io)) for r in (0, -1, 9)]
    out += [(one, (None, p, 8, kp, kp, thr, inf, 3, None, None, io)) for thr in (0.0, -1.0, nan, inf)]
    out += [(one, (None, p, 8, kp, kp, 1.0, md, 3, None, None, io)) for md in (0.0, -2.0, nan)]
    out += [(one, (None, p, 8, b, kp, 1.0, inf, 3, None, None, io)) for b in bad_k]
    out += [(one, (None, p, 8, kp, b, 1.0, inf, 3, None, None, io)) for b in bad_k]
    out += [(one, (None, p, 8, None, kp, 1.0, inf, 3, None, None, io)), (one, (None, p, 8, kp, None, 1.0, inf, 3, None, None, io)),
            (one, (None, p, 8, kp, kp, 1.0, inf, 3, None, None, None)), (one, (None, p, -1, kp, kp, 1.0, inf, 3, None, None, io)),
            (one, (None, None, 8, kp, kp, 1.0, inf, 3, None, None, io)), (one, (None, p + 4, 8, kp, kp, 1.0, inf, 3, None, None, io))]
    out += [(batch, (None, p, 64, cntp, 1, kp, kp, 1.0, inf, 3, p, None, None))]                          # no context
    if ctx is not None:
        out += [(one, (ctx, p, 8, kp, kp, 1.0, inf, 0, None, None, io)), (one, (ctx, p + 8, 8, kp, kp, 1.0, inf, 3, None, None, io)),
                (batch, (ctx, None, 64, cntp, 1, kp, kp, 1.0, inf, 3, p, None, None)),
                (batch, (ctx, p, 64, None, 1, kp, kp, 1.0, inf, 3, p, None, None)),
                (batch, (ctx, p, 64, cntp, 1, kp, kp, 1.0, inf, 3, None, None, None)),
                (batch, (ctx, p, 64, cntp, 0, kp, kp, 1.0, inf, 3, p, None, None)),
                (batch, (ctx, p, 0, cntp, 1, kp, kp, 1.0, inf, 3, p, None, None)),
                (batch, (ctx, p + 8, 64, cntp, 1, kp, kp, 1.0, inf, 3, p, None, None)),
                (batch, (ctx, p, 64, cntp, 1, None, kp, 1.0, inf, 3, p, None, None)),
                (batch, (ctx, p, 64, cntp, 1, kp, None, 1.0, inf, 3, p, None, None)),
                (batch, (ctx, p, 64, cntp, 1, kp, kp, 1.0, inf, 0, p, None, None)),
                (batch, (ctx, p, 64, cntp, 1, kp, kp, 1.0, inf, 9, p, None, None)),
                (batch, (ctx, p, 64, cntp, 1, kp, kp, nan, inf, 3, p, None, None)),
                (batch, (ctx, p, 64, cntp, 1, kp, kp, 0.0, inf, 3, p, None, None)),
                (batch, (ctx, p, 64, cntp, 1, kp, kp, 1.0, 0.0, 3, p, None, None)),
                (batch, (ctx, p, 64, cntp, 1, kp, kp, 1.0, nan, 3, p, None, None)),
                (batch, (ctx, p, 64, cntp, 1, bad_k[0], kp, 1.0, inf, 3, p, None, None)),
                (batch, (ctx, p, 64, cntp, 1, kp, bad_k[4], 1.0, inf, 3, p, None, None))]
    return out, keep, rec


def test_entry_points_exported(ah):
    out = subprocess.check_output(["nm", "-D", "--defined-only", ah.LIB_PATH], text=True)
    exported = set(re.findall(r" T (hak_[a-z0-9_]+)", out))
    assert {"hak_refine_pose", "hak_refine_pose_batch"} <= exported
    cxx = subprocess.check_output(["nm", "-D", "-C", "--defined-only", os.path.join(os.path.dirname(ah.LIB_PATH), "libakaze_hip.so")],
                                  text=True)
    assert "akaze::cuRefinePose(" in cxx
    assert callable(ah.refinePose)
    header = open(os.path.join(os.path.dirname(ah.LIB_PATH), "..", "include", "hipakaze.h")).read()
    assert "hak_refine_pose_batch" in header and "4 = refitted by hak_refine_pose" in header


def test_entry_points_refuse_bad_arguments_without_a_device(ah):
    """the refusals come before any device is touched, so they hold on a machine without one: the pointers are never followed"""
    calls, keep, rec = refusals(ah, None, 4096, 4096)
    assert len(calls) >= 29
    for k, (fn, args) in enumerate(calls):
        assert fn(*args) != 0, (k, args)
        assert ah.lib.hak_last_error().decode() != "", (k, args)
    assert not rec.tobytes().strip(b"\0")                               # nothing was written through a refused call's pointers
    if ah.device_count() == 0:
        K = ah.intrinsics((1500.0, 1500.0, 960.0, 540.0))
        assert ah.lib.hak_refine_pose(None, None, 0, K.ctypes.data, K.ctypes.data, 1.0, float("inf"), 3, None, None, rec.ctypes.data) != 0
        assert "no HIP device" in ah.lib.hak_last_error().decode()
