"""CPU suite of projection-guided matching (hak_match_projected, include/hipakaze.h): the ABI, the argument checks that need no
device, and the numpy statement tests/projected_match_ref.py against a plain double loop.  Also home of the fixtures the GPU suite
shares (tests/test_gpu_projected_match.py) -- the guided fixture lifted into 3-D, with the properties that make it a test of GATED
matching checked here, on the statement -- of the effect test against track linking, and of the statements' chain whose figures
the README's table holds (printed here)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fundamental_ref as fr
import fundamental_refit_ref as rr
import guided_match_ref as gr
import link_ref as lr
import pnp_ref as pn
import pnp_refit_ref as pf
import pose_ref as pr
import projected_match_ref as pm
from conftest import ROOT
from test_guided_match_cpu import IDENTITY, SIZES, brute_knn2, build_pair, random_points
from test_pose_cpu import dir_angle, rot_angle

ANGLES, T_VIEW = (2.0, -5.0, 1.5), (-1.0, 0.05, 0.1)                    # the planted view of the lifted fixture
K_LIFT = (500.0, 500.0, 320.0, 240.0)
# the legs of the README's table: (points, noise px, seed), look-alikes for 30 % of the points; radius of the re-match
LEGS = [(400, 0.5, 1), (400, 0.5, 2), (400, 1.0, 3), (1000, 0.5, 5)]
CHAIN_RADIUS = 8.0


@pytest.fixture(scope="module")
def synth(ah):
    from akaze_hip import synth
    return synth


def rt12(R, t):
    """twelve float32 {R row-major, t}"""
    return np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)]).astype(np.float32)


def identity_list(n):
    A = np.zeros(n, gr.MATCH_PAIR_DTYPE)
    A["query"] = A["train"] = np.arange(n)
    A["distance"], A["second"] = 20, 60
    return A


def lift(synth, q, seed, M=None, K=K_LIFT, depth=(4.0, 12.0)):
    """the points whose projections under the view M (default: the planted one) and K are the positions q (records with x, y, or an
    (n, 2) array), at camera depths uniform in `depth`: X = R^T (z K^-1 (x, y, 1) - t) in float64 from the float32 view, rounded to
    float32 -> (xyz (n, 3) float32, M).  A negative depth mirrors the point through the camera centre: it projects onto the same
    pixel from behind"""
    rng = np.random.default_rng(seed)
    M = rt12(synth.rotation_zyx(ANGLES), T_VIEW) if M is None else np.asarray(M, np.float32)
    R, t = M[:9].astype(np.float64).reshape(3, 3), M[9:].astype(np.float64)
    x, y = (q["x"], q["y"]) if getattr(q, "dtype", None) is not None and q.dtype.names else np.asarray(q).reshape(-1, 2).T
    z = rng.uniform(depth[0], depth[1], len(x))
    with np.errstate(all="ignore"):
        Xc = np.stack([(np.asarray(x, np.float64) - K[2]) / K[0] * z, (np.asarray(y, np.float64) - K[3]) / K[1] * z, z], axis=1)
        return ((Xc - t) @ R).astype(np.float32), M


def build_lifted(synth, n1, n2, dtype, seed=None):
    """test_guided_match_cpu.build_pair(n1, n2, 100 + n1, dtype, H = identity) lifted into 3-D: list A is the identity
    (train = m), D the queries, T the train set -> (A, xyz, D, T, M)"""
    q, t = build_pair(n1, n2, (100 + n1) if seed is None else seed, dtype, H=IDENTITY)
    xyz, M = lift(synth, q, 7000 + n1)
    return identity_list(n1), xyz, q, t, M


def shuffled(A, xyz, D, seed):
    """the same landmarks with `train` a permutation and D reordered to match, and a mask that drops every fifth landmark"""
    perm = np.random.default_rng(seed).permutation(len(A))
    A2 = A.copy()
    A2["train"] = perm
    D2 = D.copy()
    D2[perm] = D
    mask = (np.arange(len(A)) % 5 != 4).astype(np.uint8)
    return A2, D2, mask


def matches_of(corr, nA):
    """per landmark: the keypoint it was matched to, -1 when rejected"""
    m = np.full(nA, -1, np.int64)
    m[corr["src3d"]] = corr["src2d"]
    return m


def fixture_shares(A, xyz, D, T, M, radius=3.0):
    """what makes build_lifted a test of gated matching, measured on the statement at ratio 4/5 with the cross-check"""
    corr, why = pm.match_projected(A, None, xyz, D, T, M, K_LIFT, radius, (4, 5), True, 0)
    ungated = brute_knn2(D, T, (4, 5), True, 0)
    n = float(len(A))
    return dict(accepted=(why == 0).sum() / n, differs=(matches_of(corr, len(A)) != ungated).sum() / n, ratio=(why == 3).sum() / n,
                cross=(why == 4).sum() / n)


# ---------------------------------------------------------------------------------------------- ABI
def test_header_declares_library_exports_and_bindings(ah):
    hdr = open(os.path.join(ROOT, "include", "hipakaze.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", ah.LIB_PATH], text=True)
    exported = set(re.findall(r" T (hak_[a-z0-9_]+)", out))
    for name in ("hak_match_projected", "hak_match_projected_batch"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in ah.SYMBOLS and name in exported
        assert getattr(ah.lib.product, name) is not None
    assert "not a match index" in hdr[hdr.index("typedef struct hak_corr3d"):hdr.index("} hak_corr3d;")]
    assert callable(ah.matchProjected)
    cxx = subprocess.check_output(["nm", "-D", "-C", "--defined-only", os.path.join(os.path.dirname(ah.LIB_PATH), "libakaze_hip.so")],
                                  text=True)
    assert "akaze::cuMatchProjected(" in cxx
    assert "cuMatchProjected" in open(os.path.join(ROOT, "include", "akaze.h")).read()
    stub = open(os.path.join(ROOT, "cuda-akaze_amd", "host", "asan", "stub_hipakaze.cpp")).read()
    assert "int hak_match_projected(" in stub


def refusals(ah, ctx, p, cntp):
    """every refused call of the two entry points as (function, arguments, a word of the message): p a valid 16-byte aligned
    pointer (device memory on a machine with one), cntp a valid int pointer; ctx a context or None.  The batch form looks at its
    context last, so without one every other refusal still shows by its own message"""
    lib = ah.lib
    K = ah.intrinsics(K_LIFT)
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
    cnt = C.c_int(-5)
    keep.append(cnt)
    cp = C.pointer(cnt)
    one, bat = lib.hak_match_projected, lib.hak_match_projected_batch
    bad_k = [(k_with(fx=0.0), "fx"), (k_with(fy=0.0), "fx"), (k_with(fx=nan), "fx"), (k_with(fy=inf), "fx"), (k_with(cx=nan), "cx"),
             (k_with(cy=-inf), "cx")]
    good1 = [None, p, 8, None, p, p, 8, p, 8, view(), kp, 8.0, 4, 5, 1, 0, p, cp, None]
    good2 = [ctx, p, 64, cntp, 1, None, p, p, 64, cntp, 1, p, 64, cntp, 1, 1, p, 2, 1, kp, 8.0, 4, 5, 1, 0, p, 64, cntp]

    def vary(fn, good, changes):
        out = []
        for change in changes:
            args = list(good)
            for pos, val in zip(change[:-1:2], change[1:-1:2]):
                args[pos] = val
            out.append((fn, tuple(args), change[-1]))
        return out

    out = vary(one, good1, [(11, 0.0, "radius"), (11, -1.0, "radius"), (11, nan, "radius"), (11, inf, "radius"), (11, 3e19, "radius"),
                            (12, 0, "ratio"), (13, 0, "ratio"), (12, -4, "ratio"), (10, None, "intrinsics"), (17, None, "null"),
                            (2, -1, "negative"), (6, -1, "negative"), (8, -1, "negative"),
                            (2, 1 << 20, "2^20"), (6, 1 << 20, "2^20"), (8, 1 << 20, "2^20"),
                            (1, None, "null array"), (4, None, "null array"), (5, None, "null array"), (7, None, "null array"),
                            (16, None, 18, p, "h_out"), (1, p + 4, "aligned"), (16, p + 8, "aligned"),
                            (9, view(3, nan), "non-finite"), (9, view(11, inf), "non-finite"), (9, view(0, -inf), "non-finite")])
    out += vary(one, good1, [(10, b, word) for b, word in bad_k])
    out += vary(bat, good2, [(20, 0.0, "radius"), (20, nan, "radius"), (20, 3e19, "radius"), (21, 0, "ratio"), (22, -1, "ratio"),
                             (19, None, "intrinsics"), (19, bad_k[0][0], "fx"), (19, bad_k[5][0], "cx"), (27, None, "null"),
                             (1, None, "null"), (3, None, "null"), (6, None, "null"), (7, None, "null"), (9, None, "null"),
                             (11, None, "null"), (13, None, "null"), (25, None, "null"), (1, p + 8, "aligned"), (25, p + 8, "aligned"),
                             (17, 3, "kind"), (17, -1, "kind"), (16, None, "null view"), (16, None, 17, 1, "null view"),
                             (18, -1, "view step"), (2, 0, "strides"), (8, 0, "strides"), (12, 0, "strides"), (26, 0, "strides"),
                             (4, 0, "count steps"), (10, 0, "count steps"), (14, -2, "count steps"), (15, 0, "npairs")])
    out.append((bat, tuple([None] + good2[1:]), "context"))
    if ctx is not None:
        out += vary(bat, good2, [(15, 1 << 20, "pair capacity")])
    return out, keep, cnt


def test_entry_points_refuse_bad_arguments_without_a_device(ah):
    """the refusals come before any device is touched, so they hold on a machine without one: the pointers are never followed"""
    calls, keep, cnt = refusals(ah, None, 4096, 4096)
    assert len(calls) >= 60
    for k, (fn, args, word) in enumerate(calls):
        assert fn(*args) != 0, (k, args)
        msg = ah.lib.hak_last_error().decode()
        assert word in msg, (k, word, msg)                              # refused for the reason the case is about
    assert cnt.value == -5                                              # nothing was written through a refused call's pointers
    # nothing to match is not an error, and needs no device either
    K = ah.intrinsics(K_LIFT)
    assert ah.lib.hak_match_projected(None, None, 0, None, None, None, 0, None, 0, None, K.ctypes.data, 8.0, 4, 5, 1, 0, None,
                                      C.byref(cnt), None) == 0 and cnt.value == 0


# ---------------------------------------------------------------------------------------------- the statement
def loop_statement(A, mask, xyz, D, T, M, K, radius, ratio, cross_check, max_dist):
    """the rule of include/hipakaze.h as a plain double loop over float32 scalars -> [(m, j1, d1, d2)] of the accepted landmarks"""
    f = np.float32
    m_ = [f(v) for v in np.asarray(M, np.float32).reshape(12)]
    fx, fy, cx, cy = (f(v) for v in K)
    r2 = f(radius) * f(radius)
    max_dist = 96 if max_dist <= 0 else max_dist
    nA, n2, nD = len(A), len(T), len(D)
    G = np.zeros((nA, n2), bool)
    Dm = np.zeros((nA, n2), np.int64)
    with np.errstate(all="ignore"):
        for m in range(nA):
            e = int(A["train"][m])
            if not (0 <= e < nD) or (mask is not None and mask[m] == 0):
                continue
            X, Y, Z = (f(v) for v in xyz[m])
            xc = f(f(f(f(m_[0] * X) + f(m_[1] * Y)) + f(m_[2] * Z)) + m_[9])
            yc = f(f(f(f(m_[3] * X) + f(m_[4] * Y)) + f(m_[5] * Z)) + m_[10])
            zc = f(f(f(f(m_[6] * X) + f(m_[7] * Y)) + f(m_[8] * Z)) + m_[11])
            px, py = f(f(fx * f(xc / zc)) + cx), f(f(fy * f(yc / zc)) + cy)
            for j in range(n2):
                dx, dy = f(f(T["x"][j]) - px), f(f(T["y"][j]) - py)
                G[m, j] = bool(zc > 0) and bool(f(f(dx * dx) + f(dy * dy)) < r2)
                Dm[m, j] = sum(bin(int(a) ^ int(b)).count("1") for a, b in zip(D["features"][e], T["features"][j]))
    acc = []
    for m in range(nA):
        J = [j for j in range(n2) if G[m, j]]
        if not J:
            continue
        j1 = min(J, key=lambda j: (Dm[m, j], j))
        d1 = int(Dm[m, j1])
        d2 = min([int(Dm[m, j]) for j in J if j != j1], default=512)
        rev = min([k for k in range(nA) if G[k, j1]], key=lambda k: (Dm[k, j1], k))
        if d1 < max_dist and d1 * ratio[1] < d2 * ratio[0] and (not cross_check or rev == m):
            acc.append((m, j1, d1, d2))
    return acc


@pytest.mark.parametrize("seed", range(8))
def test_statement_equals_double_loop(ah, synth, seed):
    rng = np.random.default_rng(seed)
    n1, n2 = int(rng.integers(1, 41)), int(rng.integers(1, 41))
    q, t = build_pair(n1, n2, 50 + seed, ah.POINT_DTYPE, H=IDENTITY)
    xyz, M = lift(synth, q, 60 + seed)
    A, mask, D = identity_list(n1), None, q
    if seed == 1:                                                # non-finite points and train coordinates
        xyz[0, 0], xyz[n1 // 2, 2], xyz[n1 - 1, 1] = np.nan, np.inf, -np.inf
        t["y"][0], t["x"][n2 // 2] = np.inf, np.nan
    if seed == 2:                                                # a view that puts part of the set behind the camera, one at zc = 0
        M = rt12(synth.rotation_zyx((0.0, 0.0, 0.0)), (0.0, 0.0, -8.0))
        xyz, _ = lift(synth, q, 60 + seed, M=rt12(np.eye(3), (0.0, 0.0, 0.0)))
        xyz[0, 2] = 8.0
        zc = pm.project(xyz, M, K_LIFT)[2]
        assert zc[0] == 0 and ((zc <= 0).sum() > 0 or n1 < 4) and ((zc > 0).sum() > 0 or n1 < 4)
    if seed == 3:                                                # few prototypes: ties in both directions
        t["features"] = t["features"][np.arange(n2) % 3]
        D = q.copy()
        D["features"] = q["features"][np.arange(n1) % 2]
    if seed in (4, 5):                                           # a mask, a permuted train with out-of-range entries, a short D
        A, D, mask = shuffled(A, xyz, q, seed)
        A["train"][::7] = -1
        A["train"][3::9] = n1 + 5
        if seed == 5:
            D, mask = D[:max(n1 - 3, 1)], None
    if seed == 6:                                                # two landmarks with the same train (the same descriptor and point)
        A["train"][n1 - 1] = A["train"][0]
        xyz[n1 - 1] = xyz[0]
    for radius, ratio, cross, md in ((0.5, (4, 5), True, 0), (3.0, (1, 1), True, 40), (20.0, (4, 5), False, 0), (300.0, (1, 1), True, 0)):
        corr, why = pm.match_projected(A, mask, xyz, D, t, M, K_LIFT, radius, ratio, cross, md)
        lp = loop_statement(A, mask, xyz, D, t, M, K_LIFT, radius, ratio, cross, md)
        assert [(int(c["src3d"]), int(c["src2d"])) for c in corr] == [(m, j) for m, j, _, _ in lp], (seed, radius)
        assert (np.nonzero(why == 0)[0] == corr["src3d"]).all() and not corr["pad"].any()
        ms, js = corr["src3d"], corr["src2d"]
        for k, fld in enumerate(("X", "Y", "Z")):
            assert np.array_equal(corr[fld].view(np.uint32), xyz[ms, k].view(np.uint32))
        assert np.array_equal(corr["u"].view(np.uint32), t["x"][js].view(np.uint32))
        assert np.array_equal(corr["v"].view(np.uint32), t["y"][js].view(np.uint32))
    # a view without a model: nothing is accepted
    bad = np.zeros((), pn.ABS_POSE_DTYPE)
    bad["R"], bad["t"], bad["hypothesis"] = M[:9], M[9:], -1
    assert len(pm.match_projected(A, mask, xyz, D, t, bad, K_LIFT, 300.0)[0]) == 0
    Mn = M.copy()
    Mn[4] = np.nan
    assert len(pm.match_projected(A, mask, xyz, D, t, Mn, K_LIFT, 300.0)[0]) == 0


@pytest.mark.parametrize("n1,n2", [(1, 1), (40, 37), (150, 200)])
def test_identity_view_is_the_guided_rule(ah, n1, n2):
    """R = I, t = 0, K = (1, 1, 0, 0), Z = 1 and an identity list: the projection is the query's position, so the statement equals
    guided matching's under H = identity"""
    q, t = build_pair(n1, n2, 9, ah.POINT_DTYPE, H=IDENTITY)
    xyz = np.stack([q["x"], q["y"], np.ones(n1, np.float32)], axis=1)
    for radius, ratio, cross, md in ((3.0, (4, 5), True, 0), (20.0, (1, 1), True, 0), (1e5, (4, 5), False, 40)):
        corr, _ = pm.match_projected(identity_list(n1), None, xyz, q, t, None, (1, 1, 0, 0), radius, ratio, cross, md)
        _, pairs, _ = gr.match_guided(q, t, IDENTITY, radius, ratio, cross, md)
        assert np.array_equal(corr["src3d"], pairs["query"]) and np.array_equal(corr["src2d"], pairs["train"])
        assert np.array_equal(corr["u"], pairs["x2"]) and np.array_equal(corr["v"], pairs["y2"])


@pytest.mark.parametrize("n1,n2", [s for s in SIZES if s[0] >= 300])
def test_fixture_separates_gated_from_plain_matching(ah, synth, n1, n2):
    """the lifted fixture at the sizes the GPU suite uses: enough accepted landmarks, enough whose match differs from the ungated
    rule's, enough rejections by the ratio test inside the gate and by the cross-check alone; and the lift moves no projection by
    more than a fraction of the in-gate decoys' distance"""
    A, xyz, D, T, M = build_lifted(synth, n1, n2, ah.POINT_DTYPE)
    px, py, zc = pm.project(xyz, M, K_LIFT)
    shift = float(np.hypot(px - D["x"], py - D["y"]).max())
    s = fixture_shares(A, xyz, D, T, M)
    print(f"lifted fixture ({n1}, {n2}): {s}, projection shift <= {shift:.2e} px")
    assert (zc > 0).all() and shift <= 1e-3
    assert s["accepted"] >= 0.25 and s["differs"] >= 0.05 and s["ratio"] >= 0.05 and s["cross"] >= 0.01, s


# ---------------------------------------------------------------------------------------------- the new generator and the effect
def knn2_list(p1, p2, ratio=(4, 5), cross=True, max_dist=0):
    """the match list of hak_match_knn2 by its statement: guided matching under H = identity with every pair gated (the image
    coordinates are below 2^12, so a radius of 1e5 gates all)"""
    return gr.match_guided(p1, p2, IDENTITY, 1e5, ratio, cross, max_dist)[1]


def point_of(index, n_kp):
    """(3, n_kp): the point behind keypoint k of image i, -1 for a spurious one"""
    out = np.full((len(index), n_kp), -1, np.int64)
    for i, idx in enumerate(index):
        out[i, idx] = np.arange(len(idx))
    return out


def test_three_view_keypoints(ah, synth):
    K, (R01, t01), (R12, t12), sets, index, X0, look = synth.three_view_keypoints(6, 120, 0.0, 0.25)
    assert synth.POINT_DTYPE == ah.POINT_DTYPE
    assert len(sets) == 3 and all(len(s) == 240 and s.dtype == ah.POINT_DTYPE for s in sets) and index.shape == (3, 120)
    assert np.allclose(R01, synth.rotation_zyx((2.0, -5.0, 1.5))) and np.allclose(t12, (-0.9, -0.1, 0.25))
    assert (look >= 0).sum() == 30 and not np.isin(look[look >= 0], index[2]).any()
    X = [X0, X0 @ R01.T + t01, (X0 @ R01.T + t01) @ R12.T + t12]
    for i in range(3):
        p = X[i] @ K.T
        assert np.abs(p[:, 0] / p[:, 2] - sets[i]["x"][index[i]]).max() < 1e-3          # noise 0: the projections, rounded
        assert (sets[i]["features"][:, 60] & 0xC0 == 0).all()
    d01 = gr.hamming(sets[0][index[0]], sets[1][index[1]])
    own = np.diagonal(d01)
    assert own.min() >= 0 and own.max() <= 60 and np.median(d01) > 200                   # 5 .. 30 bits from the base, each side
    j = np.nonzero(look >= 0)[0]
    dl = np.diagonal(gr.hamming(sets[0][index[0][j]], sets[2][look[j]]))
    assert dl.max() <= 65 and np.diagonal(gr.hamming(sets[0][index[0]], sets[1][index[1]])).max() <= 60
    again = synth.three_view_keypoints(6, 120, 0.0, 0.25)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(sets, again[3])) and np.array_equal(look, again[6])


def test_projected_matching_recovers_what_linking_loses(ah, synth):
    """n = 400, look-alikes for 30 % of the points, 0.5 px of noise; landmarks are the correct matches of the 2-NN list of (I0, I1)
    with their planted points, the view is the planted one, radius 4: the statement finds at least 0.1 n more correct
    correspondences than linking the two 2-NN lists does, and at most 0.01 n wrong ones"""
    n = 400
    for seed in (1, 2):
        K, (R01, t01), (R12, t12), sets, index, X0, look = synth.three_view_keypoints(seed, n, 0.5, 0.3)
        pt = point_of(index, 2 * n)
        A, B = knn2_list(sets[0], sets[1]), knn2_list(sets[1], sets[2])
        pa = pt[0][A["query"]]
        good = (pa >= 0) & (pt[1][A["train"]] == pa)
        A, pa = A[good], pa[good]
        xyz = X0[pa].astype(np.float32)
        link = lr.link_tracks(A, None, xyz, B, 2 * n)
        link_ok = int((B["train"][link["src2d"]] == index[2][pa[link["src3d"]]]).sum())
        M = rt12(R12 @ R01, R12 @ t01 + t12)
        corr, _ = pm.match_projected(A, None, xyz, sets[1], sets[2], M, K, 4.0, (4, 5), True, 0)
        ok = int((corr["src2d"] == index[2][pa[corr["src3d"]]]).sum())
        print(f"effect n={n} seed={seed}: landmarks {len(A)}, link {link_ok} correct of {len(link)}, projected {ok} correct of {len(corr)}")
        assert ok - link_ok >= 0.1 * n, (seed, ok, link_ok)
        assert len(corr) - ok <= 0.01 * n, (seed, len(corr), ok)


def chain(synth, n, noise, seed, share=0.3, radius=CHAIN_RADIUS, ransac_seed=None, max_index=None):
    """the statement chain over one three_view_keypoints scene -> dict of every stage's outputs: 2-NN lists of (I0, I1) and
    (I1, I2), fundamental -> refit -> pose -> link -> PnP -> refit, then the re-match of the pose's points under the refitted pose
    and the refit over the re-matched list"""
    sc = synth.three_view_keypoints(seed, n, noise, share)
    K, sets = sc[0], sc[3]
    seed = seed if ransac_seed is None else ransac_seed
    max_index = 2 * n if max_index is None else max_index
    A, B = knn2_list(sets[0], sets[1]), knn2_list(sets[1], sets[2])
    rec0, _ = fr.find_fundamental(A, 256, 1.0, seed)
    rec1, _ = rr.refine_fundamental(A, rec0, 1.0, 3)
    pose, pmask, xyz = pr.recover_pose(A, rec1, K, None, 1.0, 50.0)
    corr = lr.link_tracks(A, pmask, xyz, B, max_index)
    abs2, _ = pn.solve_pnp(corr, K, 256, 2.0, seed)
    ref2, mask2 = pf.refine_pnp(corr, K, abs2, 2.0, 3)
    corrp, _ = pm.match_projected(A, pmask, xyz, sets[1], sets[2], ref2, K, radius, (4, 5), True, 0)
    ref3, mask3 = pf.refine_pnp(corrp, K, ref2, 2.0, 3)
    return dict(scene=sc, A=A, B=B, fund=rec1, pose=pose, pmask=pmask, xyz=xyz, corr=corr, abs2=abs2, ref2=ref2, mask2=mask2, corrp=corrp,
                ref3=ref3, mask3=mask3)


def test_chain_under_the_estimated_pose(synth):
    """the chain of the README's table on every leg; a line per leg is printed.  What is asserted is the rule's, not a measurement:
    every correspondence of the re-match lies in the gate of the pose it was searched under, and the refit over it never counts
    fewer inliers than that pose has on the same list"""
    for n, noise, seed in LEGS:
        c = chain(synth, n, noise, seed)
        K, (R01, t01), (R12, t12), sets, index, X0, look = c["scene"]
        pt = point_of(index, 2 * n)
        A, B, corr, corrp = c["A"], c["B"], c["corr"], c["corrp"]
        pa = pt[0][A["query"]]
        good_a = (pa >= 0) & (pt[1][A["train"]] == pa)
        want2 = np.where(good_a, index[2][np.maximum(pa, 0)], -2)           # the keypoint of I2 a landmark should get
        link_ok = int((B["train"][corr["src2d"]] == want2[corr["src3d"]]).sum())
        proj_ok = int((corrp["src2d"] == want2[corrp["src3d"]]).sum())
        scale = np.linalg.norm(t01)
        R02, t02 = R12 @ R01, R12 @ t01 + t12
        err = lambda r: (rot_angle(r["R"].reshape(3, 3), R02), dir_angle(r["t"], t02), float(np.linalg.norm(r["t"]) * scale / np.linalg.norm(t02)))
        (r2, d2, s2), (r3, d3, s3) = err(c["ref2"]), err(c["ref3"])
        print(f"projected n={n} noise={noise} seed={seed} radius={CHAIN_RADIUS}: link {len(corr)} / {link_ok} correct, projected "
              f"{len(corrp)} / {proj_ok} correct, refit inliers {c['ref2']['inliers']} -> {c['ref3']['inliers']}, rot / t-dir / |t| ratio "
              f"{r2:.3f} / {d2:.3f} / {s2:.4f} -> {r3:.3f} / {d3:.3f} / {s3:.4f}")
        assert c["ref2"]["hypothesis"] >= 0 and len(corrp) > 0
        px, py, zc = pm.project(np.stack([corrp["X"], corrp["Y"], corrp["Z"]], axis=1), pm.view(c["ref2"])[0], K)
        assert (zc > 0).all() and (np.hypot(corrp["u"] - px, corrp["v"] - py) < CHAIN_RADIUS * 1.001).all()
        rec = np.stack([corrp[f] for f in ("X", "Y", "Z", "u", "v")], axis=1)
        t2 = np.float32(2.0) * np.float32(2.0)
        before = int(pn.inlier_mask(pm.view(c["ref2"])[0], rec, pr.intrinsics(K), t2).sum())
        assert c["ref3"]["inliers"] >= before and c["ref3"]["n"] == len(corrp)
