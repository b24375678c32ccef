"""The launch shapes of the three RANSAC estimators (hak_find_homography, hak_find_fundamental, hak_solve_pnp) as one committed case
table, shared by tests/test_ransac_shapes_cpu.py (what the cases reach, on the numpy statements alone) and
tests/test_gpu_ransac_shapes.py (the kernels against the statements, bit for bit).

All three estimators launch through one rule, hak_homography_blocks(npairs, iterations): a score block owns `hp` hypotheses (16 .. 256)
and a pair gets `hblocks` blocks.  The rule is NOT restated here: SHAPES records what it gave when the table was written, and the
CPU test asks the library (hak_op_ransac_shape) whether it still does.

A case is a pure function of (kind, entry): the lists, counts, stride, seed and threshold of one call.  Lists are small planted
scenes (test_homography_cpu.planted for "H", synth.two_view_matches for "F", noise-free projections of one pose for "P") whose
records are ORDERED so that chosen hypotheses
draw nothing but planted records: the sampler is a function of (seed, h, n) alone, so the slots hypothesis h reads are known
before a list exists.  With few planted records among many random ones, the first hypothesis that draws only planted ones wins,
which puts the winner where a launch shape is weakest -- the last partial block, a block past the finish kernel's first trip over
the slots, two blocks that tie, or (homography) a hypothesis number past `iterations` that only a missing guard would score.

What "P" adds (the P3P estimator is the only one with four models per hypothesis and with an LDS staging of its own): the planted
pose of a placed list is chosen so that it is solution WANT = 0, 1, 2 or 3 of the winning hypothesis, so the key's two model bits,
the score kernel's `valid >> r & 1` and the finish kernel's read of model r decide the record; the three-record lists of the ragged
batches are fitted by every solution of a hypothesis, so the smallest-r rule decides there; and the single-pair entries of hp = 16,
32 and 64 carry their target on lists past RS_CHUNK records (P_SIZES) with a planted record behind the chunk edge, so a winner's
count depends on the staging's later chunks at every hp.
"""
import functools

import numpy as np

import fundamental_ref as fr
import homography_ref as hr
import pnp_ref as pn
from pose_ref import intrinsics

# npairs, iterations, hp, hblocks (the last two as the rule gave them; asserted through hak_op_ransac_shape)
SHAPES = (
    (1, 1025, 16, 65),              # the smallest second trip of the finish kernels' slot loop
    (1, 2000, 16, 125),
    (1, 2047, 32, 64),              # the last block one hypothesis short
    (1, 4097, 64, 65),
    (1, 8192, 128, 64),
    (1, 8200, 128, 65),             # a last block of 8 hypotheses
    (32, 129, 128, 2),              # a last block of 1 hypothesis; lists across the LDS chunk edge at two slices
    (20, 700, 128, 6),
    (16, 1024, 256, 4),
    (64, 1, 256, 1),                # one live hypothesis among 256 threads
    (64, 257, 256, 2),              # lists across the LDS chunk edge at one slice
    (9, 1800, 256, 8),
    (1, 16385, 256, 65),
    (1, 65536, 256, 256),           # the iteration limit
)
KINDS = ("H", "F", "P")              # (KINDS.index(kind) seeds the cases: append, never reorder)
SAMPLE = {"H": 4, "F": 7, "P": 3}
WIDTH = {"H": 4, "F": 4, "P": 5}    # floats per record: {x1, y1, x2, y2} or {X, Y, Z, u, v}
CHUNK = 1024                        # RS_CHUNK: the records of one LDS chunk of the score kernels
LONG = (1024, 1025, 2050)           # list lengths around it
LONG_SHAPES = ((32, 129), (64, 257))

# (npairs, iterations) -> {pair: (target hypotheses, beyond)}.  The planted records of that pair's list sit on the slots the
# targets draw.  beyond: the targets lie past `iterations` inside the last block ("H" only: k_fund_score must not read a model
# past `iterations` and neither must k_pnp_score, so "F" and "P" get IN_RANGE's target instead).
PLACED = {
    (1, 1025): {0: ((1024,), False)},                   # block 64 of 65, the 1-hypothesis last block
    (1, 2000): {0: ((1999,), False)},                   # block 124
    (1, 2047): {0: ((2047,), True)},
    (1, 4097): {0: ((4096,), False)},                   # block 64, partial
    (1, 8192): {0: ((8000, 8100), False)},              # blocks 62 and 63 tie
    (1, 8200): {0: ((8195,), False)},                   # block 64, partial
    (32, 129): {5: ((200,), True), 7: ((128,), False)},
    (20, 700): {3: ((500, 690), False)},                # blocks 3 and 5 tie
    (16, 1024): {2: ((700, 900), False)},               # blocks 2 and 3 tie
    (64, 1): {k: ((0,), False) for k in (4, 9, 33, 63)},
    (64, 257): {6: ((256,), False)},                    # the 1-hypothesis last block
    (9, 1800): {4: ((1799,), False)},                   # block 7, partial
    (1, 16385): {0: ((16384,), False)},                 # block 64, the 1-hypothesis last block
    (1, 65536): {0: ((65000,), False)},                 # block 253
}
IN_RANGE = {(1, 2047): (2046,), (32, 129): (100,)}
SEED = 20261

# "P": the camera of the scenes (test_gpu_pnp.scene: image 1920 x 1080, focal 1500, depths 4 .. 12)
P_W, P_H, P_FOCAL = 1920, 1080, 1500.0
K_TABLE = (P_FOCAL, P_FOCAL, P_W / 2.0, P_H / 2.0)
# "P": (npairs, iterations) -> the solution number (0 .. 3) of the planted pose among the models of the list's first target, per
# placed pair in ascending order.  P3P puts the true pose at solution 2 or 3 for about one sample in twenty, so make_list walks
# scene seeds until the target's sample does.  2 and 3 win in blocks >= 64 at 1025, 2000, 8200 and 65536 iterations.
WANT = {(1, 1025): (2,), (1, 2000): (3,), (1, 2047): (1,), (1, 4097): (0,), (1, 8192): (2,), (1, 8200): (3,), (32, 129): (1, 0),
        (20, 700): (0,), (16, 1024): (3,), (64, 1): (0, 1, 2, 3), (64, 257): (2,), (9, 1800): (1,), (1, 16385): (0,), (1, 65536): (3,)}
# "P": iterations -> (n, planted records) of the single lists that carry a target across the LDS chunk edge at hp = 16, 32, 64;
# at 8200 iterations the 500 records of _sizes let hypothesis 1379 of that entry's seed draw three planted ones, 600 do not
P_SIZES = {2000: (2050, 12), 2047: (1025, 12), 4097: (2050, 12), 8200: (600, 9)}
WALK = 2000                          # scene seeds tried per placed "P" list (some tens are needed)


def _planted_first(kind, n, k_in, s):
    """n records, the first k_in of them noise-free records of the planted model, the rest not"""
    if kind == "H":
        from test_homography_cpu import planted
        recs, inl, _ = planted(4 * n + 64, s, outlier_rate=0.5, noise=0.0, w=1920, h=1080)
        i_in, i_out = np.flatnonzero(inl)[:k_in], np.flatnonzero(~inl)[:n - k_in]
        assert len(i_in) == k_in and len(i_out) == n - k_in
        return np.concatenate([recs[i_in], recs[i_out]])
    from akaze_hip import synth
    if kind == "P":                                                     # one pose; the unplanted keep their point, not their pixel
        rng = np.random.default_rng([7000, s])
        R, t = synth.rotation_zyx(rng.uniform(-20, 20, 3)), rng.uniform(-1, 1, 3)
        z = rng.uniform(4.0, 12.0, n)
        uv = np.stack([rng.uniform(0, P_W, n), rng.uniform(0, P_H, n)], axis=1)
        Xc = np.stack([(uv[:, 0] - P_W / 2.0) / P_FOCAL * z, (uv[:, 1] - P_H / 2.0) / P_FOCAL * z, z], axis=1)
        uv[k_in:] = np.stack([rng.uniform(0, P_W, n), rng.uniform(0, P_H, n)], axis=1)[k_in:]
        return np.concatenate([(Xc - t) @ R, uv], axis=1).astype(np.float32)
    recs, flags, _ = synth.two_view_matches(k_in, n - k_in, s)
    return np.concatenate([recs[flags], recs[~flags]])


def sample_slots(kind, seed, targets, n):
    """the distinct slots the target hypotheses draw from a list of n records, ascending"""
    idx, ok = {"H": hr, "F": fr, "P": pn}[kind].sample_indices(seed, np.array(targets), n)
    assert ok.all()
    return np.unique(idx)


def _solution_of_planted(lst, k_in, seed, threshold, target):
    """"P": the solution number of target's model that the statement would pick (most inliers, then the smallest) if exactly the
    k_in planted records of lst pass it, else -1"""
    rec, K = pn.records(lst), intrinsics(K_TABLE)
    M, valid = pn.models(rec, K, seed, [target])
    if not valid[0].any():
        return -1
    t2 = np.float32(threshold) * np.float32(threshold)
    cnt = np.where(valid[0], pn.inlier_mask(M[0], rec, K, t2).sum(axis=1), -1)
    return int(np.argmax(cnt)) if cnt.max() == k_in else -1


def make_list(kind, n, k_in, seed, targets, rng, want=None, threshold=None):
    """(n, 4) float32, for "P" (n, 5): k_in planted records (at least the slots the targets draw), the others random.  "P" with
    want = r: the scene seed is walked until the planted pose is solution r of targets[0] and the best model of every target is
    passed by the planted records and no others"""
    if n == 0:
        return np.zeros((0, WIDTH[kind]), np.float32)
    slots = sample_slots(kind, seed, targets, n) if targets else np.zeros(0, np.int64)
    k_in = min(n, max(k_in, len(slots)))
    rest = np.setdiff1d(np.arange(n), slots)
    slots = np.concatenate([slots, rng.permutation(rest)[:k_in - len(slots)]]).astype(np.int64)
    if kind == "P" and targets and n > CHUNK and not (slots >= CHUNK).any():
        assert k_in > 3 * len(targets)                                  # (the last slot is no target's)
        slots[-1] = n - 1                                               # a planted record, so an inlier of the winner, past the chunk edge
    s0 = int(rng.integers(1 << 30))
    others = np.setdiff1d(np.arange(n), slots)
    for s in range(s0, s0 + (1 if want is None else WALK)):
        src = _planted_first(kind, n, k_in, s)
        out = np.empty((n, WIDTH[kind]), np.float32)
        out[slots] = src[:k_in]
        out[others] = src[k_in:]
        if want is None or (_solution_of_planted(out, k_in, seed, threshold, targets[0]) == want and
                            all(_solution_of_planted(out, k_in, seed, threshold, t) >= 0 for t in targets[1:])):
            return out
    raise AssertionError(("no scene puts the planted pose at solution", want, "of hypothesis", targets[0]))


def _sizes(kind, iterations):
    """(n, planted records) of a list that carries targets: few enough planted ones that no earlier hypothesis is expected to
    draw only them, enough that the count stands clear of what random records reach by accident"""
    if kind == "H":
        return (120, 8) if iterations <= 2100 else (200, 9) if iterations <= 8200 else (300, 10)
    if kind == "P":                                                     # a sample of three: a smaller planted share
        return P_SIZES.get(iterations) or ((300, 8) if iterations <= 2100 else (500, 9) if iterations <= 8200 else
                                           (800, 10) if iterations <= 16385 else (1000, 10))
    return (60, 12) if iterations <= 2100 else (100, 14) if iterations <= 8200 else (150, 18)


@functools.lru_cache(maxsize=None)
def shape_case(kind, e):
    """entry e of SHAPES for estimator `kind`: dict(npairs, iterations, hp, hblocks, seed, threshold, stride, counts (as the device
    reads them: one above the stride where npairs > 1), lists (the records the call may use, per pair), placed {pair: (targets,
    beyond), planted {pair: the number of planted records of a placed list}, for "P" want {pair: the solution number the planted
    pose takes at targets[0]}).  Cached: the arrays are shared, leave them unchanged."""
    npairs, iterations, hp, hblocks = SHAPES[e]
    rng = np.random.default_rng([SEED, KINDS.index(kind), e])
    seed = int((0, 0xFFFFFFFF, 12345, int(rng.integers(0, 2 ** 32)))[e % 4])
    threshold = float(np.float32((3.0, 1.0, 2.5)[e % 3] if kind == "H" else (1.0, 0.5, 2.0)[e % 3]))
    placed, want = {}, {}
    for pair, (targets, beyond) in PLACED[(npairs, iterations)].items():
        if beyond and kind != "H":
            targets, beyond = IN_RANGE[(npairs, iterations)], False
        placed[pair] = (targets, beyond)
        if kind == "P":
            want[pair] = WANT[(npairs, iterations)][len(want)]
    few = SAMPLE[kind]
    ns = []
    for pair in range(npairs):
        if pair in placed:
            ns.append(_sizes(kind, iterations)[0])
        elif npairs == 1:
            ns.append(120)
        else:
            ns.append(int((0, 3, few, few + 1, 33, 64, 65, 100, 127, 200, 256, 300, int(rng.integers(few, 300)))[(pair + e) % 13]))
    if (npairs, iterations) in LONG_SHAPES:
        free = [p for p in range(npairs) if p not in placed]
        for p, n in zip(free[1:4], LONG):
            ns[p] = n
    stride = max(ns)
    counts = list(ns)
    if npairs > 1:                                                      # a count above the stride: the call clamps it
        p = max(p for p in range(npairs) if p not in placed)
        ns[p], counts[p] = stride, stride + 50
    lists = []
    for pair, n in enumerate(ns):
        if pair in placed:
            lists.append(make_list(kind, n, _sizes(kind, iterations)[1], seed, placed[pair][0], rng, want.get(pair), threshold))
        else:                                                           # a planted scene in random order, 30 .. 80 % planted
            lists.append(make_list(kind, n, int(n * rng.uniform(0.3, 0.8)), seed, (), rng))
    return dict(npairs=npairs, iterations=iterations, hp=hp, hblocks=hblocks, seed=seed, threshold=threshold, stride=stride,
                counts=counts, lists=lists, placed=placed, want=want,
                planted={p: max(_sizes(kind, iterations)[1], len(sample_slots(kind, seed, placed[p][0], ns[p]))) for p in placed})


@functools.lru_cache(maxsize=None)
def statement(kind, e, refine=1):
    """the statement's (record, mask) of every pair of shape_case(kind, e); computed once per process"""
    c = shape_case(kind, e)
    if kind == "H":
        return [hr.find_homography(lst, c["iterations"], c["threshold"], c["seed"], bool(refine)) for lst in c["lists"]]
    if kind == "P":
        return [pn.solve_pnp(lst, K_TABLE, c["iterations"], c["threshold"], c["seed"]) for lst in c["lists"]]
    return [fr.find_fundamental(lst, c["iterations"], c["threshold"], c["seed"]) for lst in c["lists"]]


def counts_of(kind, c, pair, hs, with_r=False):
    """the statement's inlier count of every model of hypotheses hs over the pair's list: (h of each model, count of each model);
    with_r ("F", "P"): and the number r of each model within its hypothesis"""
    t2 = np.float32(c["threshold"]) * np.float32(c["threshold"])
    hs = np.asarray(hs)
    if kind == "P":
        rec, K = pn.records(c["lists"][pair]), intrinsics(K_TABLE)
        M, valid = pn.models(rec, K, c["seed"], hs)
        hh, rr = np.nonzero(valid)
        cnt = np.concatenate([pn.inlier_mask(M[hh[k:k + 256], rr[k:k + 256]], rec, K, t2).sum(axis=1) for k in range(0, len(hh), 256)] +
                             [np.zeros(0, np.int64)])
        return (hs[hh], cnt, rr) if with_r else (hs[hh], cnt)
    rec = hr.records(c["lists"][pair])
    if kind == "H":
        H, ok = hr.hypotheses(rec, c["seed"], hs)
        return hs[ok], hr.inlier_mask(H[ok], rec, t2).sum(axis=1)
    F, valid = fr.models(rec, c["seed"], hs)
    hh, rr = np.nonzero(valid)
    cnt = fr.inlier_mask(F[hh, rr], rec, t2).sum(axis=1)
    return (hs[hh], cnt, rr) if with_r else (hs[hh], cnt)


def shape_id(e):
    return f"{SHAPES[e][0]}x{SHAPES[e][1]}"
