"""The launch shapes of the two RANSAC estimators (hak_find_homography, hak_find_fundamental) as one committed case table, shared
by tests/test_ransac_shapes_cpu.py (what the cases reach, on the numpy statements alone) and tests/test_gpu_ransac_shapes.py (the
kernels against the statements, bit for bit).

Both estimators launch through one rule, hak_homography_blocks(npairs, iterations): a score block owns `hp` hypotheses (16 .. 256)
and a pair gets `hblocks` blocks.  The rule is NOT restated here: SHAPES records what it gave when the table was written, and the
CPU test asks the library (hak_op_ransac_shape) whether it still does.

A case is a pure function of (kind, entry): the lists, counts, stride, seed and threshold of one call.  Lists are small planted
scenes (test_homography_cpu.planted for "H", synth.two_view_matches for "F") whose records are ORDERED so that chosen hypotheses
draw nothing but planted records: the sampler is a function of (seed, h, n) alone, so the slots hypothesis h reads are known
before a list exists.  With few planted records among many random ones, the first hypothesis that draws only planted ones wins,
which puts the winner where a launch shape is weakest -- the last partial block, a block past the finish kernel's first trip over
the slots, two blocks that tie, or (homography) a hypothesis number past `iterations` that only a missing guard would score.
"""
import functools

import numpy as np

import fundamental_ref as fr
import homography_ref as hr

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
KINDS = ("H", "F")
SAMPLE = {"H": 4, "F": 7}
LONG = (1024, 1025, 2050)           # list lengths around RS_CHUNK = 1024 records
LONG_SHAPES = ((32, 129), (64, 257))

# (npairs, iterations) -> {pair: (target hypotheses, beyond)}.  The planted records of that pair's list sit on the slots the
# targets draw.  beyond: the targets lie past `iterations` inside the last block ("H" only: k_fund_score must not read a model
# past `iterations`, so "F" gets IN_RANGE's target instead).
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


def _planted_first(kind, n, k_in, s):
    """n records, the first k_in of them noise-free records of the planted model, the rest not"""
    if kind == "H":
        from test_homography_cpu import planted
        recs, inl, _ = planted(4 * n + 64, s, outlier_rate=0.5, noise=0.0, w=1920, h=1080)
        i_in, i_out = np.flatnonzero(inl)[:k_in], np.flatnonzero(~inl)[:n - k_in]
        assert len(i_in) == k_in and len(i_out) == n - k_in
        return np.concatenate([recs[i_in], recs[i_out]])
    from akaze_hip import synth
    recs, flags, _ = synth.two_view_matches(k_in, n - k_in, s)
    return np.concatenate([recs[flags], recs[~flags]])


def sample_slots(kind, seed, targets, n):
    """the distinct slots the target hypotheses draw from a list of n records, ascending"""
    idx, ok = (hr if kind == "H" else fr).sample_indices(seed, np.array(targets), n)
    assert ok.all()
    return np.unique(idx)


def make_list(kind, n, k_in, seed, targets, rng):
    """(n, 4) float32: k_in planted records (at least the slots the targets draw), the others random"""
    if n == 0:
        return np.zeros((0, 4), np.float32)
    slots = sample_slots(kind, seed, targets, n) if targets else np.zeros(0, np.int64)
    k_in = min(n, max(k_in, len(slots)))
    rest = np.setdiff1d(np.arange(n), slots)
    slots = np.concatenate([slots, rng.permutation(rest)[:k_in - len(slots)]]).astype(np.int64)
    src = _planted_first(kind, n, k_in, int(rng.integers(1 << 30)))
    out = np.empty((n, 4), np.float32)
    out[slots] = src[:k_in]
    out[np.setdiff1d(np.arange(n), slots)] = src[k_in:]
    return out


def _sizes(kind, iterations):
    """(n, planted records) of a list that carries targets: few enough planted ones that no earlier hypothesis is expected to
    draw only them, enough that the count stands clear of what random records reach by accident"""
    if kind == "H":
        return (120, 8) if iterations <= 2100 else (200, 9) if iterations <= 8200 else (300, 10)
    return (60, 12) if iterations <= 2100 else (100, 14) if iterations <= 8200 else (150, 18)


@functools.lru_cache(maxsize=None)
def shape_case(kind, e):
    """entry e of SHAPES for estimator `kind`: dict(npairs, iterations, hp, hblocks, seed, threshold, stride, counts (as the device
    reads them: one above the stride where npairs > 1), lists (the records the call may use, per pair), placed {pair: (targets,
    beyond)}).  Cached: the arrays are shared, leave them unchanged."""
    npairs, iterations, hp, hblocks = SHAPES[e]
    rng = np.random.default_rng([SEED, KINDS.index(kind), e])
    seed = int((0, 0xFFFFFFFF, 12345, int(rng.integers(0, 2 ** 32)))[e % 4])
    threshold = float(np.float32((3.0, 1.0, 2.5)[e % 3] if kind == "H" else (1.0, 0.5, 2.0)[e % 3]))
    placed = {}
    for pair, (targets, beyond) in PLACED[(npairs, iterations)].items():
        if beyond and kind == "F":
            targets, beyond = IN_RANGE[(npairs, iterations)], False
        placed[pair] = (targets, beyond)
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
            lists.append(make_list(kind, n, _sizes(kind, iterations)[1], seed, placed[pair][0], rng))
        else:                                                           # a planted scene in random order, 30 .. 80 % planted
            lists.append(make_list(kind, n, int(n * rng.uniform(0.3, 0.8)), seed, (), rng))
    return dict(npairs=npairs, iterations=iterations, hp=hp, hblocks=hblocks, seed=seed, threshold=threshold, stride=stride,
                counts=counts, lists=lists, placed=placed)


@functools.lru_cache(maxsize=None)
def statement(kind, e, refine=1):
    """the statement's (record, mask) of every pair of shape_case(kind, e); computed once per process"""
    c = shape_case(kind, e)
    if kind == "H":
        return [hr.find_homography(lst, c["iterations"], c["threshold"], c["seed"], bool(refine)) for lst in c["lists"]]
    return [fr.find_fundamental(lst, c["iterations"], c["threshold"], c["seed"]) for lst in c["lists"]]


def counts_of(kind, c, pair, hs):
    """the statement's inlier count of every model of hypotheses hs over the pair's list: (h of each model, count of each model)"""
    rec = hr.records(c["lists"][pair])
    t2 = np.float32(c["threshold"]) * np.float32(c["threshold"])
    hs = np.asarray(hs)
    if kind == "H":
        H, ok = hr.hypotheses(rec, c["seed"], hs)
        return hs[ok], hr.inlier_mask(H[ok], rec, t2).sum(axis=1)
    F, valid = fr.models(rec, c["seed"], hs)
    hh, rr = np.nonzero(valid)
    return hs[hh], fr.inlier_mask(F[hh, rr], rec, t2).sum(axis=1)


def shape_id(e):
    return f"{SHAPES[e][0]}x{SHAPES[e][1]}"
