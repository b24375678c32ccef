"""The matchers at the limits of their packed keys: train sets of up to 2^20 - 1 rows (every index bit of hak_mkey), 2047 LDS chunks
(every bit of the matrix-core kernel's chunk number q, its sixth P and the tail), up to 512 train slices, 1024 finish blocks.  The
families, shared by tests/test_match_limits_cpu.py (the expectations below against the oracle, and what the families reach) and
tests/test_gpu_match_limits.py (the kernels against the expectations, bit for bit).  Pure numpy: no GPU, no oracle.  At the end:
the gated matchers on skinny pairs (gated, and gated_blockwise, which evaluates their dense statements in blocks) and the helpers both
test modules share (the launch plan through hak_op_match_shape -- host arithmetic -- the family cache, the comparisons).

Test infrastructure.  A family is a train set from synth.random_descriptors with x = index, y = -index (match_x / match_y name the
row), a few rows of which are rewritten, and queries that are copies of train rows with exactly f flipped descriptor bits.  The
expected records follow from the construction and not from a search:

  * a GROUP is a handful of train rows that share one base descriptor: member (row, G) holds the base with the G bits
    400 .. 400 + G - 1 flipped (G = 0: an exact duplicate).  A query planted on the group is the base with f flipped bits among bits
    0 .. 399, so its distance to member (row, G) is exactly f + G.  Every group has a PARTNER (G > 0): the second neighbour of the 2-NN
    rule is then known as well.
  * every other (query, train) pair is a pair of independent uniform descriptors: 486 fair bits, mean 243, sigma 11; a distance
    below 96 is 13 sigma away.  The CPU module asserts against the oracle that none occurs (census: "far").

From a query's candidates {(row, distance)} the two rules of hak_internal.h are applied by hand: expect_match (the reference's
1-NN rule: residue classes row mod 16, accepted iff ONE class attains the minimum and it is < 96, the class's first row) and
expect_knn2 (nearest = smallest (distance, row), second = the next candidate's distance, ratio test, cross-check, list in query order).

The layout of k_match_mfma's block pass (kernels_match.hip) is restated here ONLY to choose where rows are planted: chunk_row()
names the row that tile P of chunk q holds.  The tests assert through hak_op_match_shape that the call took that path."""
import ctypes as C
import functools

import numpy as np

import akaze_hip as ah
import epipolar_match_ref as er
import guided_match_ref as gr
from akaze_hip import synth

NMAX = (1 << 20) - 1            # the largest set the entry points accept (hak_mkey_fits)
CHUNK = 192                     # rows of an LDS chunk of k_match_mfma (six tiles of 32)
MM_MAX_ROWS = 2047 * CHUNK      # 393 024: the largest train set of the matrix-core kernel
MAX_DIST = 96
QBITS = 400                     # queries flip bits below, group members bits from here on
FLIPS = (0, 1, 40, 95, 96, 97)
PARTNER_G = (10, 30, 60)
PAIR = np.dtype([("query", "<i4"), ("train", "<i4"), ("distance", "<i4"), ("second", "<i4"),
                 ("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4")])
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming(a, b):
    """Hamming distances of descriptor arrays (.., 61) uint8, broadcast"""
    return _POP[a ^ b].sum(axis=-1)


def _flip(feat, bits):
    for b in bits:
        feat[b >> 3] ^= np.uint8(1 << (b & 7))


class Family:
    """train set + queries + by-construction candidates; see the module docstring"""

    def __init__(self, name, n2, seed):
        self.name, self.seed = name, seed
        self.rng = np.random.default_rng([seed, n2])
        self.train = synth.random_descriptors(n2, seed, ah.POINT_DTYPE)
        self.train["x"] = np.arange(n2, dtype=np.float32)          # (exact: n2 < 2^24)
        self.train["y"] = -np.arange(n2, dtype=np.float32)
        self.used = {}                      # rewritten train row -> group
        self.groups = []                    # [(row, G), ...] per group
        self.base = []                      # base descriptor per group
        self.plan = []                      # per query: (group or -1, f, tag)
        self.free = 1000                    # partner rows are taken from here on (low indices: a partner is never reported)

    # ---- train side
    def _take(self, row, g):
        assert 0 <= row < len(self.train) and row not in self.used, (self.name, row)
        self.used[row] = g

    def group(self, rows, base=None, partner=True):
        """rows: the exact duplicates (the first keeps its random descriptor unless `base` is given) -> group number"""
        g = len(self.groups)
        for r in rows:
            self._take(r, g)
        feat = self.train["features"][rows[0]].copy() if base is None else np.asarray(base, np.uint8).copy()
        members = [(r, 0) for r in rows]
        if partner:
            while self.free in self.used or self.free % 16 == rows[0] % 16:
                self.free += 1
            self._take(self.free, g)
            members.append((self.free, PARTNER_G[g % len(PARTNER_G)]))
        for r, G in members:
            f = feat.copy()
            _flip(f, range(QBITS, QBITS + G))
            self.train["features"][r] = f
        self.groups.append(members)
        self.base.append(feat)
        return g

    # ---- query side
    def query(self, g, f, tag=""):
        self.plan.append((g, f, tag))

    def unplanted(self, n=1):
        for _ in range(n):
            self.plan.append((-1, 0, "unplanted"))

    def finish(self, n1, qseed, where=None):
        """n1 queries: the planned ones at positions `where` (default: the first ones), unplanted random descriptors elsewhere"""
        assert len(self.plan) <= n1, (self.name, len(self.plan), n1)
        self.queries = synth.random_descriptors(n1, qseed, ah.POINT_DTYPE)
        where = np.arange(len(self.plan)) if where is None else np.asarray(where)
        assert len(where) == len(self.plan) and len(np.unique(where)) == len(where) and where.max(initial=0) < n1
        self.where = where
        self.cands = {}                     # query -> [(row, distance)], ascending (distance, row)
        self.qplan = {}
        for (g, f, tag), i in zip(self.plan, where):
            self.qplan[int(i)] = (g, f, tag)
            if g < 0:
                continue
            feat = self.base[g].copy()
            _flip(feat, self.rng.choice(QBITS, f, replace=False))
            self.queries["features"][i] = feat
            self.cands[int(i)] = sorted((f + G, r) for r, G in self.groups[g])
        return self

    # ---- the rules, by hand
    def expect_match(self):
        """hak_match: the four match fields of every query"""
        n1 = len(self.queries)
        out = {"match": np.full(n1, -1, np.int32), "distance": np.full(n1, -1, np.int32),
               "match_x": np.full(n1, -1, np.float32), "match_y": np.full(n1, -1, np.float32)}
        for i, c in self.cands.items():
            dmin = c[0][0]
            rows = [r for d, r in c if d == dmin]
            if dmin < MAX_DIST and len({r % 16 for r in rows}) == 1:
                j = min(rows)
                out["match"][i], out["distance"][i] = j, dmin
                out["match_x"][i], out["match_y"][i] = self.train["x"][j], self.train["y"][j]
        return out

    def expect_knn2(self, ratio=(4, 5), cross=True, max_dist=MAX_DIST):
        """hak_match_knn2: (the four match fields of every query, the accepted list)"""
        n1 = len(self.queries)
        out = {"match": np.full(n1, -1, np.int32), "distance": np.full(n1, -1, np.int32),
               "match_x": np.full(n1, -1, np.float32), "match_y": np.full(n1, -1, np.float32)}
        nearest = {}                        # train row -> (distance, query): its nearest query among those that know it
        for i, c in self.cands.items():
            for d, r in c:
                if r not in nearest or (d, i) < nearest[r]:
                    nearest[r] = (d, i)
        lst = []
        for i in sorted(self.cands):
            c = self.cands[i]
            assert len(c) >= 2              # the second neighbour is known by construction
            (d1, j1), (d2, _) = c[0], c[1]
            ok = d1 < max_dist and d1 * ratio[1] < d2 * ratio[0]
            if ok and cross:
                ok = nearest[j1][1] == i
            if ok:
                out["match"][i], out["distance"][i] = j1, d1
                out["match_x"][i], out["match_y"][i] = self.train["x"][j1], self.train["y"][j1]
                lst.append((i, j1, d1, d2, self.queries["x"][i], self.queries["y"][i], self.train["x"][j1], self.train["y"][j1]))
        return out, np.array(lst, PAIR)

    # ---- what the family reaches
    def census(self):
        """accepted / tie-losing / rejected indices by kind, for the floors of the CPU module"""
        em = self.expect_match()
        acc = [int(em["match"][i]) for i in self.cands if em["match"][i] >= 0]
        losers, other_class = [], 0
        for i, c in self.cands.items():
            rows = [r for d, r in c if d == c[0][0]]
            if len(rows) > 1 and len({r % 16 for r in rows}) == 1 and c[0][0] < MAX_DIST:
                losers += sorted(rows)[1:]
            if len({r % 16 for r in rows}) > 1:
                other_class += 1
        return {"accepted": acc, "losers": losers, "other_class_ties": other_class,
                "accepted_d": {(int(em["distance"][i]), int(em["match"][i])) for i in self.cands if em["match"][i] >= 0},
                "rejected_d": {(c[0][0], c[0][1]) for i, c in self.cands.items() if em["match"][i] < 0 and len({r for d, r in c if d == c[0][0]}) == 1},
                "unplanted": [i for i, (g, f, t) in self.qplan.items() if g < 0]}


def bits_seen(indices, lo=14, hi=19):
    """{bit: (seen as 1, seen as 0)} over the indices"""
    return {b: (any(i >> b & 1 for i in indices), any(not (i >> b & 1) for i in indices)) for b in range(lo, hi + 1)}


# ------------------------------------------------------------------ index_bits
def index_bits(n2=NMAX, n1=129, seed=101):
    """every index bit 14 .. 19 set and clear in an accepted match, in the loser of a same-class tie and in a rejected other-class tie;
    d = 95 / 96 at the top of the set; an all-zero and an all-one row at high indices.  The first 33 planned queries hold one of each
    kind (n1 = 33: one query block with a second wave barely used; 129: two query blocks, a wave past n1).  Rows that n2 does not
    hold are left out (the `switch` family runs the same plan on smaller sets)."""
    F = Family("index_bits", n2, seed)
    fits = lambda r: r < n2 - 64
    single = {}

    def target(t):
        if t not in single:
            single[t] = F.group([t])
        return single[t]

    tb = [t for b in range(14, 20) for t in (1 << b, (1 << b) - 1) if fits(t)]
    top, top17 = target(n2 - 1), target(n2 - 17)
    same = [F.group([40 + b, 40 + b + (1 << b)]) for b in range(14, 20) if fits(40 + b + (1 << b))]
    other = [F.group([80 + b, 80 + b + (1 << b) + 1]) for b in range(14, 20) if fits(80 + b + (1 << b) + 1)]
    z = (1 << 19) + (1 << 14) + 5 if fits((1 << 19) + (1 << 14) + 5) else n2 // 2 + 5
    zero = np.zeros(61, np.uint8)
    ones = np.full(61, 0xFF, np.uint8)
    ones[60] = 0x3F
    gz, go = F.group([z], base=zero), F.group([n2 - 3], base=ones)
    # the first 33: one of each kind
    for k, t in enumerate(tb):
        F.query(target(t), FLIPS[k % 4], "bit")
    F.query(top, 95, "top")
    F.query(top17, 96, "top")
    for k, g in enumerate(same):
        F.query(g, FLIPS[(k + 1) % 4], "same")
    for k, g in enumerate(other):
        F.query(g, FLIPS[(k + 2) % 4], "other")
    F.query(gz, 0, "zero")
    F.query(go, 0, "ones")
    F.query(gz, 95, "zero")
    F.query(go, 96, "ones")
    F.unplanted(max(0, 33 - len(F.plan)))
    if n1 > 33:
        for t in (0, 15, 16383, 16384):
            for f in FLIPS:
                F.query(target(t), f, "low")
        for k, t in enumerate(tb):
            for f in (FLIPS[(k + 1) % 4], 96, 97):
                F.query(target(t), f, "bit")
        F.query(top, 96, "top")
        F.query(top17, 95, "top")
        for g in same:
            F.query(g, 96, "same")
        F.query(gz, 97, "zero")
        F.query(go, 1, "ones")
        F.unplanted(13)
    assert len(F.plan) <= n1, len(F.plan)
    return F.finish(n1, seed + 1)


# ------------------------------------------------------------------ chunks
CHUNK_Q = (0, 62, 63, 64, 127, 128, 1023, 1024, 2045, 2046)
TILE_ROWS = (0, 31, 4, 27)        # first / last row of a tile and of a lane half (rows 0-3, 8-11, .. | 4-7, 12-15, ..)


def chunk_row(n2, P, q, rho, jbeg=0):
    """the row that tile P (< 6; 6: the tail, q = its tile) of chunk q of a block pass over rows [jbeg, n2) holds at position rho of
    the tile; None when the pass has no such tile"""
    nrows = n2 - jbeg
    nq = nrows // CHUNK
    if P < 6:
        return jbeg + P * 32 * nq + 32 * q + rho if q < nq else None
    r = jbeg + CHUNK * nq + 32 * q + rho
    return r if r < n2 else None


def slice_of(row, rps):
    return row // rps


def chunks(n2=MM_MAX_ROWS, seams=(), seed=202):
    """targets in chunks CHUNK_Q of every sixth and in the tail of an unsliced block pass; same-class duplicate pairs whose order by
    (P, q) must equal their order by index; for every rows-per-slice in `seams` (from hak_op_match_shape) duplicate pairs in the first
    and the last slice and across the seams 7 | 8 and 63 | 64"""
    F = Family("chunks", n2, seed)
    F.hit = set()                           # (P, q) of the accepted targets
    k = 0
    for q in CHUNK_Q:
        for P in range(7):
            qq = q if P < 6 else CHUNK_Q.index(q)       # the tail has tiles 0 .. 5
            t = chunk_row(n2, P, qq, TILE_ROWS[(P + CHUNK_Q.index(q)) % 4])
            if t is None or t in F.used:
                continue
            g = F.group([t])
            F.query(g, (0, 1, 40, 95)[k % 4], "chunk")
            if k % 7 == 3:
                F.query(g, 96, "chunk")
            F.hit.add((P, qq))
            k += 1
    F.order = []
    nq = n2 // CHUNK
    pairs = [((1, 0), (0, nq - 1)), ((0, 1023), (0, 1024)), ((3, 0), (2, nq - 1)), ((5, nq - 1), (6, 0))]
    for n, (a, b) in enumerate(pairs):
        for rho, same in ((8 + n, True), (20 + n, False)):
            ra, rb = chunk_row(n2, a[0], a[1], rho), chunk_row(n2, b[0], b[1], rho + (0 if same else 1))
            if ra is None or rb is None:
                continue
            F.query(F.group(sorted((ra, rb))), (1, 40)[n % 2], "order" if same else "order other")
            if same:
                F.order.append((a, b))
    F.seams = {}
    for rps in seams:
        ns = (n2 + rps - 1) // rps
        got = []
        for lo, hi in ((0, 0), (ns - 1, ns - 1), (7, 8), (63, 64)):
            if hi >= ns:
                continue
            # a pair in the last rows of slice lo and the first rows of slice hi (lo == hi: both inside), 16 k apart: one class
            ra = min((lo + 1) * rps, n2) - 48 - 2 * len(F.seams)
            rb = hi * rps + 16 - 2 * len(F.seams) if lo != hi else ra + 32
            rb += (ra - rb) % 16
            for off, same in ((0, True), (1, False)):
                a, b = ra - 16 * off, rb + 17 * off
                if a in F.used or b in F.used or b >= n2:
                    continue
                F.query(F.group([a, b]), (0, 40)[off], "seam" if same else "seam other")
                if same:
                    got.append((slice_of(a, rps), slice_of(b, rps)))
        F.seams[rps] = got
    F.unplanted(3)
    return F.finish(len(F.plan), seed + 1)


# ------------------------------------------------------------------ many_queries
def many_queries(n2=64, n1=NMAX, seed=303):
    """2^20 - 1 queries against a small train set whose rows (2 k, 2 k + 1) are group and partner: the forward grid is capped and
    loops, the reverse search of the cross-check has the long train set, the 2-NN finish has 1024 blocks.  Planted queries in the
    first, the last and every 64th finish block; block 5 accepts all of its 1024 queries, block 700 some, most blocks none."""
    F = Family("many_queries", n2, seed)
    F.free = 1
    groups = []
    for k in range(0, n2 - 1, 2):
        F.free = k + 1
        groups.append(F.group([k]))
    where = []
    nb = (n1 + 1023) // 1024
    for b in sorted(set(range(0, nb, 64)) | {nb - 1}):
        last = min(1024 * b + 1023, n1 - 1)
        for n, i in enumerate((1024 * b, 1024 * b + 517, last)):
            F.query(groups[(len(where) // 3 + 17 * n) % len(groups)], (0, 3, 95)[n], "sparse")     # (f = 0: a group of its own, it wins the cross-check)
            where.append(i)
    # block 5: every query accepted without the cross-check (f < 4 G for every partner distance G >= 10: f <= 39); block 700: f = 1 .. 97
    for n in range(1024):
        F.query(groups[n % len(groups)], 2 + n % 38, "full")
        where.append(1024 * 5 + n)
    for n in range(1024):
        F.query(groups[(3 * n) % len(groups)], 1 + n % 97, "mixed")
        where.append(1024 * 700 + n)
    F.full_block, F.sparse_blocks = 5, sorted(set(range(0, nb, 64)) | {nb - 1})
    return F.finish(n1, seed + 1, where)


# ------------------------------------------------------------------ the gated matchers on skinny shapes
GATED_RATIO = (3, 2)            # d1 * 2 < d2 * 3: two gated candidates of EQUAL distance pass, so the list shows which index won the tie
GATED_RADIUS = 3.0
H_IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], np.float32)
F_ROWS = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], np.float32)       # the line of query (x, y) is the row y2 = y: e = y - y2, den = 1


def gated_blockwise(matcher, pts1, pts2, M, radius, ratio=(4, 5), cross_check=True, max_dist=0, block=1 << 15):
    """(block: rows per block of both axes, or (queries, train rows))  match_guided / match_epipolar (tests/guided_match_ref.py, tests/epipolar_match_ref.py) evaluated in blocks of both axes, for
    shapes whose dense (n1, n2) form does not fit: the statements' own `gate` per block; the Hamming distance of the gated pairs
    alone; forward, per query, the two smallest keys distance << 20 | train index as a running pair; reverse, per train point, the
    running minimum of distance << 20 | query index.  The accept rule is the statements'.  -> (out, pairs, why) as they return it"""
    gate = gr.gate if matcher == "guided" else er.gate
    n1, n2 = len(pts1), len(pts2)
    max_dist = 96 if max_dist <= 0 else int(max_dist)
    num, den = int(ratio[0]), int(ratio[1])
    out = pts1.copy()
    out["match"], out["distance"], out["match_x"], out["match_y"] = -1, -1, -1.0, -1.0
    why = np.ones(n1, np.int32)
    k1, k2 = np.full(n1, gr.NONE, np.int64), np.full(n1, gr.NONE, np.int64)
    rev = np.full(n2, gr.NONE, np.int64)
    bq, bt = block if isinstance(block, tuple) else (block, block)
    for i0 in range(0, n1, bq):
        a = pts1[i0:i0 + bq]
        for j0 in range(0, n2, bt):
            b = pts2[j0:j0 + bt]
            ii, jj = np.nonzero(gate(a, b, M, radius))
            if len(ii) == 0:
                continue
            d = hamming(a["features"][ii], b["features"][jj]).astype(np.int64)
            np.minimum.at(rev, jj + j0, (d << 20) | (ii + i0))
            key = (d << 20) | (jj + j0)                                      # (the keys of a query are distinct: they carry the index)
            order = np.lexsort((key, ii))
            qs, ks = ii[order] + i0, key[order]
            first = np.nonzero(np.r_[True, qs[1:] != qs[:-1]])[0]             # the block's smallest key of each of its queries ...
            q, a1 = qs[first], ks[first]
            nxt = np.minimum(first + 1, len(qs) - 1)
            a2 = np.where((first + 1 < len(qs)) & (qs[nxt] == q), ks[nxt], gr.NONE)      # ... and its second smallest
            k2[q] = np.minimum(np.minimum(np.maximum(k1[q], a1), k2[q]), a2)
            k1[q] = np.minimum(k1[q], a1)
    pairs = []
    for i in np.nonzero(k1 != gr.NONE)[0]:
        d1, j = int(k1[i] >> 20), int(k1[i] & 0xFFFFF)
        d2 = 512 if k2[i] == gr.NONE else int(k2[i] >> 20)
        if not d1 < max_dist:
            why[i] = 2
        elif not d1 * den < d2 * num:
            why[i] = 3
        elif cross_check and int(rev[j] & 0xFFFFF) != i:
            why[i] = 4
        else:
            why[i] = 0
            out["match"][i], out["distance"][i] = j, d1
            out["match_x"][i], out["match_y"][i] = pts2["x"][j], pts2["y"][j]
            pairs.append((i, j, d1, d2, pts1["x"][i], pts1["y"][i], pts2["x"][j], pts2["y"][j]))
    return out, np.array(pairs, gr.MATCH_PAIR_DTYPE), why


class Gated:
    """a skinny pair for both gated matchers; see gated()"""


def gated(long_queries, seed=404):
    """(64, 2^20 - 1) or, long_queries, (2^20 - 1, 64).  The long set lies on a lattice of pitch 16 (index k at (16 (k mod 1024),
    16 (k div 1024)), inside the epipolar domain of +-16384); the 64 points of the short set at (16 a + 8, 16 b + 8), one lattice row
    band each.  Under H = identity and under the F whose lines are the rows y2 = y, a lattice point is 8 or more from every projection
    and every line: more than two radii (radius 3).  Chosen points of the long set are then MOVED next to a point of the short set
    (offsets of 0.5 .. 1.5: inside both gates), their descriptors copies of its descriptor with a chosen number of flipped bits:
      forward (long train axis): a query gates train rows t and t + 2^b, b = 14 .. 19, with equal distances (the smaller index wins,
        and GATED_RATIO lets the tie pass), with the nearer one at the larger index, at the smaller index, or t + 2^b alone;
      reverse (long query axis): a train point is gated by queries s, s + 2^b, s + 2^b' of equal distance (the smallest wins the
        cross-check, the others lose it), or by a farther query at the smaller index and the nearest at the larger.
    Coordinates are multiples of 0.5 below 2^15: every float32 operation of both gates is exact.  What is expected comes from
    gated_blockwise (the statements), not from this construction; `planted` is kept for the census of the CPU module."""
    G = Gated()
    rng = np.random.default_rng([seed, int(long_queries)])
    lng = synth.random_descriptors(NMAX, seed + int(long_queries), ah.POINT_DTYPE)
    k = np.arange(NMAX)
    lng["x"], lng["y"] = (16 * (k % 1024)).astype(np.float32), (16 * (k // 1024)).astype(np.float32)
    sht = synth.random_descriptors(64, seed + 7, ah.POINT_DTYPE)
    s = np.arange(64)
    sht["x"], sht["y"] = np.float32(16 * 500 + 8), (16 * (10 + 15 * s) + 8).astype(np.float32)
    G.planted = []                          # (short index, [(long index, distance)], kind)
    taken = set()
    for i in range(60):
        b = 14 + i % 6
        kind = (i // 6) % 4
        b2 = 14 + (i + 1 + i // 6 % 5) % 6                                   # (never b: the step is 1 .. 5)
        e = 14 + (i + 3) % 6
        t = 1000 + 37 * i + ((1 << e) if i % 2 and e not in (b, b2) else 0)  # distinct bits: every index stays below 2^20
        f = int(rng.integers(0, 60))
        if not long_queries:
            members = [[(t, f), (t + (1 << b), f)], [(t, f + 1), (t + (1 << b), f)], [(t, f), (t + (1 << b), f + 1)], [(t + (1 << b), f)]][kind]
        else:
            hi2 = t + (1 << b) + (1 << b2)
            members = [[(t, f), (t + (1 << b), f), (hi2, f)], [(t, f + 2), (t + (1 << b), f)], [(t + (1 << b), f), (hi2, f)],
                       [(t + (1 << b), f)]][kind]
        for n, (r, d) in enumerate(members):
            assert r < NMAX and r not in taken
            taken.add(r)
            feat = sht["features"][i].copy()
            _flip(feat, rng.choice(486, d, replace=False))
            lng["features"][r] = feat
            lng["x"][r], lng["y"][r] = sht["x"][i] + np.float32(0.5 + 0.5 * n), sht["y"][i] + np.float32(0.5 * n - 0.5)
        G.planted.append((i, members, kind))
    G.pts1, G.pts2 = (lng, sht) if long_queries else (sht, lng)
    G.long_queries = long_queries
    return G


# ------------------------------------------------------------------ what both test modules share
FIELDS = ("match", "distance", "match_x", "match_y")
PLAN = ("kernel", "qt", "gx", "slices", "rows_per_slice", "chunks_per_slice", "finish_blocks")


def plan_of(search, n1, n2, npairs=1, device_counts=False, capacity=0, scratch=True):
    """the launch plan of a matcher call as a dict (PLAN), from the library's own rule under the HAK_MATCH_* variables of the moment"""
    v = (C.c_int * 7)()
    ah.check(ah.lib.hak_op_match_shape(search, n1, n2, npairs, int(device_counts), capacity, int(scratch), v))
    return dict(zip(PLAN, v))


def seam_rows(monkeypatch, n2, n1=85):
    """rows per slice of the two sliced runs of the chunks family: the default rule and a slice count that is no multiple of 8"""
    monkeypatch.setenv("HAK_MATCH_VALU", "0")
    monkeypatch.setenv("HAK_MATCH_QT", "1")
    monkeypatch.delenv("HAK_MATCH_SLICES", raising=False)
    a = plan_of(0, n1, n2)
    monkeypatch.setenv("HAK_MATCH_SLICES", "100")
    b = plan_of(0, n1, n2)
    monkeypatch.delenv("HAK_MATCH_SLICES")
    return a, b


@functools.lru_cache(maxsize=None)
def family(name, n2, arg=None):
    """a family, built once per process (the GPU module shares them between its kernel selections; nobody writes to one)"""
    if name == "index_bits":
        return index_bits(n2, arg or 129)
    if name == "chunks":
        return chunks(n2, arg or ())
    if name == "gated":
        return gated(bool(n2))
    return many_queries(n2)


@functools.lru_cache(maxsize=None)
def gated_statement(matcher, long_queries, cross):
    """the statement of a gated family, evaluated once per process"""
    G = family("gated", int(long_queries))
    return gated_blockwise(matcher, G.pts1, G.pts2, H_IDENTITY if matcher == "guided" else F_ROWS, GATED_RADIUS, GATED_RATIO, cross)


def assert_fields(got, want, what):
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), (what, f, np.nonzero(got[f] != want[f])[0][:8])


def assert_list(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for f in PAIR.names:
        assert np.array_equal(got[f], want[f]), (what, f, np.nonzero(got[f] != want[f])[0][:8])
