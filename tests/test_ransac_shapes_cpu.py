"""CPU suite: the committed launch-shape cases of tests/ransac_shapes.py, held to what they claim on the numpy statements alone
(homography_ref, fundamental_ref, pnp_ref: three estimators) and on the library's own launch rule (hak_op_ransac_shape: no device is
touched).  The GPU side is tests/test_gpu_ransac_shapes.py.  These are conditions on the inputs, not measurements of the kernels: if
the launch rule changes, the table no longer covers what it says and the assertions here fail.  For "P" (hak_solve_pnp, four models
per hypothesis) the cases also reach every solution number as a winner, a tie between two models of one hypothesis, and lists past
the LDS chunk at every block size."""
import ctypes as C

import numpy as np
import pytest

import ransac_shapes as rs

# "P": the longest list of the entries whose placed list is longer than the 300 records of a batch's (the others: 300, or 2050 at
# LONG_SHAPES)
P_LONGEST = {(1, 2000): 2050, (1, 2047): 1025, (1, 4097): 2050, (1, 8192): 500, (1, 8200): 600, (1, 16385): 800, (1, 65536): 1000}

def shape_of(ah, npairs, iterations):
    hp, hb = C.c_int(-1), C.c_int(-1)
    ah.check(ah.lib.hak_op_ransac_shape(npairs, iterations, C.byref(hp), C.byref(hb)))
    return hp.value, hb.value


def test_shape_query(ah):
    """the table's (hp, hblocks) are the library's, every block size occurs, and the query refuses what the calls refuse"""
    for npairs, iterations, hp, hblocks in rs.SHAPES:
        assert shape_of(ah, npairs, iterations) == (hp, hblocks), (npairs, iterations)
    assert {s[2] for s in rs.SHAPES} == {16, 32, 64, 128, 256}          # (one table for all three estimators)
    assert sum(s[3] > 64 for s in rs.SHAPES) >= 6
    # the shapes the suite reached before this table: at most 64 blocks per pair
    assert shape_of(ah, 1, 1024) == (16, 64) and shape_of(ah, 1, 4096) == (64, 64) and shape_of(ah, 7, 1024) == (64, 16)
    assert shape_of(ah, 256, 1024) == (256, 4)                          # the shape every RANSAC figure under profiles/ was timed at
    hp, hb = C.c_int(), C.c_int()
    for bad in ((0, 10), (1, 0), (1, 65537)):
        assert ah.lib.hak_op_ransac_shape(*bad, C.byref(hp), C.byref(hb)) != 0
    assert ah.lib.hak_op_ransac_shape(1, 10, None, C.byref(hb)) != 0 and ah.lib.hak_last_error().decode() != ""


def test_cases_are_pure_and_ragged():
    for kind in rs.KINDS:
        rs.shape_case.cache_clear()
        a = rs.shape_case(kind, 6)
        rs.shape_case.cache_clear()
        b = rs.shape_case(kind, 6)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a["lists"], b["lists"])) and a["counts"] == b["counts"]
        for e, s in enumerate(rs.SHAPES):
            c = rs.shape_case(kind, e)
            assert (c["npairs"], c["iterations"]) == s[:2] and len(c["lists"]) == c["npairs"] == len(c["counts"])
            assert all(len(lst) == min(n, c["stride"]) for lst, n in zip(c["lists"], c["counts"]))
            assert all(np.isfinite(lst).all() for lst in c["lists"])
            if c["npairs"] > 1:
                assert {0, 3} <= set(c["counts"]) and max(c["counts"]) > c["stride"]
            big = max(len(lst) for lst in c["lists"])
            if kind == "P":                                             # the exact lengths: targets ride on lists past the LDS chunk
                assert all(lst.shape[1:] == (5,) for lst in c["lists"])
                assert big == (2050 if s[:2] in rs.LONG_SHAPES else P_LONGEST.get(s[:2], 300)), (s, big)
            else:
                assert big <= 300 or (s[:2] in rs.LONG_SHAPES and big == 2050)
        for s in rs.LONG_SHAPES:                                        # the LDS chunk edge at two slices (hp 128) and at one (hp 256)
            c = rs.shape_case(kind, [x[:2] for x in rs.SHAPES].index(s))
            assert set(rs.LONG) <= {len(lst) for lst in c["lists"]}
        assert {rs.shape_case(kind, rs.SHAPES.index(s))["hp"] for s in rs.SHAPES if s[:2] in rs.LONG_SHAPES} == {128, 256}


@pytest.mark.parametrize("kind", rs.KINDS)
def test_winners_sit_where_the_shapes_are_weak(kind):
    """(a) a winner in the last, partial block; (b) winners in a block >= 64 at three or more shapes; (c) at an hp >= 128 shape the
    winning count is reached in two different blocks, so the smallest-h rule is decided between slots; (d, homography) at a
    partial last block, the statement run over hblocks * hp hypotheses names a winner past `iterations`.  Every list that
    carries targets is won by its first target (or, past `iterations`, by none of them).
    "P" only: (e) the placed winners take every solution number 0 .. 3, one of 2 and 3 in a block >= 64; (f) on some list two
    models of the winning hypothesis reach the winning count and the record names the smaller; (g) lists reach past the 1024
    records of an LDS chunk at every hp, with an inlier of the winner beyond them (a score that stops at the chunk edge miscounts); (h) a placed list's inliers are its planted records, which makes the ties of (c) exact."""
    last_partial, late_blocks, two_block_ties, beyond = [], set(), [], []
    solutions, late_solutions, model_ties, long_hp = set(), set(), [], set()
    for e in range(len(rs.SHAPES)):
        c = rs.shape_case(kind, e)
        hp, hblocks, it = c["hp"], c["hblocks"], c["iterations"]
        st = rs.statement(kind, e, 0) if kind == "H" else rs.statement(kind, e)
        for pair, (r, mask) in enumerate(st):
            h = int(r["hypothesis"])
            assert r["n"] == len(c["lists"][pair]) == len(mask) and -1 <= h < it
            if h >= 0 and h // hp == hblocks - 1 and it % hp:
                last_partial.append((e, pair))
            if h // hp >= 64:
                late_blocks.add(e)
            if kind == "P":
                if mask[rs.CHUNK:].any():                               # (g): an inlier of the winner in a later chunk
                    long_hp.add(hp)
                if h >= 0:                                              # (f): the models of the winning hypothesis, ascending r
                    _, cnt, rr = rs.counts_of(kind, c, pair, [h], with_r=True)
                    assert cnt.max() == r["inliers"] and rr[np.argmax(cnt)] == r["solution"]
                    if (cnt == cnt.max()).sum() >= 2:
                        model_ties.append((e, pair))
        for pair, (targets, past) in c["placed"].items():
            r = st[pair][0]
            if not past:
                assert r["hypothesis"] == targets[0], (e, pair, r)
            if kind == "P":
                assert not past and r["inliers"] == c["planted"][pair] and r["solution"] == c["want"][pair], (e, pair, r)      # (h)
                solutions.add(int(r["solution"]))
                if targets[0] // hp >= 64:
                    late_solutions.add(int(r["solution"]))
            if len(targets) > 1 and hp >= 128:
                hs, cnt = rs.counts_of(kind, c, pair, np.arange(it))
                assert cnt.max() == r["inliers"] and hs[np.argmax(cnt)] == r["hypothesis"]
                blocks = set((hs[cnt == cnt.max()] // hp).tolist())
                assert {t // hp for t in targets} <= blocks
                if len(blocks) >= 2:
                    two_block_ties.append((e, pair))
            if past:
                assert kind == "H" and it % hp and it <= min(targets) and max(targets) < hblocks * hp
                import homography_ref as hr
                for refine in (False, True):
                    up, _ = hr.find_homography(c["lists"][pair], hblocks * hp, c["threshold"], c["seed"], refine)
                    assert up["hypothesis"] == targets[0] and up["inliers"] > r["inliers"]
                    assert up["H"].tobytes() != rs.statement(kind, e, int(refine))[pair][0]["H"].tobytes()
                beyond.append((e, pair))
    assert last_partial and len(late_blocks) >= 3 and two_block_ties, (last_partial, late_blocks, two_block_ties)
    assert all(rs.SHAPES[e][3] > 64 for e in late_blocks)
    assert len(late_blocks) >= 5                                        # (what the table delivers: 1025, 2000, 4097, 8200, 16385, 65536)
    if kind == "H":
        assert len(beyond) >= 2
    if kind == "P":
        assert solutions == {0, 1, 2, 3} and late_solutions & {2, 3}, (solutions, late_solutions)                  # (e)
        assert model_ties, "no list on which two models of the winning hypothesis tie"                               # (f)
        assert long_hp == {16, 32, 64, 128, 256}, long_hp                                                            # (g)
