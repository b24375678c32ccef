"""CPU suite: the families of tests/match_limits.py held to what they claim, on the statements alone.  The expectations that the
families derive from their construction equal the oracle (okz.match, okz.match_knn2), field for field; the census floors below keep a
later change of a generator from thinning what the families reach; and the library's launch rule (hak_op_match_shape: host
arithmetic, no device is touched) names for every case the path it was made for.  The GPU side is tests/test_gpu_match_limits.py.
Measured times: profiles/match_limits.txt."""
import ctypes as C

import numpy as np
import pytest

import epipolar_match_ref as er  # noqa: F401
import fuzz_gated as fg
import match_limits as ml

from match_limits import assert_fields, assert_list, family, plan_of, seam_rows


def held_to_oracle(okz, F, knn=((True,),)):
    q = F.queries.copy()
    okz.match(q, F.train)
    assert_fields(q, F.expect_match(), F.name + " 1-NN")
    for cross in knn[0]:
        q = F.queries.copy()
        lst = okz.match_knn2(q, F.train, (4, 5), cross)
        want, wlst = F.expect_knn2((4, 5), cross)
        assert_fields(q, want, f"{F.name} 2-NN cross={cross}")
        assert_list(lst, wlst, f"{F.name} 2-NN cross={cross}")
        assert 0 < len(wlst) < len(F.cands)                       # both outcomes of the 2-NN rule


@pytest.mark.parametrize("n2,n1", [(ml.NMAX, 129), (ml.NMAX, 33), (ml.MM_MAX_ROWS, 129), (ml.MM_MAX_ROWS + 1, 129)])
def test_index_bits_expectation_is_the_oracle(okz, n2, n1):
    held_to_oracle(okz, family("index_bits", n2, n1))


@pytest.mark.parametrize("n2", [ml.MM_MAX_ROWS, ml.MM_MAX_ROWS - 1])
def test_chunks_expectation_is_the_oracle(ah, okz, monkeypatch, n2):
    a, b = seam_rows(monkeypatch, n2)
    held_to_oracle(okz, family("chunks", n2, (a["rows_per_slice"], b["rows_per_slice"])))


@pytest.mark.parametrize("n2", [64, 300])
def test_many_queries_match_is_the_oracle(okz, n2):
    held_to_oracle(okz, family("many_queries", n2), knn=((),))


@pytest.mark.parametrize("n2", [64, 300])
def test_many_queries_knn2_is_the_oracle(okz, n2):
    """(the oracle's cross-check searches all 2^20 - 1 queries again for EVERY query that passes the ratio test, minutes for this
    family.  The same search of the oracle is therefore asked once per train row that a forward match names -- okz.match_knn2 with
    the sets exchanged reports the nearest query of each, smallest index among equal distances -- and the cross-check applied to
    the oracle's forward list)"""
    F = family("many_queries", n2)
    q = F.queries.copy()
    fwd = okz.match_knn2(q, F.train, (4, 5), False)
    want, wlst = F.expect_knn2((4, 5), False)
    assert_fields(q, want, "many_queries 2-NN")
    assert_list(fwd, wlst, "many_queries 2-NN")
    rows = np.unique(fwd["train"])
    back = okz.match_knn2(F.train[rows].copy(), F.queries, (1000, 1), False, 600)     # (d1 < 1000 d2: every row is listed)
    assert np.array_equal(back["query"], np.arange(len(rows)))
    rev = np.full(n2, -1, np.int64)
    rev[rows] = back["train"]
    lst = fwd[rev[fwd["train"]] == fwd["query"]]
    want, wlst = F.expect_knn2((4, 5), True)
    assert_list(lst, wlst, "many_queries 2-NN cross-checked")
    assert np.array_equal(np.nonzero(want["match"] >= 0)[0], lst["query"]) and np.array_equal(want["match"][lst["query"]], lst["train"])
    assert 0 < len(lst) <= n2 < len(fwd)


def test_unplanted_pairs_are_far(okz):
    """what keeps the hand expectation valid: a query that was not planted has no neighbour below 96 in the whole train set (for the
    planted ones the oracle's `second` in the tests above says the same of every row their candidates do not list)"""
    for F in (family("index_bits", ml.NMAX, 129), family("chunks", ml.MM_MAX_ROWS, ()), family("many_queries", 64), family("many_queries", 300)):
        free = np.setdiff1d(np.arange(len(F.queries)), np.fromiter(F.cands, int))[:2000]
        assert len(free) >= (16 if F.name == "index_bits" else 3)
        lst = okz.match_knn2(F.queries[free].copy(), F.train, (1000, 1), False, 600)      # (every query with a neighbour is listed)
        assert len(lst) == len(free) and lst["distance"].min() >= ml.MAX_DIST, (F.name, len(lst), lst["distance"].min())


def test_census_index_bits():
    F = family("index_bits", ml.NMAX, 129)
    c = F.census()
    for what in ("accepted", "losers"):
        for b, (one, zero) in ml.bits_seen(c[what]).items():
            assert one and zero, (what, b)
    assert c["other_class_ties"] >= 6
    assert any(d == 95 and j >= 1 << 19 for d, j in c["accepted_d"]) and any(d == 96 and j >= 1 << 19 for d, j in c["rejected_d"])
    assert {0, 1, 40, 95} <= {d for d, _ in c["accepted_d"]} and {96, 97} <= {d for d, _ in c["rejected_d"]}
    assert len(c["unplanted"]) >= 16
    # the reverse search of the cross-check: the query that wins a train row and one that loses it, at train indices with every bit
    # set and clear (the reverse keys carry QUERY indices below 129; their high bits are the many_queries family's)
    want, lst = F.expect_knn2((4, 5), True)
    for b, (one, zero) in ml.bits_seen(lst["train"]).items():
        assert one and zero, ("cross-checked", b)
    _, nocross = F.expect_knn2((4, 5), False)
    assert len(lst) < len(nocross)                                # the cross-check rejects some
    # the first 33 queries alone: every bit in an accepted match and in a tie's loser as well
    c33 = family("index_bits", ml.NMAX, 33).census()
    for what in ("accepted", "losers"):
        for b, (one, zero) in ml.bits_seen(c33[what]).items():
            assert one and zero, (33, what, b)
    assert c33["other_class_ties"] >= 6 and len(c33["unplanted"]) >= 3


def test_census_chunks(ah, monkeypatch):
    for n2 in (ml.MM_MAX_ROWS, ml.MM_MAX_ROWS - 1):
        a, b = seam_rows(monkeypatch, n2)
        assert a["slices"] == 512 and b["slices"] > 64 and b["slices"] % 8 != 0, (a, b)
        F = family("chunks", n2, (a["rows_per_slice"], b["rows_per_slice"]))
        assert len(F.queries) <= 128                              # one query block: gx = 1, the default rule gives 512 slices
        nq = n2 // ml.CHUNK
        for q in ml.CHUNK_Q:
            if q < nq:
                assert {(P, q) for P in range(6)} <= F.hit, (n2, q)
        if n2 % ml.CHUNK:
            assert {(6, k) for k in range((n2 % ml.CHUNK + 31) // 32)} <= F.hit, n2
            assert ((5, nq - 1), (6, 0)) in F.order
        assert {((1, 0), (0, nq - 1)), ((0, 1023), (0, 1024))} <= set(F.order)
        for rps, ns in ((a["rows_per_slice"], a["slices"]), (b["rows_per_slice"], b["slices"])):
            assert {(0, 0), (ns - 1, ns - 1), (7, 8), (63, 64)} <= set(F.seams[rps]), (n2, rps, F.seams[rps])
        c = F.census()
        assert c["other_class_ties"] >= 8 and len(c["losers"]) >= 8
        em = F.expect_match()
        # the order pairs are accepted with the smaller index, which is NOT the smaller (P, q) read the other way round
        for i, (g, f, tag) in F.qplan.items():
            if tag in ("order", "seam"):
                assert em["match"][i] == min(r for r, G in F.groups[g] if G == 0)
            if tag in ("order other", "seam other"):
                assert em["match"][i] == -1


def test_census_many_queries():
    for n2 in (64, 300):
        F = family("many_queries", n2)
        assert len(F.queries) == ml.NMAX
        for cross in (False, True):
            want, lst = F.expect_knn2((4, 5), cross)
            blocks = np.bincount(lst["query"] >> 10, minlength=1024)
            assert (blocks[F.sparse_blocks] >= 1).all() and (blocks == 0).sum() >= 900, cross
            assert (blocks[F.full_block] == 1024) == (not cross)
            assert 0 < blocks[700] < 1024
        # reverse keys (the cross-check's search: train rows against 2^20 - 1 queries): a winning query with every high bit set, clear
        for b, (one, zero) in ml.bits_seen(lst["query"]).items():
            assert one and zero, ("reverse", b)
        em = F.expect_match()
        assert (em["match"][F.where] >= 0).sum() > 1024 and (em["match"][F.where] < 0).sum() > 10


def test_families_are_a_pure_function_of_their_seed():
    for lq in (False, True):
        a, b = ml.gated(lq), ml.gated(lq)
        assert a.pts1.tobytes() == b.pts1.tobytes() and a.pts2.tobytes() == b.pts2.tobytes() and a.planted == b.planted
    for make in (lambda: ml.index_bits(ml.MM_MAX_ROWS + 1, 129), lambda: ml.chunks(ml.MM_MAX_ROWS - 1, (768, 4032)),
                 lambda: ml.many_queries(64)):
        a, b = make(), make()
        assert a.train.tobytes() == b.train.tobytes() and a.queries.tobytes() == b.queries.tobytes() and a.cands == b.cands
    assert ml.index_bits(4096 * 100, 129, seed=5).queries.tobytes() != ml.index_bits(4096 * 100, 129, seed=6).queries.tobytes()


def test_plan_names_the_paths(ah, monkeypatch):
    """the launch rule at the sizes the families use (host arithmetic: the GPU module asserts the same before every comparison)"""
    monkeypatch.setenv("HAK_MATCH_QT", "1")
    monkeypatch.delenv("HAK_MATCH_SLICES", raising=False)
    monkeypatch.setenv("HAK_MATCH_VALU", "0")
    for search in (0, 1):
        p = plan_of(search, 33, ml.MM_MAX_ROWS)
        assert (p["kernel"], p["gx"], p["slices"], p["rows_per_slice"], p["chunks_per_slice"]) == (0, 1, 512, 768, 4), p
        for n2 in (ml.MM_MAX_ROWS + 1, ml.NMAX):
            assert plan_of(search, 129, n2)["kernel"] == 1
        p = plan_of(search, ml.NMAX, 64)
        assert (p["kernel"], p["gx"], p["slices"], p["finish_blocks"]) == (0, 4096, 1, 1024), p
        assert plan_of(search, ml.NMAX, 64, scratch=False)["finish_blocks"] == 1
        p = plan_of(search, 0, 0, npairs=1, device_counts=True, capacity=ml.MM_MAX_ROWS)
        assert p["kernel"] == 0 and p["slices"] == (8 if search == 0 else 1) and p["finish_blocks"] == 1, p
        assert plan_of(search, 0, 0, npairs=1, device_counts=True, capacity=ml.MM_MAX_ROWS + 1)["kernel"] == 1
    monkeypatch.setenv("HAK_MATCH_SLICES", "1")
    p = plan_of(0, 33, ml.MM_MAX_ROWS)
    assert (p["kernel"], p["slices"], p["chunks_per_slice"]) == (0, 1, 2047), p
    p = plan_of(0, 33, ml.MM_MAX_ROWS - 1)
    assert (p["kernel"], p["slices"], p["chunks_per_slice"]) == (0, 1, 2047), p     # 2046 whole chunks and the tail
    monkeypatch.setenv("HAK_MATCH_VALU", "1")
    monkeypatch.delenv("HAK_MATCH_SLICES")
    p = plan_of(0, 129, ml.NMAX)
    assert p["kernel"] == 1 and p["slices"] > 1 and p["rows_per_slice"] % 128 == 0, p
    assert plan_of(1, 129, ml.NMAX)["kernel"] == 1
    bad = (C.c_int * 7)()
    assert ah.lib.hak_op_match_shape(2, 1, 1, 1, 0, 0, 1, bad) != 0 and ah.lib.hak_op_match_shape(0, 1, 1, 1, 0, 0, 1, None) != 0


# ------------------------------------------------------------------ the gated matchers
def test_blockwise_gated_driver_is_the_dense_statement(ah):
    """ml.gated_blockwise against match_guided / match_epipolar on the committed gated fuzz family (tests/fuzz_gated.py, seed 3),
    wherever the dense (n1, n2) form fits: records, lists and reasons, byte for byte, in blocks of 97 x 211 and in one block"""
    seen = {"guided": 0, "epipolar": 0}
    multi = accepted = 0
    for i in range(60):
        c = fg.draw_case(3, i)
        m = fg.make_case(c, ah.POINT_DTYPE)
        n1, n2 = len(m["q"]), len(m["t"])
        if n1 * n2 > 400_000:
            continue
        wout, wlist, wwhy = fg.statement(c, m)
        for blk in ((97, 211), (1 << 15, 1 << 15)):
            out, lst, why = ml.gated_blockwise(c["matcher"], m["q"], m["t"], m["M"], m["radius"], c["ratio"], bool(c["cross"]), c["max_dist"],
                                               block=blk)
            assert out.tobytes() == wout.tobytes() and lst.tobytes() == wlist.tobytes() and np.array_equal(why, wwhy), (i, blk)
        seen[c["matcher"]] += 1
        multi += n1 > 97 and n2 > 211
        accepted += len(wlist)
    assert min(seen.values()) >= 10 and multi >= 10 and accepted >= 500, (seen, multi, accepted)


@pytest.mark.parametrize("matcher", ["guided", "epipolar"])
def test_census_gated(matcher):
    """what the skinny gated families reach, on the statements alone: the construction's winners are the statements' winners, every
    index bit 14 .. 19 is set and clear in a forward winner, in the loser of a forward tie, in a reverse (cross-check) winner and in
    a query that loses the cross-check; nothing but the planted pairs is inside a gate"""
    # ---- the long train axis: forward keys
    G = family("gated", 0)
    out, lst, why = ml.gated_statement(matcher, False, True)
    want = {i: min(m, key=lambda rd: (rd[1], rd[0])) for i, m, kind in G.planted}
    assert np.array_equal(lst["query"], sorted(want)) and (why == 1).sum() == 64 - len(want)
    assert [int(j) for j in lst["train"]] == [want[i][0] for i in sorted(want)]
    assert [int(d) for d in lst["distance"]] == [want[i][1] for i in sorted(want)]
    for b, (one, zero) in ml.bits_seen(lst["train"]).items():
        assert one and zero, ("forward winner", b)
    losers = [r for i, m, kind in G.planted for r, d in m if r != want[i][0]]
    for b, (one, zero) in ml.bits_seen(losers).items():
        assert one and zero, ("forward loser", b)
    ties = [(i, m) for i, m, kind in G.planted if kind == 0]
    assert len(ties) >= 12 and all(want[i][0] == min(r for r, d in m) for i, m in ties)          # equal distance: the smaller index
    assert sum(kind == 1 for i, m, kind in G.planted) >= 12                                       # one apart: the LARGER index wins
    assert all(want[i][0] == max(r for r, d in m) for i, m, kind in G.planted if kind == 1)
    second = {int(q): int(s) for q, s in zip(lst["query"], lst["second"])}
    assert all(second[i] == (512 if len(m) == 1 else sorted(d for r, d in m)[1]) for i, m, kind in G.planted)
    # ---- the long query axis: reverse keys
    G = family("gated", 1)
    out, lst, why = ml.gated_statement(matcher, True, True)
    _, nocross, _ = ml.gated_statement(matcher, True, False)
    gating = sorted(r for i, m, kind in G.planted for r, d in m)
    assert [int(q) for q in nocross["query"]] == gating and (why == 1).sum() == ml.NMAX - len(gating)
    win = {i: min(m, key=lambda rd: (rd[1], rd[0]))[0] for i, m, kind in G.planted}
    assert sorted(int(q) for q in lst["query"]) == sorted(win.values())
    assert all(int(t) == i for i in win for q, t in zip(lst["query"], lst["train"]) if int(q) == win[i])
    for b, (one, zero) in ml.bits_seen(lst["query"]).items():
        assert one and zero, ("reverse winner", b)
    lost = np.nonzero(why == 4)[0]
    assert len(lost) == len(gating) - len(win)
    for b, (one, zero) in ml.bits_seen(lost).items():
        assert one and zero, ("cross-check loser", b)
    assert sum(kind == 0 for i, m, kind in G.planted) >= 12 and sum(kind == 1 for i, m, kind in G.planted) >= 12
    assert all(win[i] == max(r for r, d in m) for i, m, kind in G.planted if kind == 1)          # the nearer query at the larger index
    assert all(win[i] == min(r for r, d in m) for i, m, kind in G.planted if kind in (0, 2))     # equal distances: the smallest index
