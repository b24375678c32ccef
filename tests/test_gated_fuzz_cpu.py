"""CPU suite: the inputs of tests/fuzz_gated.py can fail a wrong kernel.  Runs on the numpy statements alone (no device): the first
300 cases of the committed seed cover every regime, the sentinels decide the statement's answer for their query, removing one
changes that answer, and the strict boundary of the gate is straddled.  The thresholds are conditions on the generator, not
measurements: where one is missed the generator is tuned, not the threshold.

The sensitivity conditions hold in every case that has watched eligible queries, in one of two forms; how many cases fall under the
weaker form or under an exemption is asserted, so that neither can grow unnoticed (the cases and queries all run on the GPU):
  resolved    (j1, d1, d2) = (A, 0, 1) for at least half of the queries
  unresolved  0.001 * radius is below one float32 rounding step (2^-24 relative) of the coordinate sums |x| + |y| the gate works on
              (the train box for the epipolar gate, the projections for the guided one): whether a point at 0.999 or 1.001 radius
              passes is rounding noise, `out` (a d = 0 copy) is gated about half the time and d2 = 1 cannot be had.  These cases keep
              the condition that makes a lost A visible: j1 = A with d1 = 0 for at least half of the queries (A has the smallest
              index of the d = 0 copies)
  coarse      exempt: the float32 step of those coordinates exceeds radius / 8, so not even 0.5 radius is representable and the three
              sentinels fall on the same few float32 values (radii of 0.01 against coordinates in the thousands, projections beyond
              2^20)
  r2 den inf  exempt queries: r2 * den overflows float32 and the band ends where e e overflows, inside u = 0.999 (fuzz_gated `watch`)
  plain       exempt: tiny clouds and H far in their stated grid shape (one cell; every projection in a border cell) cannot hold
              sentinels, which are train points and stretch the grid; a share of those cases runs without sentinels (fuzz_gated
              `plain`)
On the 300 committed cases: 240 have watched queries, of which 146 resolved, 70 unresolved, 24 coarse; 26 plain; 40 112 queries meet
their condition; 22.6 % of the epipolar and 8.8 % of the guided A / B sentinels sit on a cell boundary of the real grid."""
import collections

import numpy as np
import pytest

import epipolar_match_ref as er
import fuzz_gated as fg
import guided_match_ref as gr

SEED = 3                             # the committed seed: tests/test_gpu_gated_fuzz.py and profiles/fuzz_gated.txt use it
NCASES = 300


def _gate(c, m, q=None, t=None):
    f = gr.gate if c["matcher"] == "guided" else er.gate
    with np.errstate(all="ignore"):
        return f(m["q"] if q is None else q, m["t"] if t is None else t, m["M"], m["radius"])


@pytest.fixture(scope="module")
def survey(ah):
    """one pass over the 300 cases: per case the drawn parameters, what make_case reports, and what the statement says about the
    sentinels (computed once, shared by the tests below, never modified)"""
    rows = []
    for i in range(NCASES):
        c = fg.draw_case(SEED, i)
        m = fg.make_case(c, ah.POINT_DTYPE)
        s = m["sent"]
        r = dict(c=c, m=m, good=0, weak_mask=np.zeros(len(s), bool), good_mask=np.zeros(len(s), bool), inA=np.zeros(len(s), bool), inB=np.zeros(len(s), bool),
                 inO=np.zeros(len(s), bool))
        if len(s):
            _, wl, _ = fg.statement(c, m, ratio=(1000, 1), cross=False, max_dist=512)       # exposes j1, d1, d2 of every query with a J_i
            byq = np.full(len(m["q"]), -1)
            byq[wl["query"]] = np.arange(len(wl))
            k = byq[s[:, 0]]
            if len(wl):
                hit = wl[np.maximum(k, 0)]
                r["good_mask"] = (k >= 0) & (hit["train"] == s[:, 1]) & (hit["distance"] == 0) & (hit["second"] == 1)
            g = _gate(c, m, q=m["q"][s[:, 0]])
            rows_ = np.arange(len(s))
            r["inA"], r["inB"], r["inO"] = g[rows_, s[:, 1]], g[rows_, s[:, 2]], g[rows_, s[:, 3]]
            # (j1, d1) by the statement's key rule (the list above hides a query whose d2 is 0 as well: the ratio test rejects it)
            key = np.where(g, (gr.hamming(m["q"][s[:, 0]], m["t"]).astype(np.int64) << 20) | np.arange(len(m["t"]))[None, :], gr.NONE)
            r["weak_mask"] = key.min(axis=1) == s[:, 1]                   # d1 = 0 and j1 = A
        rows.append(r)
    return rows


def test_cases_are_a_pure_function_of_seed_and_index(ah):
    a = [fg.draw_case(SEED, i) for i in range(40)]
    b = [fg.draw_case(SEED, i) for i in reversed(range(40))][::-1]
    assert a == b
    assert fg.draw_case(SEED, 5) != fg.draw_case(SEED + 1, 5) and fg.draw_case(SEED, 5) != fg.draw_case(SEED, 6)
    for i in (0, 9, 25):
        m1, m2 = fg.make_case(a[i], ah.POINT_DTYPE), fg.make_case(b[i], ah.POINT_DTYPE)
        assert m1["q"].tobytes() == m2["q"].tobytes() and m1["t"].tobytes() == m2["t"].tobytes() and m1["M"].tobytes() == m2["M"].tobytes()
    for i in range(40):                                                   # a group's members agree on what the batch call shares
        g = a[i]["group"]
        if g:
            first = fg.draw_case(SEED, g[0])
            assert all(a[i][k] == first[k] for k in ("matcher", "radius", "ratio", "cross", "max_dist", "group"))


def test_every_regime_occurs(survey):
    cnt = collections.Counter()
    for r in survey:
        c, m = r["c"], r["m"]
        cnt[(c["matcher"], "train", c["train"])] += 1
        cnt[(c["matcher"], "regime", c["regime"])] += 1
        if c["regime"] == "affine" and c["matcher"] == "epipolar":
            cnt[("angle", c["angle"])] += 1
        if c["group"]:
            cnt["grouped"] += 1
            cnt["broken"] += c["bad"] is not None
        cnt["n2 = 0"] += len(m["t"]) == 0
        cnt["n1 = 1"] += len(m["q"]) == 1
        cnt[("radius", c["radius"])] += c["radius"] in fg.RADII
        with np.errstate(all="ignore"):
            if c["matcher"] == "epipolar":
                a, b, _, den = er.line(m["q"], m["M"])
                r2den = np.float32(m["radius"]) * np.float32(m["radius"]) * den
                cnt["den below the floor"] += bool(((den < er.DEN_MIN) & (den > 0)).any() and (den >= er.DEN_MIN).any())
                cnt["r2 den = inf"] += bool((np.isinf(r2den) & np.isfinite(den)).any())
                cnt["epipole query"] += bool(m["epipole"])
                cnt["den = 0 at the epipole"] += bool(m["epipole"] and den[0] == 0)
                if c["regime"] == "affine" and c["angle"] == "45":
                    assert (np.abs(a) == np.abs(b))[np.isfinite(a) & np.isfinite(b)].all()
            else:
                wz = gr.project(m["q"], m["M"])[2]
                cnt["wz changes sign"] += bool((wz > 0).any() and (wz < 0).any())
    for matcher in ("guided", "epipolar"):
        for kind in fg.TRAIN_KINDS:
            assert cnt[(matcher, "train", kind)] >= 10, (matcher, kind, cnt[(matcher, "train", kind)])
    for kind in fg.F_KINDS:
        assert cnt[("epipolar", "regime", kind)] >= 10, (kind, cnt)
    for kind in fg.H_KINDS:
        assert cnt[("guided", "regime", kind)] >= 10, (kind, cnt)
    for angle in fg.ANGLES:
        assert cnt[("angle", angle)] >= 1, angle
    for what in ("den below the floor", "r2 den = inf", "epipole query", "wz changes sign"):
        assert cnt[what] >= 5, (what, cnt[what])
    assert cnt["den = 0 at the epipole"] >= 1 and cnt["n2 = 0"] >= 1 and cnt["n1 = 1"] >= 1
    assert cnt["grouped"] >= 40 and cnt["broken"] >= 10
    for rad in fg.RADII:
        assert cnt[("radius", rad)] >= 1, rad


def test_sentinels_decide_the_statement(survey):
    """in every case with watched eligible queries at least half of them have (j1, d1, d2) = (A, 0, 1) -- (j1, d1) = (A, 0) where
    float32 cannot resolve 0.001 radius; in at least 90 % of those cases at least 20 queries, or all of them, do.  The numbers of
    cases under the weaker form and under each exemption are bounded (module docstring)."""
    n = collections.Counter()
    for r in survey:
        c, m = r["c"], r["m"]
        assert len(m["sent"]) == len(m["eligible"]) == len(m["watch"])   # every eligible query has its three points
        if c["plain"]:
            assert len(m["sent"]) == 0
            n["plain"] += m["unwatched"] > 0
            continue
        nel = int(m["watch"].sum())
        if nel == 0:
            continue
        n["with watched queries"] += 1
        if m["coarse"]:
            n["coarse"] += 1
            continue
        mask = r["good_mask"] if m["resolved"] else r["weak_mask"]
        n["resolved" if m["resolved"] else "unresolved"] += 1
        good = int((mask & m["watch"]).sum())
        assert 2 * good >= nel, (c["index"], fg.describe(c, m), m["resolved"], good, nel)
        n["strong"] += good >= 20 or good == nel
        n["served"] += good
    counted = n["resolved"] + n["unresolved"]
    print(dict(n))
    assert n["with watched queries"] >= 220 and n["resolved"] >= 120, n
    assert n["coarse"] <= 30 and n["plain"] <= 30 and n["unresolved"] <= 100, n
    assert n["strong"] >= 0.9 * counted and n["served"] >= 20000, n


def test_sentinels_are_aimed_at_the_real_grid(survey):
    """the sentinels are train points and move the bin kernel's box, so the generator fixes the box first (two fill points on the
    corners of a box that holds every sentinel): the grid the positions were aimed at IS the grid of the finished train set, in
    every case, and the stated share of A / B sentinels sits within 0.001 cell of a cell boundary of it (30 % are aimed, those whose
    boundary is out of reach stay where they were; a random position is that close with probability 0.004)"""
    on, tot, cases = collections.Counter(), collections.Counter(), 0
    for r in survey:
        c, m = r["c"], r["m"]
        s = m["sent"]
        if not len(s):
            continue
        cases += 1
        assert m["grid"] == m["grid_real"], (c["index"], m["grid"], m["grid_real"])
        side, ox, oy = m["grid_real"]
        for col in (1, 2):
            x, y = m["t"]["x"][s[:, col]].astype(np.float64), m["t"]["y"][s[:, col]].astype(np.float64)
            with np.errstate(all="ignore"):
                fx, fy = np.abs(((x - ox) / side + 0.5) % 1 - 0.5), np.abs(((y - oy) / side + 0.5) % 1 - 0.5)
                on[c["matcher"]] += int((np.minimum(fx, fy) < 1e-3).sum())
            tot[c["matcher"]] += len(s)
    print(dict(on), dict(tot), cases)
    assert cases >= 200
    assert on["epipolar"] >= 0.15 * tot["epipolar"] and on["guided"] >= 0.05 * tot["guided"], (on, tot)


def test_grid_shapes_of_tiny_thin_and_far(survey):
    """the regimes that are defined by the grid they produce keep it in a minimum number of cases, sentinels and all: tiny = one
    cell, thin = one row or one column of cells, H far = every finite projection outside the train set's box"""
    n = collections.Counter()
    for r in survey:
        c, m = r["c"], r["m"]
        t = m["t"]
        if not len(t):
            continue
        nx, ny = fg.grid_shape(c["matcher"], m["radius"], t["x"], t["y"])
        if c["train"] == "tiny":
            n[("tiny one cell", c["matcher"])] += (nx, ny) == (1, 1)
        if c["train"] == "thin":
            n["thin one row or column"] += min(nx, ny) == 1
            n["thin one row or column, with sentinels"] += min(nx, ny) == 1 and len(m["sent"]) > 0
        if c["matcher"] == "guided" and c["regime"] == "far":
            with np.errstate(all="ignore"):
                px, py, wz = gr.project(m["q"], m["M"])
                ok = (wz > 0) & np.isfinite(px) & np.isfinite(py)
                inside = (px >= t["x"].min()) & (px <= t["x"].max()) & (py >= t["y"].min()) & (py <= t["y"].max())
            n["far outside the box"] += bool(ok.any() and not (inside & ok).any() and np.isfinite(t["x"]).all() and np.isfinite(t["y"]).all())
    print(dict(n))
    assert n[("tiny one cell", "guided")] >= 5 and n[("tiny one cell", "epipolar")] >= 5, n
    assert n["thin one row or column"] >= 10 and n["thin one row or column, with sentinels"] >= 5, n
    assert n["far outside the box"] >= 5, n


def test_a_lost_sentinel_changes_the_output(survey):
    """the property that turns a skipped candidate into a failing field: with a gated sentinel's x replaced by NaN the statement's
    (j1, d1, d2) of its query changes, and for A so does a match field under the case's own ratio and max_dist (the query alone,
    so the cross-check has nothing to add: rev(A) is this query, the only one with A's descriptor)"""
    rng = np.random.default_rng(11)
    tried = 0
    for r in survey:
        c, m = r["c"], r["m"]
        s = m["sent"]
        cand = np.nonzero(r["good_mask"])[0]
        for k in rng.permutation(cand)[:2]:
            which = 1 + int(rng.integers(2))                              # A or B
            i, j = int(s[k, 0]), int(s[k, which])
            q1 = m["q"][i:i + 1]
            f = gr.match_guided if c["matcher"] == "guided" else er.match_epipolar
            before = f(q1, m["t"], m["M"], m["radius"], (1000, 1), False, 512)[1]
            t2 = m["t"].copy()
            t2["x"][j] = np.nan
            after = f(q1, t2, m["M"], m["radius"], (1000, 1), False, 512)[1]
            assert before.tobytes() != after.tobytes(), (c["index"], i, j)           # (j1, d1, d2) as the list exposes them
            if which == 1:                                                # A: visible under every rule the case may run with
                b2 = f(q1, m["t"], m["M"], m["radius"], c["ratio"], False, c["max_dist"])[0]
                a2 = f(q1, t2, m["M"], m["radius"], c["ratio"], False, c["max_dist"])[0]
                assert any(b2[fld].tobytes() != a2[fld].tobytes() for fld in fg.FIELDS), (c["index"], i, j)
            tried += 1
    assert tried >= 200, tried


def test_the_strict_boundary_is_straddled(survey):
    """u = 0.999 sentinels and out sentinels on each side of the statement's gate"""
    n = collections.Counter()
    for r in survey:
        m = r["m"]
        for u, ing in ((m["uA"], r["inA"]), (m["uB"], r["inB"])):
            k = u == 0.999
            n["0.999 in"] += int(ing[k].sum())
            n["0.999 out"] += int((~ing[k]).sum())
        n["out in"] += int(r["inO"].sum())
        n["out out"] += int((~r["inO"]).sum())
    assert min(n.values()) >= 20, n
    assert n["0.999 in"] > 5 * n["0.999 out"] and n["out out"] > 5 * n["out in"], n       # and mostly on the intended side


def test_lattice_ties_on_the_boundary(survey):
    """integer coordinates, integer-valued model and radius: pairs exactly ON the boundary, which the strict < rejects"""
    ties = collections.Counter()
    for r in survey:
        c, m = r["c"], r["m"]
        if c["train"] != "lattice" or not len(m["t"]):
            continue
        r2 = np.float32(m["radius"]) * np.float32(m["radius"])
        x2, y2 = m["t"]["x"][None, :], m["t"]["y"][None, :]
        with np.errstate(all="ignore"):
            if c["matcher"] == "epipolar":
                a, b, cc, den = er.line(m["q"], m["M"])
                e = (a[:, None] * x2 + b[:, None] * y2) + cc[:, None]
                ties["epipolar"] += int(((e * e) == (r2 * den)[:, None]).sum())
            else:
                px, py, wz = gr.project(m["q"], m["M"])
                dx, dy = x2 - px[:, None], y2 - py[:, None]
                ties["guided"] += int(((((dx * dx) + (dy * dy)) == r2) & (wz > 0)[:, None]).sum())
    assert ties["epipolar"] >= 20 and ties["guided"] >= 20, ties
