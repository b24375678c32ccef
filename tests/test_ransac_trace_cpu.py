"""CPU suite: the statements' side of the RANSAC scratch (tests/ransac_trace.py) held to the statements' own RANSAC loops, on the
committed randomised families of all three estimators -- test_homography_cpu.all_parity_cases ("H"), test_fundamental_cpu.parity_case
("F"), test_pnp_cpu.parity_case ("P").  The best slot triple over a case's score blocks must be the record find_homography /
find_fundamental / solve_pnp returns, at the launch shape the library reports for the call (hak_op_ransac_shape: no device is
touched) and at every other block size; the word layout and the comparison are checked on the statement's own words with one bit
flipped.  The GPU side is tests/test_gpu_ransac_trace.py, which imports the cases and their traces from here."""
import ctypes as C
import functools

import numpy as np
import pytest

import fundamental_ref as fr
import homography_ref as hr
import pnp_ref as pn
import ransac_trace as rt
import test_fundamental_cpu as tf
import test_homography_cpu as th
import test_pnp_cpu as tp
from test_ransac_shapes_cpu import shape_of


@functools.lru_cache(maxsize=None)
def cases(kind):
    """the committed cases of one estimator as dicts of (lst, iterations, threshold, seed, K, ctx, group)"""
    if kind == "H":
        src = th.all_parity_cases()
    elif kind == "F":
        src = [tf.parity_case(k) for k in range(tf.PARITY_CASES)]
    else:
        src = [tp.parity_case(k) for k in range(tp.PARITY_CASES)]
    return [dict(lst=c["corr"] if kind == "P" else c["recs"], iterations=c["iterations"], threshold=c["threshold"], seed=c["seed"],
                 K=c.get("K"), ctx=c["ctx"], group=c["group"]) for c in src]


def groups(kind):
    """group -> the indices of its four cases (one ragged batch call each)"""
    out = {}
    for k, c in enumerate(cases(kind)):
        if c["group"] >= 0:
            out.setdefault(c["group"], []).append(k)
    return out


@functools.lru_cache(maxsize=None)
def case_trace(kind, k, hp, hblocks):
    c = cases(kind)[k]
    return rt.trace(kind, c["lst"], c["iterations"], c["threshold"], c["seed"], hp, hblocks, c["K"])


def statement_triple(kind, c):
    """(inliers, hypothesis, model) of the statement's record; the homography without its refit, which changes no slot"""
    if kind == "H":
        r = hr.find_homography(c["lst"], c["iterations"], c["threshold"], c["seed"], False)[0]
        return (int(r["inliers"]), int(r["hypothesis"]), 0), r["H"]
    if kind == "F":
        r = fr.find_fundamental(c["lst"], c["iterations"], c["threshold"], c["seed"])[0]
        return (int(r["inliers"]), int(r["hypothesis"]), int(r["root"])), r["F"]
    r = pn.solve_pnp(c["lst"], c["K"], c["iterations"], c["threshold"], c["seed"])[0]
    return (int(r["inliers"]), int(r["hypothesis"]), int(r["solution"])), np.concatenate([r["R"], r["t"]])


@pytest.mark.parametrize("kind", rt.KINDS)
def test_best_slot_is_the_statements_record(ah, kind):
    """every committed case at the single call's shape, the grouped ones also at their batch's; a tenth of the cases at every other
    block size too (the largest key must not depend on hp)"""
    shapes = set()
    with_model = partial_last = 0
    for k, c in enumerate(cases(kind)):
        want, model = statement_triple(kind, c)
        todo = [shape_of(ah, 1, c["iterations"])]
        if c["group"] >= 0:
            todo.append(shape_of(ah, 4, c["iterations"]))
        if k % 10 == 0:
            todo += [(hp, (c["iterations"] + hp - 1) // hp) for hp in (16, 32, 64, 128, 256)]
        for hp, hblocks in dict.fromkeys(todo):
            tr = case_trace(kind, k, hp, hblocks)
            assert rt.best_slot(tr["slots"]) == want, (kind, k, hp, hblocks, rt.best_slot(tr["slots"]), want)
            assert tr["slots"].shape == (hblocks, 3) and tr["slots"].dtype == np.int32
            have = tr["slots"][:, 1] >= 0
            assert (tr["slots"][~have] == (0, -1, 0)).all()
            assert (tr["slots"][have, 1] // hp == np.nonzero(have)[0]).all()          # a block names one of its own hypotheses
            assert tr["valid"][tr["slots"][have, 1], tr["slots"][have, 2]].all()
            shapes.add((hp, hblocks))
            partial_last += bool(c["iterations"] % hp)
        if want[1] >= 0:
            with_model += 1
            assert tr["models"][want[1], want[2]].tobytes() == model.tobytes()
            assert not tr["models"][~tr["valid"]].any() or kind == "H"   # the statements write zeros where there is no model
    assert with_model >= 50 and partial_last >= 50 and len({s[0] for s in shapes}) == 5 and max(s[1] for s in shapes) >= 17, shapes


def test_words_and_differences():
    """the [word][iterations] layout of ransac_common.h on the statement's own models: no difference; one flipped bit in a valid
    model, a `valid` word and a slot are each reported; for "F" a flipped bit in a model without a bit is not"""
    for kind in ("F", "P"):
        k = next(k for k, c in enumerate(cases(kind)) if c["iterations"] == 64 and
                 0 < case_trace(kind, k, 16, 4)["valid"].sum() < case_trace(kind, k, 16, 4)["valid"].size)
        tr = case_trace(kind, k, 16, 4)
        nm, nw = rt.NM[kind], rt.NW[kind]
        assert rt.WORDS[kind] == nm * nw + 1
        words = np.concatenate([tr["models"].view(np.uint32).reshape(64, nm * nw).T, rt.valid_words(tr["valid"])[None]])
        assert words.shape == (rt.WORDS[kind], 64) and not rt.differences(tr, words, tr["slots"])
        assert not rt.differences(tr, words.reshape(-1), tr["slots"].reshape(-1))
        h, r = (int(v[0]) for v in np.nonzero(tr["valid"]))
        bad = words.copy()
        bad[nw * r + 3, h] ^= 1
        assert "model" in rt.differences(tr, bad, tr["slots"])[0]
        h0, r0 = (int(v[0]) for v in np.nonzero(~tr["valid"]))
        bad = words.copy()
        bad[nw * r0 + 3, h0] ^= 1
        assert bool(rt.differences(tr, bad, tr["slots"])) == (kind == "P")
        bad = words.copy()
        bad[nm * nw, h] ^= 1 << r
        assert "valid" in rt.differences(tr, bad, tr["slots"])[0]
        slots = tr["slots"].copy()
        slots[2, 0] += 1
        assert "block 2" in rt.differences(tr, words, slots)[0]
        assert rt.differences(tr, words, slots[:3])
    tr = case_trace("H", next(k for k, c in enumerate(cases("H")) if c["iterations"] == 64), 16, 4)
    assert not rt.differences(tr, None, tr["slots"])


def test_block_slots_by_hand():
    valid = np.array([[1, 1], [0, 1], [0, 0], [1, 0], [1, 1], [0, 0]], bool)
    cnt = np.array([[3, 5], [0, 5], [9, 9], [5, 0], [2, 2], [7, 7]])
    assert rt.block_slots(valid, cnt, 2, 3).tolist() == [[5, 0, 1], [5, 3, 0], [2, 4, 0]]
    assert rt.block_slots(valid, cnt, 4, 2).tolist() == [[5, 0, 1], [2, 4, 0]]
    assert rt.block_slots(valid[2:3], cnt[2:3], 16, 1).tolist() == [[0, -1, 0]]
    assert rt.best_slot(rt.block_slots(valid, cnt, 2, 3)) == (5, 0, 1) and rt.best_slot(np.array([[0, -1, 0]])) == (0, -1, 0)
    assert rt.best_slot(np.array([[0, -1, 0], [0, 17, 2], [0, 33, 0]])) == (0, 17, 2)      # a model without inliers is a model
    assert rt.valid_words(valid).tolist() == [3, 2, 0, 1, 3, 0]


def test_accessor_refuses_without_a_device(ah):
    slots = np.full(3, -7, np.int32)
    words = np.full(49, 0xEE, np.uint32)
    fn = ah.lib.hak_debug_ransac_scratch
    assert fn(None, 1, 49, 1, 1, words.ctypes.data, slots.ctypes.data) != 0
    assert "context" in ah.lib.hak_last_error().decode()
    assert (slots == -7).all() and (words == 0xEE).all()
