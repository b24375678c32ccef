"""The numpy statement's side of the RANSAC scratch of hak_find_essential (hak_debug_ransac_scratch, include/hipakaze_test.h), as
tests/ransac_trace.py is for the other estimators: every model of every hypothesis and the best (inliers, hypothesis, model) of
every score block of one list.

The checker only -- the product never calls it.  hak_find_essential keeps hypothesis h as the three VIRTUAL hypotheses 3 h + g,
g = 0..2, of four models each: root r is model r mod 4 of virtual hypothesis 3 h + r / 4, slots 10 and 11 never hold a model, 37
words per virtual hypothesis.  The accessor and hak_op_ransac_shape are asked with 3 x the call's iterations; a slot's triple is in
virtual terms.  What `differences` compares, as bytes: the `valid` word of every virtual hypothesis, every word of every model whose
bit is set (the words of a root that gave no model are nobody's contract, as for the fundamental matrix), every slot triple.
"""
import numpy as np

import essential_ref as er
import fundamental_ref as fr
import homography_ref as hr
import ransac_trace as rt

NM, NW, WORDS = 4, 9, 37


def virtual(M, valid):
    """(iterations, 10, 9), (iterations, 10) -> (3 iterations, 4, 9), (3 iterations, 4)"""
    it = M.shape[0]
    Mv = np.zeros((it, 12, 9), np.float32)
    vv = np.zeros((it, 12), bool)
    Mv[:, :10], vv[:, :10] = M, valid
    return Mv.reshape(3 * it, 4, 9), vv.reshape(3 * it, 4)


def trace(lst, K1, K2, iterations, threshold, seed, hp, hblocks):
    """the statement's scratch of one list at the launch shape (hp, hblocks) of hak_op_ransac_shape(npairs, 3 * iterations):
    dict(models (3 it, 4, 9) float32, valid (3 it, 4) bool, counts (3 it, 4) int64, slots (hblocks, 3) int32)"""
    assert hblocks * hp >= 3 * iterations > (hblocks - 1) * hp, (iterations, hp, hblocks)
    rec = hr.records(lst)
    M, valid = virtual(*er.models(rec, K1, K2, seed, np.arange(iterations)))
    t2 = np.float32(threshold) * np.float32(threshold)
    cnt = np.zeros(valid.shape, np.int64)
    hh, rr = np.nonzero(valid)
    if len(hh) and len(rec):
        cnt[hh, rr] = fr.inlier_mask(M[hh, rr], rec, t2).sum(axis=1)
    return dict(models=M, valid=valid, counts=cnt, slots=rt.block_slots(valid, cnt, hp, hblocks))


def record_of(tr, n):
    """the record the finish kernel makes of the trace's slots: (inliers, hypothesis, root) in the call's terms"""
    inl, vh, r = rt.best_slot(tr["slots"])
    return (0, -1, 0) if vh < 0 else (inl, vh // 3, er.ROOT_BASE + 4 * (vh % 3) + r)


def differences(tr, got_words, got_slots, limit=5):
    """the statement's trace against what the accessor returned for the same list: got_words (37, 3 iterations) uint32, got_slots
    (hblocks, 3) int32.  Returns at most `limit` descriptions, empty when every compared byte agrees"""
    out = []
    vit = tr["valid"].shape[0]
    got = np.asarray(got_words, np.uint32).reshape(WORDS, vit)
    gv, wv = got[NM * NW], rt.valid_words(tr["valid"])
    for h in np.nonzero(gv != wv)[0][:limit]:
        out.append(f"virtual hypothesis {h}: valid {int(gv[h]):#x}, statement {int(wv[h]):#x}")
    gm = got[:NM * NW].T.reshape(vit, NM, NW)
    bad = (gm != tr["models"].view(np.uint32)).any(axis=2) & tr["valid"]
    for h, r in zip(*np.nonzero(bad)):
        if len(out) >= limit:
            break
        out.append(f"virtual hypothesis {h} model {r}: {gm[h, r].view(np.float32)}, statement {tr['models'][h, r]}")
    gs = np.asarray(got_slots, np.int32).reshape(-1, 3)
    if gs.shape != tr["slots"].shape:
        out.append(f"{len(gs)} slots, statement {len(tr['slots'])}")
    else:
        for b in np.nonzero((gs != tr["slots"]).any(axis=1))[0][:limit]:
            out.append(f"block {b}: slot {gs[b].tolist()}, statement {tr['slots'][b].tolist()}")
    return out[:limit]
