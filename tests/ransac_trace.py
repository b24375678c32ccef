"""The numpy statements' side of the RANSAC scratch (hak_debug_ransac_scratch, include/hipakaze_test.h): every model of every
hypothesis and the best (inliers, hypothesis, model) of every score block, for one list of a homography ("H"), fundamental-matrix
("F") or P3P ("P") call.  A call returns only the winner; a solver that is wrong on a degenerate or ill-conditioned sample stays
unseen as long as a well-conditioned one wins.  Here every hypothesis is held to the statement.

The checker only -- the product never calls it.  Plain numpy, imports without a device.  The models are fundamental_ref.models and
pnp_ref.models (homography_ref.hypotheses for "H", which keeps no models scratch); a block's triple is made from the statement's
models scored with the statement's inlier_mask: the largest count among the block's valid models, then the smallest hypothesis,
then the smallest model index; (0, -1, 0) for a block without a valid model.  The blocks are those of the launch shape
(hp hypotheses per block, hblocks blocks) that hak_op_ransac_shape reports for the call: the helper takes them as arguments and
restates no launch rule.

What `differences` compares, as bytes:
  * the `valid` word of every hypothesis;
  * every word of every model whose bit is set;
  * "P": all 48 model words of every hypothesis -- the rule fixes zeros for a missing or rejected solution;
  * "F": the words of a model WITHOUT a bit are left out.  include/hipakaze.h defines the record and the mask of a call, not the
    scratch words of a root that gave no model, so they are nobody's contract;
  * every slot triple.
"""
import numpy as np

import fundamental_ref as fr
import homography_ref as hr
import pnp_ref as pn
from pose_ref import intrinsics

KINDS = ("H", "F", "P")
NM = {"H": 1, "F": 3, "P": 4}                                           # models per hypothesis
NW = {"H": 9, "F": 9, "P": 12}                                          # float32 words per model
WORDS = {"H": 0, "F": 28, "P": 49}                                      # scratch words per hypothesis: NM NW + 1, none for "H"
_ROWS = 1 << 22                                                         # model x record products scored at a time


def records(kind, lst):
    return pn.records(lst) if kind == "P" else hr.records(lst)


def statement_models(kind, rec, iterations, seed, K=None):
    """(M (iterations, NM, NW) float32, valid (iterations, NM) bool) of hypotheses 0 .. iterations - 1"""
    hs = np.arange(iterations)
    if kind == "H":
        H, ok = hr.hypotheses(rec, seed, hs)
        return H[:, None], ok[:, None]
    if kind == "F":
        return fr.models(rec, seed, hs)
    return pn.models(rec, intrinsics(K), seed, hs)


def model_counts(kind, M, valid, rec, threshold, K=None):
    """(iterations, NM) int64: the statement's inlier count of every valid model, 0 where there is none"""
    t2 = np.float32(threshold) * np.float32(threshold)
    cnt = np.zeros(valid.shape, np.int64)
    hh, rr = np.nonzero(valid)
    if len(hh) == 0 or len(rec) == 0:
        return cnt
    step = max(1, _ROWS // len(rec))
    for a in range(0, len(hh), step):
        m = M[hh[a:a + step], rr[a:a + step]]
        if kind == "H":
            c = hr.inlier_mask(m, rec, t2)
        elif kind == "F":
            c = fr.inlier_mask(m, rec, t2)
        else:
            c = pn.inlier_mask(m, rec, intrinsics(K), t2)
        cnt[hh[a:a + step], rr[a:a + step]] = c.sum(axis=1)
    return cnt


def block_slots(valid, cnt, hp, hblocks):
    """(hblocks, 3) int32 {inliers, hypothesis, model}: per block of hp hypotheses the largest count among its valid models, then
    the smallest hypothesis, then the smallest model; (0, -1, 0) without one"""
    out = np.zeros((hblocks, 3), np.int32)
    out[:, 1] = -1
    for b in range(hblocks):
        v, c = valid[b * hp:(b + 1) * hp], cnt[b * hp:(b + 1) * hp]
        hh, rr = np.nonzero(v)                                          # ascending (h, r)
        if len(hh):
            j = int(np.argmax(c[hh, rr]))                               # the first maximum
            out[b] = (c[hh[j], rr[j]], b * hp + hh[j], rr[j])
    return out


def best_slot(slots):
    """the triple a finish kernel takes from a list's slots: the largest count, then the smallest hypothesis (blocks ascend in h)"""
    have = slots[slots[:, 1] >= 0]
    if len(have) == 0:
        return (0, -1, 0)
    return tuple(int(v) for v in have[int(np.argmax(have[:, 0]))])


def trace(kind, lst, iterations, threshold, seed, hp, hblocks, K=None):
    """the statement's scratch of one list: dict(kind, models (iterations, NM, NW) float32, valid (iterations, NM) bool,
    counts (iterations, NM) int64, slots (hblocks, 3) int32)"""
    assert kind in KINDS and hblocks * hp >= iterations > (hblocks - 1) * hp, (kind, iterations, hp, hblocks)
    rec = records(kind, lst)
    M, valid = statement_models(kind, rec, iterations, seed, K)
    cnt = model_counts(kind, M, valid, rec, threshold, K)
    return dict(kind=kind, models=M, valid=valid, counts=cnt, slots=block_slots(valid, cnt, hp, hblocks))


def valid_words(valid):
    """(iterations,) uint32: bit r = model r exists"""
    return (valid.astype(np.uint32) << np.arange(valid.shape[1], dtype=np.uint32)).sum(axis=1).astype(np.uint32)


def differences(tr, got_words, got_slots, limit=5):
    """the statement's trace against what the accessor returned for the same list: got_words (WORDS[kind], iterations) uint32 (None
    for "H"), got_slots (hblocks, 3) int32.  Returns a list of at most `limit` descriptions, empty when every compared byte agrees"""
    kind, out = tr["kind"], []
    if WORDS[kind]:
        nm, nw = NM[kind], NW[kind]
        it = tr["valid"].shape[0]
        got = np.asarray(got_words, np.uint32).reshape(WORDS[kind], it)
        gv, wv = got[nm * nw], valid_words(tr["valid"])
        for h in np.nonzero(gv != wv)[0][:limit]:
            out.append(f"hypothesis {h}: valid {int(gv[h]):#x}, statement {int(wv[h]):#x}")
        gm = got[:nm * nw].T.reshape(it, nm, nw)
        wm = tr["models"].view(np.uint32)
        bad = (gm != wm).any(axis=2)
        if kind == "F":
            bad &= tr["valid"]
        for h, r in zip(*np.nonzero(bad)):
            if len(out) >= limit:
                break
            out.append(f"hypothesis {h} model {r} (valid {bool(tr['valid'][h, r])}): {gm[h, r].view(np.float32)}, statement "
                       f"{tr['models'][h, r]}")
    gs = np.asarray(got_slots, np.int32).reshape(-1, 3)
    if gs.shape != tr["slots"].shape:
        out.append(f"{len(gs)} slots, statement {len(tr['slots'])}")
    else:
        for b in np.nonzero((gs != tr["slots"]).any(axis=1))[0][:limit]:
            out.append(f"block {b}: slot {gs[b].tolist()}, statement {tr['slots'][b].tolist()}")
    return out[:limit]
