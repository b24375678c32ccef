"""GPU suite: the three RANSAC estimators (homography, fundamental matrix, P3P absolute pose) at every launch shape of
tests/ransac_shapes.py -- all five block sizes hp = 16 .. 256, last blocks of 1 and 8 hypotheses, more than 64 score blocks per
pair (the finish kernels' second trip over the slots), the iteration limit, ragged batches with lists across the LDS chunk edge --
bit for bit against the numpy statements: every H / F / R, t bit, inliers, hypothesis, refined / root / solution, n and every mask
byte; mask bytes past a pair's count and records past npairs keep their 0xEE fill.
What the cases reach (winners in the last partial block, in blocks >= 64, ties between blocks, a better hypothesis just past
`iterations`; for P3P, whose hypotheses have four models and whose score kernel stages {X, Y, Z, u} + {v}: winners at each of the
solutions 0 .. 3, two models of one hypothesis that tie, lists past the LDS chunk at every hp, more than 16 model blocks up to the
1024 of the iteration limit) is asserted on the statements alone in tests/test_ransac_shapes_cpu.py.  No case is exempt and
nothing is tolerated."""
import numpy as np
import pytest

import fundamental_ref as fr
import fundamental_refit_ref as rr
import homography_ref as hr
import pnp_ref as pn
import ransac_shapes as rs
from test_gpu_fundamental import as_pairs, assert_same as assert_same_f, det, gpu_single as gpu_single_f, torch, upload  # noqa: F401
from test_gpu_homography import assert_same as assert_same_h, gpu_single as gpu_single_h
from test_gpu_pnp import assert_same as assert_same_p, gpu_pnp
from test_pnp_cpu import corr_array

pytestmark = pytest.mark.gpu

ENTRIES = list(range(len(rs.SHAPES)))
FILL = 0xEE


def record_dtype(ah, kind):
    return {"H": ah.HOMOGRAPHY_DTYPE, "F": ah.FUNDAMENTAL_DTYPE, "P": ah.ABS_POSE_DTYPE}[kind]


def as_corr(lst):
    """(n, 5) float32 {X, Y, Z, u, v} as correspondences"""
    return corr_array(lst[:, :3], lst[:, 3:])


def enqueue(ah, torch, ctx, kind, c, refine=1):
    """one batch call of case c on the context's stream, not synchronised: -> the tensors that must outlive it (lists, counts,
    records with one sentinel record behind them, masks)"""
    np_, stride = c["npairs"], c["stride"]
    if kind == "P":
        allp = np.zeros(np_ * stride, ah.CORR3D_DTYPE)
        allp["X"] = np.nan                                              # records past a pair's count are not the call's business
    else:
        allp = np.zeros(np_ * stride, ah.MATCH_PAIR_DTYPE)
        for f in ("x1", "y1", "x2", "y2"):
            allp[f] = np.nan
    for k, lst in enumerate(c["lists"]):
        allp[k * stride:k * stride + len(lst)] = as_corr(lst) if kind == "P" else as_pairs(ah, lst)
    d = upload(torch, allp)
    d_cnt = torch.tensor(c["counts"], dtype=torch.int32, device="cuda")
    size = record_dtype(ah, kind).itemsize
    d_out = torch.full(((np_ + 1) * size,), FILL, dtype=torch.uint8, device="cuda")
    d_mask = torch.full((np_ * stride,), FILL, dtype=torch.uint8, device="cuda")
    if kind == "H":
        ah.check(ah.lib.hak_find_homography_batch(ctx, d.data_ptr(), stride, d_cnt.data_ptr(), np_, c["iterations"], c["threshold"],
                                                  c["seed"], refine, d_out.data_ptr(), d_mask.data_ptr()))
    elif kind == "F":
        ah.check(ah.lib.hak_find_fundamental_batch(ctx, d.data_ptr(), stride, d_cnt.data_ptr(), np_, c["iterations"], c["threshold"],
                                                   c["seed"], d_out.data_ptr(), d_mask.data_ptr()))
    else:
        K = ah.intrinsics(rs.K_TABLE)
        ah.check(ah.lib.hak_solve_pnp_batch(ctx, d.data_ptr(), stride, d_cnt.data_ptr(), np_, K.ctypes.data, c["iterations"],
                                            c["threshold"], c["seed"], d_out.data_ptr(), d_mask.data_ptr()))
    return d, d_cnt, d_out, d_mask


def compare(ah, kind, c, want, d_out, d_mask, what):
    """the downloaded records and masks of a finished batch call against the statement's"""
    np_, stride = c["npairs"], c["stride"]
    dtype = record_dtype(ah, kind)
    raw = d_out.cpu().numpy()
    assert (raw[np_ * dtype.itemsize:] == FILL).all(), (what, "a record past npairs was written")
    out = raw[:np_ * dtype.itemsize].view(dtype)
    masks = d_mask.cpu().numpy().reshape(np_, stride)
    same = {"H": assert_same_h, "F": assert_same_f, "P": assert_same_p}[kind]
    for k, (w, wm) in enumerate(want):
        n = len(c["lists"][k])
        same(out[k], masks[k, :n], w, wm, (what, k))
        assert (masks[k, n:] == FILL).all(), (what, k, "written past the count")


def run(ah, torch, det, kind, c, want, refine=1):
    """the call of one table entry: the batch call, or for one pair the single call without and with a context"""
    if c["npairs"] > 1:
        keep = enqueue(ah, torch, det.ctx, kind, c, refine)
        ah.check(ah.lib.hak_sync(det.ctx))
        compare(ah, kind, c, want, keep[2], keep[3], (kind, c["npairs"], c["iterations"], refine))
        return keep
    if kind == "P":
        corr = as_corr(c["lists"][0])
        for ctx in (None, det.ctx):
            got, gm = gpu_pnp(ah, torch, corr, rs.K_TABLE, c["iterations"], c["threshold"], c["seed"], ctx=ctx)
            assert len(gm) == len(corr)
            assert_same_p(got, gm, want[0][0], want[0][1], (kind, c["iterations"], ctx is not None))
        return None
    pairs = as_pairs(ah, c["lists"][0])
    for ctx in (None, det.ctx):
        if kind == "H":
            got, gm = gpu_single_h(ah, torch, pairs, c["iterations"], c["threshold"], c["seed"], refine, ctx=ctx)
            assert_same_h(got, gm, want[0][0], want[0][1], (kind, c["iterations"], refine, ctx is not None))
        else:
            got, gm = gpu_single_f(ah, torch, pairs, c["iterations"], c["threshold"], c["seed"], ctx=ctx)
            assert_same_f(got, gm, want[0][0], want[0][1], (kind, c["iterations"], ctx is not None))


@pytest.mark.parametrize("e", ENTRIES, ids=rs.shape_id)
def test_homography_shape(ah, torch, det, e):
    c = rs.shape_case("H", e)
    for refine in (0, 1):
        run(ah, torch, det, "H", c, rs.statement("H", e, refine), refine)


@pytest.mark.parametrize("e", ENTRIES, ids=rs.shape_id)
def test_fundamental_shape(ah, torch, det, e):
    run(ah, torch, det, "F", rs.shape_case("F", e), rs.statement("F", e))


@pytest.mark.parametrize("e", ENTRIES, ids=rs.shape_id)
def test_pnp_shape(ah, torch, det, e):
    run(ah, torch, det, "P", rs.shape_case("P", e), rs.statement("P", e))


def test_refit_follows_the_64_pair_batch(ah, torch, det):
    """hak_refine_fundamental_batch in place on the device records of the 64 x 257 batch (hp = 256): equal to the statement's refit
    chained from the statement's RANSAC records"""
    e = [s[:2] for s in rs.SHAPES].index((64, 257))
    c, want = rs.shape_case("F", e), rs.statement("F", e)
    d, d_cnt, d_out, d_mask = run(ah, torch, det, "F", c, want)
    d_mask.fill_(FILL)
    ah.check(ah.lib.hak_refine_fundamental_batch(det.ctx, d.data_ptr(), c["stride"], d_cnt.data_ptr(), c["npairs"], c["threshold"], 3,
                                                 d_out.data_ptr(), d_mask.data_ptr()))
    ah.check(ah.lib.hak_sync(det.ctx))
    refit = [rr.refine_fundamental(lst, w, c["threshold"], 3) for lst, (w, _) in zip(c["lists"], want)]
    assert sum(int(r["root"]) == rr.REFINED_ROOT for r, _ in refit) >= 10
    compare(ah, "F", c, refit, d_out, d_mask, "refit")


def test_calls_in_flight_share_growing_scratch(ah, torch):
    """2 x 64, 64 x 257, 1 x 65536 and 2 x 64 again, homography, fundamental and P3P interleaved on one fresh context with one
    hak_sync at the end: the grow-only slot and model scratch, which the estimators share (28 words per hypothesis for the
    fundamental matrix, 49 for P3P, so the two outgrow it in turn), is reallocated between calls that are still in flight; every
    result equals its statement"""
    ea, eb = ([s[:2] for s in rs.SHAPES].index(s) for s in ((64, 257), (1, 65536)))
    small = {}
    for kind in rs.KINDS:
        rng = np.random.default_rng([rs.SEED, 99, rs.KINDS.index(kind)])
        lists = [rs.make_list(kind, n, n // 2, 7, (), rng) for n in (150, 90)]
        small[kind] = dict(npairs=2, iterations=64, seed=7, threshold=2.0, stride=150, counts=[150, 90], lists=lists)
    want_small = {"H": [hr.find_homography(lst, 64, 2.0, 7, True) for lst in small["H"]["lists"]],
                  "F": [fr.find_fundamental(lst, 64, 2.0, 7) for lst in small["F"]["lists"]],
                  "P": [pn.solve_pnp(lst, rs.K_TABLE, 64, 2.0, 7) for lst in small["P"]["lists"]]}
    dt = ah.Akazer()
    dt.init((256, 192, 256), max_pts=500, batch=2)                      # a context that has run no estimator yet
    calls = []
    for c_of, w_of in ((small.get, want_small.get), (lambda k: rs.shape_case(k, ea), lambda k: rs.statement(k, ea)),
                       (lambda k: rs.shape_case(k, eb), lambda k: rs.statement(k, eb)), (small.get, want_small.get)):
        for kind in rs.KINDS:
            calls.append((kind, c_of(kind), w_of(kind), enqueue(ah, torch, dt.ctx, kind, c_of(kind))))
    ah.check(ah.lib.hak_sync(dt.ctx))
    for k, (kind, c, want, keep) in enumerate(calls):
        compare(ah, kind, c, want, keep[2], keep[3], ("call", k, kind))
    dt.close()
