"""GPU suite: every hypothesis and every score block of the three RANSAC estimators against the numpy statements, not only the
winner a call returns.  After each hak_find_homography / hak_find_fundamental / hak_solve_pnp call on a context the context's RANSAC
scratch is read through hak_debug_ransac_scratch (include/hipakaze_test.h) and compared as tests/ransac_trace.py says: the `valid`
word of every hypothesis, every word of every model with a bit (P3P: all 48 model words, zeros included), and the (inliers,
hypothesis, model) of every score block -- on the committed randomised families (150 P3P cases, 150 fundamental-matrix cases, 152
homography cases, the last slots only: the homography keeps no models), and on their ragged batch groups with npairs = 4.  What the
cases reach is asserted on the statements alone in test_pnp_cpu.py, test_fundamental_cpu.py, test_homography_cpu.py; that the
helper's best slot is the statements' record in test_ransac_trace_cpu.py."""
import numpy as np
import pytest

import ransac_trace as rt
from test_gpu_fundamental import as_pairs, det, synth, torch, upload  # noqa: F401 (fixtures)
from test_ransac_shapes_cpu import shape_of
from test_ransac_trace_cpu import case_trace, cases, groups

pytestmark = pytest.mark.gpu

RECORD = {"H": "HOMOGRAPHY_DTYPE", "F": "FUNDAMENTAL_DTYPE", "P": "ABS_POSE_DTYPE"}


def read_scratch(ah, ctx, kind, npairs, iterations, hblocks):
    """-> (words (npairs, WORDS, iterations) uint32 or None, slots (npairs, hblocks, 3) int32) of the last call on ctx"""
    nw = rt.WORDS[kind]
    words = np.full(max(1, npairs * nw * iterations), 0xEEEEEEEE, np.uint32)
    slots = np.full(npairs * hblocks * 3, -7, np.int32)
    ah.check(ah.lib.hak_debug_ransac_scratch(ctx, npairs, nw, iterations, hblocks, words.ctypes.data if nw else None, slots.ctypes.data))
    return (words.reshape(npairs, nw, iterations) if nw else None), slots.reshape(npairs, hblocks, 3)


def device_list(ah, kind, lst):
    return lst if kind == "P" else as_pairs(ah, lst)


def call(ah, torch, ctx, kind, d_list, stride, counts, c):
    """one call of `kind` on ctx: single (counts = n, an int) or batch (counts: a device tensor); the record and the mask go to
    buffers of their own and are compared elsewhere (test_gpu_homography / _fundamental / _pnp)"""
    lib, it, thr, seed = ah.lib, c["iterations"], c["threshold"], c["seed"]
    batch = not isinstance(counts, int)
    npairs = len(counts) if batch else 1
    size = getattr(ah, RECORD[kind]).itemsize
    rec = np.zeros(size, np.uint8)
    d_out = torch.zeros(npairs * size, dtype=torch.uint8, device="cuda")
    out = d_out.data_ptr() if batch else rec.ctypes.data
    K = ah.intrinsics(c["K"]) if kind == "P" else None
    if kind == "H":
        args = (it, thr, seed, 1, out, None) if batch else (it, thr, seed, 1, None, out)
        fn = lib.hak_find_homography_batch if batch else lib.hak_find_homography
    elif kind == "F":
        args = (it, thr, seed, out, None) if batch else (it, thr, seed, None, out)
        fn = lib.hak_find_fundamental_batch if batch else lib.hak_find_fundamental
    else:
        args = (K.ctypes.data, it, thr, seed, out, None) if batch else (K.ctypes.data, it, thr, seed, None, out)
        fn = lib.hak_solve_pnp_batch if batch else lib.hak_solve_pnp
    head = (ctx, d_list.data_ptr(), stride, counts.data_ptr(), npairs) if batch else (ctx, d_list.data_ptr(), counts)
    ah.check(fn(*head, *args))


@pytest.mark.parametrize("kind", rt.KINDS)
def test_every_hypothesis_and_slot_of_the_parity_cases(ah, torch, det, kind):
    """single calls.  Measured on an MI355X box: see profiles/ransac_trace.txt (the numpy statement is the larger share)"""
    fails = []
    compared = models = 0
    for k, c in enumerate(cases(kind)):
        hp, hblocks = shape_of(ah, 1, c["iterations"])
        tr = case_trace(kind, k, hp, hblocks)
        lst = device_list(ah, kind, c["lst"])
        call(ah, torch, det.ctx, kind, upload(torch, lst), 0, len(lst), c)
        words, slots = read_scratch(ah, det.ctx, kind, 1, c["iterations"], hblocks)
        fails += [f"{kind} case {k}: {d}" for d in rt.differences(tr, None if words is None else words[0], slots[0], 2)]
        compared += c["iterations"]
        models += int(tr["valid"].sum())
    assert compared >= 10000 and models >= 2000, (compared, models)
    assert not fails, f"{len(fails)} differ: " + "; ".join(fails[:4])


@pytest.mark.parametrize("kind", rt.KINDS)
def test_every_hypothesis_and_slot_of_the_ragged_groups(ah, torch, det, kind):
    """the groups of four cases as one batch call each: [pair][word][iterations] models, [pair][block] slots at the batch's shape"""
    fails = []
    gs = groups(kind)
    assert len(gs) >= 5
    for g, ks in sorted(gs.items()):
        cs = [cases(kind)[k] for k in ks]
        c0 = cs[0]
        hp, hblocks = shape_of(ah, len(ks), c0["iterations"])
        lists = [device_list(ah, kind, c["lst"]) for c in cs]
        stride = max(1, max(len(lst) for lst in lists))
        allp = np.zeros(len(ks) * stride, lists[0].dtype)
        for f in (("X",) if kind == "P" else ("x1", "y1", "x2", "y2")):
            allp[f] = np.nan                                            # records past a pair's count are not the call's business
        for slot, lst in enumerate(lists):
            allp[slot * stride:slot * stride + len(lst)] = lst
        d_cnt = torch.tensor([len(lst) for lst in lists], dtype=torch.int32, device="cuda")
        call(ah, torch, det.ctx, kind, upload(torch, allp), stride, d_cnt, c0)
        words, slots = read_scratch(ah, det.ctx, kind, len(ks), c0["iterations"], hblocks)
        for slot, k in enumerate(ks):
            tr = case_trace(kind, k, hp, hblocks)
            fails += [f"{kind} group {g} case {k}: {d}"
                      for d in rt.differences(tr, None if words is None else words[slot], slots[slot], 2)]
    assert not fails, f"{len(fails)} differ: " + "; ".join(fails[:4])


def test_accessor_refusals(ah, torch, det):
    c = dict(iterations=64, threshold=1.0, seed=1, K=(1500.0, 1500.0, 960.0, 540.0))
    call(ah, torch, det.ctx, "P", upload(torch, np.zeros(8, ah.CORR3D_DTYPE)), 0, 8, c)
    slots, words = np.full(12, -7, np.int32), np.full(49 * 64, 0xEE, np.uint32)
    fn = ah.lib.hak_debug_ransac_scratch
    bad = [(None, 1, 49, 64, 4, words.ctypes.data, slots.ctypes.data), (det.ctx, 1, 49, 64, 4, None, slots.ctypes.data),
           (det.ctx, 1, 49, 64, 4, words.ctypes.data, None), (det.ctx, 0, 49, 64, 4, words.ctypes.data, slots.ctypes.data),
           (det.ctx, 1, -1, 64, 4, words.ctypes.data, slots.ctypes.data), (det.ctx, 1, 49, 0, 4, words.ctypes.data, slots.ctypes.data),
           (det.ctx, 1, 49, 64, 0, words.ctypes.data, slots.ctypes.data),
           (det.ctx, 1 << 20, 49, 65536, 4, words.ctypes.data, slots.ctypes.data),                 # beyond the models' capacity
           (det.ctx, 1, 49, 64, 1 << 28, words.ctypes.data, slots.ctypes.data)]                    # beyond the slots'
    for args in bad:
        assert fn(*args) != 0, args
        assert ah.lib.hak_last_error().decode() != ""
    assert (slots == -7).all() and (words == 0xEE).all()
    ah.check(fn(det.ctx, 1, 49, 64, 4, words.ctypes.data, slots.ctypes.data))
    assert (slots.reshape(4, 3) == (0, -1, 0)).all() and not words.any()     # eight all-zero correspondences: no model anywhere
    ah.check(fn(det.ctx, 1, 0, 64, 4, None, slots.ctypes.data))         # no words asked for: the slots alone
