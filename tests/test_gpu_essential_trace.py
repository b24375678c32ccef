"""GPU suite: every hypothesis and every score block of hak_find_essential against the numpy statement, not only the winner a call
returns.  After a call on a context the context's RANSAC scratch is read through hak_debug_ransac_scratch (include/hipakaze_test.h)
with 37 words per hypothesis and 3 x the call's iterations, at the shape hak_op_ransac_shape(npairs, 3 * iterations) reports, and
compared as tests/essential_trace.py says: the `valid` word of every virtual hypothesis, every word of every model with a bit and
the (inliers, hypothesis, model) of every score block -- on members of every scene family of test_essential_cpu.parity_case, the
degenerate ones and the ten-root members included, single and as ragged batch groups."""
import numpy as np
import pytest

import essential_trace as et
from test_essential_cpu import PARITY_CASES, PARITY_SCENES, parity_case
from test_gpu_fundamental import as_pairs, det, synth, torch, upload  # noqa: F401 (fixtures)
from test_ransac_shapes_cpu import shape_of

pytestmark = pytest.mark.gpu


def chosen():
    """the first case with a non-empty list of every scene family, then the cases with the most iterations, up to a dozen, and the
    two built ten-root members"""
    cases = [parity_case(k) for k in range(PARITY_CASES)]
    ks = []
    for scene in PARITY_SCENES:
        ks.append(next(k for k, c in enumerate(cases) if c["scene"] == scene and len(c["recs"]) >= 5))
    rest = sorted((k for k in range(PARITY_CASES - 2) if k not in ks and len(cases[k]["recs"]) >= 5),
                  key=lambda k: (-cases[k]["iterations"], k))
    ks += rest[:12 - len(ks)] + [PARITY_CASES - 2, PARITY_CASES - 1]
    return [(k, cases[k]) for k in ks]


def read_scratch(ah, ctx, npairs, iterations, hblocks):
    words = np.full(npairs * et.WORDS * 3 * iterations, 0xEEEEEEEE, np.uint32)
    slots = np.full(npairs * hblocks * 3, -7, np.int32)
    ah.check(ah.lib.hak_debug_ransac_scratch(ctx, npairs, et.WORDS, 3 * iterations, hblocks, words.ctypes.data, slots.ctypes.data))
    return words.reshape(npairs, et.WORDS, 3 * iterations), slots.reshape(npairs, hblocks, 3)


def test_every_hypothesis_and_slot_of_chosen_cases(ah, torch, det):
    fails = []
    compared = models = 0
    top = 0
    for k, c in chosen():
        hp, hblocks = shape_of(ah, 1, 3 * c["iterations"])
        tr = et.trace(c["recs"], c["K1"], c["K2"], c["iterations"], c["threshold"], c["seed"], hp, hblocks)
        lst = as_pairs(ah, c["recs"])
        rec = np.zeros((), ah.FUNDAMENTAL_DTYPE)
        k1, k2 = ah.intrinsics(c["K1"]), ah.intrinsics(c["K2"])
        ah.check(ah.lib.hak_find_essential(det.ctx, upload(torch, lst).data_ptr(), len(lst), k1.ctypes.data, k2.ctypes.data,
                                           c["iterations"], c["threshold"], c["seed"], None, rec.ctypes.data))
        words, slots = read_scratch(ah, det.ctx, 1, c["iterations"], hblocks)
        fails += [f"case {k} ({c['scene']}): {d}" for d in et.differences(tr, words[0], slots[0], 2)]
        if (int(rec["inliers"]), int(rec["hypothesis"]), int(rec["root"])) != et.record_of(tr, len(lst)):
            fails.append(f"case {k}: record {rec}, slots say {et.record_of(tr, len(lst))}")
        compared += c["iterations"]
        models += int(tr["valid"].sum())
        top = max(top, int(tr["valid"].reshape(-1, 12).sum(axis=1).max()))
    assert compared >= 1000 and models >= 1000 and top == 10, (compared, models, top)
    assert not fails, f"{len(fails)} differ: " + "; ".join(fails[:4])


def test_every_hypothesis_and_slot_of_the_ragged_groups(ah, torch, det):
    """the first three groups of four cases as one batch call each: [pair][word][3 iterations] models, [pair][block] slots at the
    batch's shape"""
    fails = []
    cases = [parity_case(k) for k in range(PARITY_CASES)]
    groups = sorted({c["group"] for c in cases if c["group"] >= 0})[:3]
    assert len(groups) == 3
    for g in groups:
        ks = [k for k, c in enumerate(cases) if c["group"] == g]
        c0 = cases[ks[0]]
        hp, hblocks = shape_of(ah, len(ks), 3 * c0["iterations"])
        lists = [as_pairs(ah, cases[k]["recs"]) for k in ks]
        stride = max(1, max(len(lst) for lst in lists))
        allp = np.zeros(len(ks) * stride, ah.MATCH_PAIR_DTYPE)
        for f in ("x1", "y1", "x2", "y2"):
            allp[f] = np.nan
        for slot, lst in enumerate(lists):
            allp[slot * stride:slot * stride + len(lst)] = lst
        d = upload(torch, allp)
        d_cnt = torch.tensor([len(lst) for lst in lists], dtype=torch.int32, device="cuda")
        d_out = torch.zeros(len(ks) * ah.FUNDAMENTAL_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        k1, k2 = ah.intrinsics(c0["K1"]), ah.intrinsics(c0["K2"])
        ah.check(ah.lib.hak_find_essential_batch(det.ctx, d.data_ptr(), stride, d_cnt.data_ptr(), len(ks), k1.ctypes.data, k2.ctypes.data,
                                                 c0["iterations"], c0["threshold"], c0["seed"], d_out.data_ptr(), None))
        words, slots = read_scratch(ah, det.ctx, len(ks), c0["iterations"], hblocks)
        for slot, k in enumerate(ks):
            tr = et.trace(cases[k]["recs"], c0["K1"], c0["K2"], c0["iterations"], c0["threshold"], c0["seed"], hp, hblocks)
            fails += [f"group {g} case {k}: {d}" for d in et.differences(tr, words[slot], slots[slot], 2)]
    assert not fails, f"{len(fails)} differ: " + "; ".join(fails[:4])
