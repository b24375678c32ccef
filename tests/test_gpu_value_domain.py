"""GPU parity over the VALUE domain: every stage operator of include/hipakaze_test.h and the whole pipeline against the oracle on
float32 content that is not "uint8 scene / 255" (tests/value_domain.py): full-mantissa, dark, subnormal, signed zeros, large, overflowing
and non-finite planes.  tests/test_value_domain_cpu.py holds the conditions on those inputs (tier A finite, at least half of every
tier-B / C output non-NaN, `spikes` on both sides of 2^64 in one row segment).

Comparison rule (value_domain.same_bits): two float32 arrays agree iff at each element the uint32 words are equal or both are NaN; -0
and +0 are different words.  A tier-A case additionally asserts that NO element passed by the NaN clause.  Stage cases with a contrast
factor of KC_EXTREME (1e-30, 1e30) are tier B whatever their input.  There is no other exclusion and no mask: the reference defines
every compared value (float -> int conversions follow the device cast, oracle/README.md).

Kernel families: as tests/conftest.py forces them (register-streaming kernels) and the tile fall-backs (HAK_HESS_STREAM = HAK_FUSE_SF =
HAK_BASE_STREAM = 0); the pipeline also with one launch per sublevel (HAK_LEVEL_TILE = 2).  Stage operators read the knobs per call,
contexts at hak_create.

The tier-C tests (non-finite input pixels) are the last functions of the file and carry `tierC` in their names: run the finite tiers
first (-k "not tierC"), tier C in an invocation of its own (-k tierC).  HAK_VD_REPORT=<file> writes the case and NaN-clause counts per
tier when the module finishes.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import retain_best_ref as rb
import value_domain as vd

pytestmark = pytest.mark.gpu

SEED = 5
TILE = {"HAK_HESS_STREAM": "0", "HAK_FUSE_SF": "0", "HAK_BASE_STREAM": "0"}
FAMILIES = {"streaming": {}, "tile": TILE}
SELECTIONS = {"streaming": {}, "level_tile": {"HAK_LEVEL_TILE": "2"}, "tile": TILE}
PIPE_SHAPES = [(320, 240), (1284, 200)]
FINITE = vd.TIERS["A"] + vd.TIERS["B"]
FLOAT_FIELDS = ("x", "y", "response", "size", "angle")
MAX_PTS = 5000
TALLY = {t: dict(cases=0, nan_clause=0, elements=0) for t in "ABC"}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module", autouse=True)
def _report():
    with np.errstate(all="ignore"):
        yield
    if os.environ.get("HAK_VD_REPORT"):
        with open(os.environ["HAK_VD_REPORT"], "w") as f:
            json.dump(TALLY, f)


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def zeros(torch, h, p):
    return torch.zeros((h, p), dtype=torch.float32, device="cuda")


class Cmp:
    """collects the mismatches of one test; every comparison goes through value_domain.same_bits"""

    def __init__(self, tier):
        self.tier, self.fails = tier, []

    def planes(self, what, got, want, tier=None):
        tier = tier or self.tier
        ok, nnan, first = vd.same_bits(got, want)
        TALLY[tier]["cases"] += 1
        TALLY[tier]["nan_clause"] += nnan
        TALLY[tier]["elements"] += int(np.asarray(want).size)
        if not ok:
            g, w = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
            self.fails.append(f"{what}: differs at {first}: got {g[first]!r} ({g.view(np.uint32)[first]:#010x}), oracle {w[first]!r} "
                              f"({w.view(np.uint32)[first]:#010x}); {int((g.view(np.uint32) != w.view(np.uint32)).sum())} words differ")
        if tier == "A" and nnan:
            self.fails.append(f"{what}: {nnan} elements of a tier-A case passed by the NaN clause")

    def exact(self, what, got, want):
        if not np.array_equal(got, want):
            self.fails.append(f"{what}: {got!r} != {want!r}" if np.ndim(got) == 0 else f"{what}: {int((np.asarray(got) != np.asarray(want)).sum())} entries differ")

    def points(self, what, got, want, fields=FLOAT_FIELDS):
        if len(got) != len(want):
            self.fails.append(f"{what}: {len(got)} keypoints, oracle {len(want)}")
            return
        if not len(got):
            return
        for f in fields:
            self.planes(f"{what} field {f}", got[f], want[f])
        self.exact(f"{what} field octave", got["octave"], want["octave"])
        bad = (got["features"] != want["features"]).any(axis=1).sum()
        if bad:
            self.fails.append(f"{what}: descriptor bits differ at {int(bad)} of {len(got)} points")

    def done(self):
        assert not self.fails, "\n".join(self.fails[:12] + ([f"... {len(self.fails)} mismatches"] if len(self.fails) > 12 else []))


# ------------------------------------------------------------------------------------------------ stage level
def run_op(ah, torch, op, a, w, args):
    """the HIP operator of one stage case on the pitched plane `a` -> outputs in the order of value_domain.oracle_stage_cases"""
    h, p = a.shape
    lib = ah.lib
    d_a = dev(torch, a)
    if op == "lowpass":
        d = zeros(torch, h, p)
        ah.check(lib.hak_op_lowpass(d_a.data_ptr(), d.data_ptr(), w, h, p, args["var"], args["R"]))
        return [d.cpu().numpy()]
    if op == "down_smooth":
        dw, dh, dp = args["dw"], args["dh"], args["dp"]
        d_dst, d_sm = zeros(torch, dh, dp), zeros(torch, dh, dp)
        ah.check(lib.hak_op_down_smooth(d_a.data_ptr(), d_dst.data_ptr(), d_sm.data_ptr(), w, h, p, dw, dh, dp))
        return [d_dst.cpu().numpy(), d_sm.cpu().numpy()]
    if op == "kcontrast":
        kc, hmax = C.c_float(), C.c_float()
        hist = np.zeros(300, np.int32)
        d_sm = dev(torch, args["sm"])
        ah.check(lib.hak_op_kcontrast(d_sm.data_ptr(), w, h, p, vd.PER, C.byref(kc), C.byref(hmax), hist.ctypes.data_as(C.POINTER(C.c_int))))
        return [np.array([[kc.value, hmax.value]], np.float32), hist]
    if op == "flow":
        d = zeros(torch, h, p)
        ah.check(lib.hak_op_flow(d_a.data_ptr(), d.data_ptr(), w, h, p, args["diff"], args["kc"]))
        return [d.cpu().numpy()]
    if op == "smooth_flow":
        d_sm, d_g = zeros(torch, h, p), zeros(torch, h, p)
        ah.check(lib.hak_op_smooth_flow(d_a.data_ptr(), d_sm.data_ptr(), d_g.data_ptr(), w, h, p, args["diff"], args["kc"]))
        return [d_sm.cpu().numpy(), d_g.cpu().numpy()]
    if op == "nld_steps":
        d_g, d_dst, d_tmp = dev(torch, args["g"]), zeros(torch, h, p), zeros(torch, h, p)
        t = np.array(args["taus"], np.float32)
        ah.check(lib.hak_op_nld_steps(d_a.data_ptr(), d_g.data_ptr(), d_dst.data_ptr(), d_tmp.data_ptr(), w, h, p,
                                      t.ctypes.data_as(C.POINTER(C.c_float)), len(t)))
        return [d_dst.cpu().numpy()]
    if op == "hessian":
        outs = [zeros(torch, h, p) for _ in range(3)]
        ah.check(lib.hak_op_hessian(d_a.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), w, h, p, args["step"]))
        return [o.cpu().numpy() for o in outs]
    raise ValueError(op)


def stage_cases(ah, okz, torch, monkeypatch, op, name, family):
    for k, v in FAMILIES[family].items():
        monkeypatch.setenv(k, v)
    g = vd.GENERATORS[name]
    cmp = Cmp(g.tier)
    for w, h in vd.STAGE_SHAPES:
        a = vd.pitched(g(w, h, SEED))
        for _, label, extreme, args, want in vd.oracle_stage_cases(okz, a, w, ops=(op,)):
            got = run_op(ah, torch, op, a, w, args)
            tier = "B" if (extreme and g.tier == "A") else g.tier
            for (nm, ref, ww), out in zip(want, got):
                what = f"{name} {w}x{h} {family} {op} {label} {nm}"
                if ref.dtype == np.float32:
                    cmp.planes(what, out[:, :ww], ref[:, :ww], tier)
                else:
                    cmp.exact(what, out, ref)
    cmp.done()


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("name", FINITE)
@pytest.mark.parametrize("op", vd.OPS)
def test_stage_finite_tiers(ah, okz, torch, monkeypatch, op, name, family):
    stage_cases(ah, okz, torch, monkeypatch, op, name, family)


# ------------------------------------------------------------------------------------------------ pipeline level
_oracle_cache = {}


def oracle_run(okz, name, w, h, dthreshold=None, max_pts=MAX_PTS):
    key = (name, w, h, dthreshold, max_pts)
    if key not in _oracle_cache:
        p = (w + 127) // 128 * 128
        kw = {} if dthreshold is None else dict(dthreshold=dthreshold)
        img = vd.pitched(vd.GENERATORS[name](w, h, SEED), p)
        _oracle_cache[key] = (img, okz.detect_and_compute(img, w, okz.default_params(**kw), max_pts=max_pts, keep_arena=True))
    return _oracle_cache[key]


def compare_image(ah, okz, cmp, det, ref, what, got_pts, img=0):
    """every plane of every level, the contrast factor, the count and every record field of one image of the last call"""
    assert len(det.geometry()) == ref.noct
    for o in range(ref.noct):
        for s in range(ref.ms):
            for kind, nm in ((0, "Lt"), (2, "Lx"), (3, "Ly"), (1, "det")):
                cmp.planes(f"{what} {nm}({o},{s})", det.plane(kind, o, s, img), okz.plane(ref, kind, o, s))
    cmp.planes(f"{what} contrast factor", np.array([det.kcontrast(img)], np.float32), np.array([ref.kcontrast], np.float32))
    cmp.points(what, got_pts, ref.points)


def pipeline_case(ah, okz, torch, monkeypatch, name, w, h, selection, dthreshold=None, min_pts=0):
    for k, v in SELECTIONS[selection].items():
        monkeypatch.setenv(k, v)
    p = ah.iAlignUp(w, 128)
    img, ref = oracle_run(okz, name, w, h, dthreshold)
    assert len(ref.points) >= min_pts and len(ref.points) < MAX_PTS
    kw = {} if dthreshold is None else dict(dthreshold=dthreshold)
    det = ah.Akazer()
    det.init((w, h, p), max_pts=MAX_PTS, **kw)
    data = ah.AkazeData()
    ah.initAkazeData(data, MAX_PTS, True, True)
    try:
        d_img = dev(torch, img)
        det.detectAndCompute(d_img.data_ptr(), data, (w, h, p), True)
        cmp = Cmp(vd.GENERATORS[name].tier)
        compare_image(ah, okz, cmp, det, ref, f"{name} {w}x{h} {selection}", data.h_data[:min(data.num_pts, MAX_PTS)].copy())
        cmp.done()
    finally:
        ah.freeAkazeData(data)
        det.close()


@pytest.mark.parametrize("selection", list(SELECTIONS))
@pytest.mark.parametrize("w,h", PIPE_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("name", FINITE)
def test_pipeline_finite_tiers(ah, okz, torch, monkeypatch, name, w, h, selection):
    pipeline_case(ah, okz, torch, monkeypatch, name, w, h, selection)


@pytest.mark.parametrize("selection", list(SELECTIONS))
@pytest.mark.parametrize("name", list(vd.LOW_DTHRESHOLD))
def test_pipeline_small_amplitude_with_a_low_threshold(ah, okz, torch, monkeypatch, name, selection):
    """no keypoints at the default threshold: again with the threshold at which the oracle finds > 50 (value_domain.LOW_DTHRESHOLD)"""
    pipeline_case(ah, okz, torch, monkeypatch, name, 320, 240, selection, dthreshold=vd.LOW_DTHRESHOLD[name], min_pts=51)


def test_pair_of_hdr_and_x255_with_match(ah, okz, torch):
    """hak_detect_and_compute_pair on two value ranges at once == the oracle's two detections + okz.match"""
    w, h = 320, 240
    p = ah.iAlignUp(w, 128)
    (i1, r1), (i2, r2) = oracle_run(okz, "hdr", w, h), oracle_run(okz, "x255", w, h)
    a, b = r1.points.copy(), r2.points
    okz.match(a, b)
    det = ah.Akazer()
    det.init((w, h, p), max_pts=MAX_PTS, batch=2)
    d1, d2 = ah.AkazeData(), ah.AkazeData()
    ah.initAkazeData(d1, MAX_PTS, True, True)
    ah.initAkazeData(d2, MAX_PTS, True, True)
    try:
        t1, t2 = dev(torch, i1), dev(torch, i2)
        det.detectAndComputePair(t1.data_ptr(), t2.data_ptr(), d1, d2, (w, h, p), True, True)
        cmp = Cmp(vd.GENERATORS["hdr"].tier)                                       # (tier A: no element may pass by the NaN clause)
        g1, g2 = d1.h_data[:d1.num_pts], d2.h_data[:d2.num_pts]
        cmp.points("pair image 1 (hdr)", g1, a, FLOAT_FIELDS + ("match_x", "match_y"))
        cmp.tier = vd.GENERATORS["x255"].tier
        cmp.points("pair image 2 (x255)", g2, b)
        if len(g1) == len(a):
            cmp.exact("match", g1["match"], a["match"])
            cmp.exact("distance", g1["distance"], a["distance"])
        assert (a["match"] >= 0).sum() > 20
        cmp.done()
    finally:
        ah.freeAkazeData(d1)
        ah.freeAkazeData(d2)
        det.close()


def test_retain_best_on_x255(ah, okz, torch):
    """the strongest-N selection on responses 255^2 times those of [0, 1] content: the order-preserving key map on real output of
    another range, against tests/retain_best_ref.py"""
    w, h, cap = 320, 240, 300
    p = ah.iAlignUp(w, 128)
    img, ref = oracle_run(okz, "x255", w, h)
    full = ref.points
    assert len(full) > 2 * cap and full["response"].max() > 100
    want = rb.retain(full, cap)
    assert not np.array_equal(rb.retained(full, cap), np.arange(cap))
    det = ah.Akazer()
    det.init((w, h, p), max_pts=MAX_PTS, retain_best=True)
    data = ah.AkazeData()
    ah.initAkazeData(data, cap, True, True)
    try:
        d_img = dev(torch, img)
        det.detectAndCompute(d_img.data_ptr(), data, (w, h, p), True)
        got = data.h_data[:data.num_pts].copy()
        assert len(got) == cap
        assert got.tobytes() == want.tobytes(), int((got.view(np.uint8).reshape(cap, -1) != want.view(np.uint8).reshape(cap, -1)).any(1).sum())
    finally:
        ah.freeAkazeData(data)
        det.close()


# ------------------------------------------------------------------------------------------------ tier C: non-finite pixels (run last, on its own)
@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("name", vd.TIERS["C"])
@pytest.mark.parametrize("op", vd.OPS)
def test_tierC_stage(ah, okz, torch, monkeypatch, op, name, family):
    stage_cases(ah, okz, torch, monkeypatch, op, name, family)


@pytest.mark.parametrize("selection", list(SELECTIONS))
@pytest.mark.parametrize("w,h", PIPE_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("name", vd.TIERS["C"])
def test_tierC_pipeline(ah, okz, torch, monkeypatch, name, w, h, selection):
    pipeline_case(ah, okz, torch, monkeypatch, name, w, h, selection)


BATCH_CLASSES = ("hdr", "nan_frame", "sub_squares", "spikes", "x255", "one_inf", "signed_zero", "x1e18")


@pytest.mark.parametrize("selection", list(SELECTIONS))
def test_tierC_batch_of_mixed_classes(ah, okz, torch, monkeypatch, selection):
    """one hak_detect_and_compute_batch of 8 images, one class each, all three tiers side by side: an image's special values must not
    reach its neighbours through a wave-level decision or a shared histogram -- every slot equals its single-image oracle result"""
    for k, v in SELECTIONS[selection].items():
        monkeypatch.setenv(k, v)
    w, h, B = 320, 240, len(BATCH_CLASSES)
    p = ah.iAlignUp(w, 128)
    runs = [oracle_run(okz, n, w, h) for n in BATCH_CLASSES]
    stack = dev(torch, np.stack([img for img, _ in runs]))
    d_pts = torch.zeros(B * MAX_PTS * 104, dtype=torch.uint8, device="cuda")
    d_num = torch.zeros(B, dtype=torch.int32, device="cuda")
    det = ah.Akazer()
    det.init((w, h, p), max_pts=MAX_PTS, batch=B)
    try:
        ah.check(ah.lib.hak_detect_and_compute_batch(det.ctx, stack.data_ptr(), h * p, p, B, d_pts.data_ptr(), d_num.data_ptr(), 1))
        ah.check(ah.lib.hak_sync(det.ctx))
        nums = d_num.cpu().numpy()
        allp = d_pts.cpu().numpy().view(ah.POINT_DTYPE).reshape(B, MAX_PTS)
        cmp = Cmp("C")
        for i, n in enumerate(BATCH_CLASSES):
            cmp.tier = vd.GENERATORS[n].tier
            compare_image(ah, okz, cmp, det, runs[i][1], f"batch slot {i} ({n}) {selection}", allp[i, :min(nums[i], MAX_PTS)], img=i)
        cmp.done()
    finally:
        det.close()
