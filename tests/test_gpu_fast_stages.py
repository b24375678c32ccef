"""GPU stage parity of the integer FAST path over the int32 VALUE domain: every hak_op_fast_* operator of include/hipakaze_test.h --
each drives the `int` launcher overload the FAST launch sequence calls -- against the oracle's stage functions (oracle/akaze_oracle_fast.c)
on the planes of tests/fast_domain.py: uint8-range, signed, blown up until sums of squares wrap, uniform random int32, INT_MIN / INT_MAX
blocks.  tests/test_fast_domain_cpu.py holds the conditions on those inputs and pins the oracle to int64 restatements and hand-derived
fixtures.

Comparison rule: np.array_equal on the int32 words of every output plane over the valid columns; contrast factor, lattice maximum and
all 300 histogram bins exactly.  No mask, no tolerance, no excluded case: the statement defines every value (wrapping products,
saturating conversions with NaN -> 0, arithmetic shifts).

Kernel families: as tests/conftest.py forces them (the register-streaming kernels), the tile fall-backs (HAK_HESS_STREAM = HAK_FUSE_SF =
HAK_BASE_STREAM = 0) and one FED step per launch (HAK_FED_MAX_FUSE = 1).  The operators read the knobs per call.  Every base test asserts
that the streaming prologue, kf_base and the unfused prologue were all reached, every Hessian test that the streaming kernel, the tile
kernel and the dilation > 4 passes were (the operators infer routes 1 and 2 from the launchers' cover rules, include/hipakaze_test.h).

FED cycles: the step lists of tests/value_domain.py have at most 4 steps -- one launch under the FAST group rule -- so fast_domain adds a
7-step list (two launches of 4 + 3: the ping-pong through d_tmp) and, for the tile kernel, a 37-step list (19 + 18: the continuation
launch k_level_tile<int, false, false>).  The k_fed_sf cycle writes its conductivity plane only when a later launch of the cycle reads
it, i.e. for the 7-step list in every family and for every list of more than one step under HAK_FED_MAX_FUSE = 1; it is compared then
and only then.
"""
import ctypes as C
import numpy as np
import pytest

import fast_domain as fd
from conftest import assert_points_equal

pytestmark = pytest.mark.gpu

TILE = {"HAK_HESS_STREAM": "0", "HAK_FUSE_SF": "0", "HAK_BASE_STREAM": "0"}
FAMILIES = {"streaming": {}, "tile": TILE, "one_step": {"HAK_FED_MAX_FUSE": "1"}}
_fp, _ip = C.POINTER(C.c_float), C.POINTER(C.c_int)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


# one case list per (operator, generator): the oracle is evaluated once and shared by the three families, which run back to back
_cases = {}


def cases_of(okz, op, name):
    key = (op, name)
    if key not in _cases:
        _cases.clear()
        gen = fd.u8_stage_cases if name in fd.U8_GENERATORS else fd.stage_cases
        _cases[key] = [(w, h, c) for w, h in fd.shapes_of(op) for c in gen(okz, name, w, h, ops=(op,))]
    return _cases[key]


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def izeros(torch, *shape):
    return torch.zeros(shape, dtype=torch.int32, device="cuda")


def taus_of(args):
    t = np.array(args["taus"], np.float32)
    return t, t.ctypes.data_as(_fp)


def slots(torch, planes, n, S):
    """n slots of len(planes) image planes, S elements apart, in ONE allocation (the streaming kernels address their output planes as
    32-bit offsets from the lowest one); slot 0 holds `planes`"""
    B = len(planes)
    buf = np.zeros((n, B, S), np.int32)
    for i, q in enumerate(planes):
        buf[0, i, :q.size] = q.ravel()
    return dev(torch, buf)


def unslot(buf, k, i, h, p):
    return buf[k, i, :h * p].reshape(h, p).cpu().numpy()


def run_op(ah, torch, op, w, h, args, family):
    """the HIP operator of one stage case -> (outputs in the order of the case's oracle outputs, extra (name, got, want, width) checks)"""
    lib = ah.lib
    extra = []
    if op in ("conv_u8", "base"):
        u8 = args["u8"]
        p = u8.shape[1]
        d_u8, d = dev(torch, u8), izeros(torch, h, p)
        if op == "conv_u8":
            ah.check(lib.hak_op_fast_conv_u8(d_u8.data_ptr(), p, d.data_ptr(), w, h, p, args["var"], args["R"]))
            return [d.cpu().numpy()], extra
        kc, hmax, route = C.c_int(), C.c_int(), C.c_int()
        hist = np.zeros(300, np.int32)
        ah.check(lib.hak_op_fast_base(d_u8.data_ptr(), p, d.data_ptr(), w, h, p, args["var"], args["R"], fd.PER, C.byref(kc), C.byref(hmax),
                                      hist.ctypes.data_as(_ip), C.byref(route)))
        args["route"] = route.value
        return [d.cpu().numpy(), np.array([kc.value, hmax.value], np.int32), hist], extra
    a = args["a"]
    p = a.shape[-1]
    if op == "lowpass":
        d_a, d = dev(torch, a), izeros(torch, h, p)
        ah.check(lib.hak_op_fast_lowpass(d_a.data_ptr(), d.data_ptr(), w, h, p, args["var"], args["R"]))
        return [d.cpu().numpy()], extra
    if op == "down_smooth":
        dw, dh, dp = args["dw"], args["dh"], args["dp"]
        d_a, d_dst, d_sm = dev(torch, a), izeros(torch, dh, dp), izeros(torch, dh, dp)
        ah.check(lib.hak_op_fast_down_smooth(d_a.data_ptr(), d_dst.data_ptr(), d_sm.data_ptr(), w, h, p, dw, dh, dp))
        return [d_dst.cpu().numpy(), d_sm.cpu().numpy()], extra
    if op == "kcontrast":
        kc, hmax = C.c_int(), C.c_int()
        hist = np.zeros(300, np.int32)
        d_a = dev(torch, a)
        ah.check(lib.hak_op_fast_kcontrast(d_a.data_ptr(), w, h, p, fd.PER, C.byref(kc), C.byref(hmax), hist.ctypes.data_as(_ip)))
        return [np.array([kc.value, hmax.value], np.int32), hist], extra
    if op == "flow":
        d_a, d = dev(torch, a), izeros(torch, h, p)
        ah.check(lib.hak_op_fast_flow(d_a.data_ptr(), d.data_ptr(), w, h, p, args["diff"], args["kc"]))
        return [d.cpu().numpy()], extra
    if op == "smooth_flow":
        buf = slots(torch, [a], 3, h * p)
        ah.check(lib.hak_op_fast_smooth_flow(buf[0].data_ptr(), buf[1].data_ptr(), buf[2].data_ptr(), w, h, p, args["diff"], args["kc"]))
        return [unslot(buf, 1, 0, h, p), unslot(buf, 2, 0, h, p)], extra
    if op == "nld_steps":
        t, tp = taus_of(args)
        d_a, d_g, d_dst, d_tmp = dev(torch, a), dev(torch, args["g"]), izeros(torch, h, p), izeros(torch, h, p)
        ah.check(lib.hak_op_fast_nld_steps(d_a.data_ptr(), d_g.data_ptr(), d_dst.data_ptr(), d_tmp.data_ptr(), w, h, p, tp, len(t)))
        return [d_dst.cpu().numpy()], extra
    if op == "nld_steps_batch":
        t, tp = taus_of(args)
        B, S = len(a), h * p
        d_a, d_g, d_dst, d_tmp = dev(torch, a), dev(torch, args["g"]), izeros(torch, B, h, p), izeros(torch, B, h, p)
        ah.check(lib.hak_op_fast_nld_steps_batch(d_a.data_ptr(), d_g.data_ptr(), d_dst.data_ptr(), d_tmp.data_ptr(), S, w, h, p, B, tp, len(t)))
        outs = [d_dst[i].cpu().numpy() for i in range(B)]
        for i in range(B):                                  # image i of the batch call == the single-image call on plane i
            d1, t1 = izeros(torch, h, p), izeros(torch, h, p)
            ah.check(lib.hak_op_fast_nld_steps(d_a[i].data_ptr(), d_g[i].data_ptr(), d1.data_ptr(), t1.data_ptr(), w, h, p, tp, len(t)))
            extra.append((f"single call on plane {i}", d1.cpu().numpy(), outs[i], w))
        return outs, extra
    if op in ("fed_cycle", "level_tile"):
        t, tp = taus_of(args)
        B, head, dw, dh, dp = len(a), args["head"], args["dw"], args["dh"], args["dp"]
        S = h * p                                           # (a head's source planes are the larger ones)
        kc = (C.c_int * B)(*args["kc"])

        def call(planes, kcs):
            buf = slots(torch, planes, 5, S)                # src, smooth, flow, dst, tmp
            src, sm, fl, dst, tmp = (buf[k].data_ptr() for k in range(5))
            n = len(planes)
            if op == "fed_cycle":
                ah.check(lib.hak_op_fast_fed_cycle(src, head, w, h, p, sm, fl, dst, tmp, S, dw, dh, dp, n, kcs, tp, len(t)))
            else:
                nl = C.c_int()
                ah.check(lib.hak_op_fast_level_tile(src, head, w, h, p, sm, dst, tmp, S, dw, dh, dp, n, args["diff"], kcs, tp, len(t), C.byref(nl)))
                # the 37-step list exists to reach the continuation launch: two launches, every other list one
                assert nl.value == (2 if args["taus"] is fd.LONG_TAUS else 1), (nl.value, len(t))
            return buf
        buf = call(list(a), kc)
        outs = [unslot(buf, 1, i, dh, dp) for i in range(B)] + [unslot(buf, 3, i, dh, dp) for i in range(B)]
        if op == "fed_cycle" and len(t) > (1 if family == "one_step" else 4):      # a later launch of the cycle reads the conductivity
            extra += [(f"flow[{i}]", unslot(buf, 2, i, dh, dp), args["g"][i], dw) for i in range(B)]
        for i in range(B):
            one = call([a[i]], (C.c_int * 1)(args["kc"][i]))
            extra.append((f"single call on plane {i}: smooth", unslot(one, 1, 0, dh, dp), outs[i], dw))
            extra.append((f"single call on plane {i}: L", unslot(one, 3, 0, dh, dp), outs[B + i], dw))
        return outs, extra
    if op == "hessian":
        d_a = dev(torch, a)
        outs = [izeros(torch, h, p) for _ in range(3)]
        route = C.c_int()
        ah.check(lib.hak_op_fast_hessian(d_a.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), w, h, p, args["step"], C.byref(route)))
        args["route"] = route.value
        return [o.cpu().numpy() for o in outs], extra
    raise ValueError(op)


def differ(what, got, want, width):
    got, want = np.asarray(got), np.asarray(want)
    if width is not None:
        got, want = got[..., :width], want[..., :width]
    if got.dtype == want.dtype and np.array_equal(got, want):
        return None
    bad = np.argwhere(got != want)
    first = tuple(int(v) for v in bad[0])
    return f"{what}: {len(bad)} words differ, first at {first}: got {got[first]!r}, oracle {want[first]!r}"


def run_family(ah, okz, torch, monkeypatch, op, name, family):
    for k, v in FAMILIES[family].items():
        monkeypatch.setenv(k, v)
    fails, routes = [], set()
    for w, h, (_, label, args, want) in cases_of(okz, op, name):
        got, extra = run_op(ah, torch, op, w, h, args, family)
        assert len(got) == len(want)
        for (nm, ref, ww), out in zip(want, got):
            msg = differ(f"{name} {w}x{h} {family} {op} {label} {nm}", out, ref, ww)
            if msg:
                fails.append(msg)
        for nm, out, ref, ww in extra:
            msg = differ(f"{name} {w}x{h} {family} {op} {label} {nm}", out, ref, ww)
            if msg:
                fails.append(msg)
        routes.add(args.get("route"))
    assert not fails, "\n".join(fails[:12] + ([f"... {len(fails)} mismatches"] if len(fails) > 12 else []))
    return routes


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("name", list(fd.GENERATORS))
@pytest.mark.parametrize("op", fd.OPS)
def test_fast_stage(ah, okz, torch, monkeypatch, op, name, family):
    routes = run_family(ah, okz, torch, monkeypatch, op, name, family)
    if op == "hessian":                                     # 1 streaming, 2 tile, 3 dilation > 4
        assert routes == ({2, 3} if family == "tile" else {1, 2, 3}), routes


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("name", list(fd.U8_GENERATORS))
@pytest.mark.parametrize("op", fd.U8_OPS)
def test_fast_u8_stage(ah, okz, torch, monkeypatch, op, name, family):
    routes = run_family(ah, okz, torch, monkeypatch, op, name, family)
    if op == "base":                                        # 1 streaming prologue, 2 kf_base, 3 unfused
        assert routes == ({2, 3} if family == "tile" else {1, 2, 3}), routes


# ------------------------------------------------------------------------------------------------ the wrapped states through the real sequence
# 640 x 640 is the smallest extent with four octaves, and it takes the fourth: at 320 x 240 (two octaves) no plane leaves +-2^11 under any
# parameters hak_create accepts (soffset <= 2.0: base kernels of at most 11 taps), at three octaves Lt reaches 1e5 but no plane 2^24
PIPE_WH = (640, 640)
PIPE = dict(noctaves=4, max_scale=3, soffset=2.0, reordering=False, derivative_factor=0.5, diffusivity=3)
PIPE_SEEDS = (5, 6)
PIPE_MAX_PTS = 5000
_pipe_ref = {}


def pipe_oracle(okz, w, h):
    """long FED cycles in ascending step order (reordering off) from the largest base scale the library takes: octaves 2 and 3 leave the
    uint8 range by orders of magnitude, and from there on the level sequence runs on wrapped sums of squares"""
    if not _pipe_ref:
        for seed in PIPE_SEEDS:
            u8 = fd.u8_scene(w, h, seed)
            prm = okz.default_params(**{k: (int(v) if isinstance(v, bool) else v) for k, v in PIPE.items()})
            r = okz.fast_detect_and_compute(u8, prm, max_pts=PIPE_MAX_PTS, keep_arena=True)
            _pipe_ref[seed] = (u8, r)
    return _pipe_ref


@pytest.mark.parametrize("selection", ["default", "level_tile"])
def test_pipeline_with_a_blown_coarse_level(ah, okz, torch, monkeypatch, selection):
    if selection == "level_tile":
        monkeypatch.setenv("HAK_LEVEL_TILE", "2")
    w, h = PIPE_WH
    p = ah.iAlignUp(w, 128)
    refs = pipe_oracle(okz, w, h)
    B = len(PIPE_SEEDS)
    for seed, (u8, r) in refs.items():
        # checked on the CPU first: a plane value beyond +-2^24, a scale-space plane beyond anything a uint8 image holds, and a wrapped
        # Scharr sum of squares of the plane the conductivity of the last level is taken of
        planes = [okz.plane(r, kind, o, s).astype(np.int64) for o in range(r.noct) for s in range(r.ms) for kind in range(4)]
        assert max(int(np.abs(q).max()) for q in planes) > 2 ** 24
        last = okz.plane(r, 0, r.noct - 1, r.ms - 2)
        assert np.abs(last.astype(np.int64)).max() > 2 ** 12
        A = fd.Arith(True)
        fd.np_scharr(A, fd.np_conv(fd.Arith(True), last, okz.fast_gauss_taps(1.0, 2), 2))
        assert A.out_of_range > 0
        assert 50 < len(r.points) < PIPE_MAX_PTS and r.points["octave"].max() >= r.ms
    stack = np.zeros((B, h, p), np.uint8)
    for i, seed in enumerate(PIPE_SEEDS):
        stack[i, :, :w] = refs[seed][0]
    d_img = dev(torch, stack)
    d_pts = torch.zeros(B * PIPE_MAX_PTS * 104, dtype=torch.uint8, device="cuda")
    d_num = torch.zeros(B, dtype=torch.int32, device="cuda")
    det = ah.Akazer()
    det.init((w, h, p), max_pts=PIPE_MAX_PTS, batch=B, **PIPE)
    try:
        ah.check(ah.lib.hak_fast_detect_and_compute_batch(det.ctx, d_img.data_ptr(), h * p, p, B, d_pts.data_ptr(), d_num.data_ptr(), 1))
        ah.check(ah.lib.hak_sync(det.ctx))
        nums = d_num.cpu().numpy()
        allp = d_pts.cpu().numpy().view(ah.POINT_DTYPE).reshape(B, PIPE_MAX_PTS)
        fails = []
        for i, seed in enumerate(PIPE_SEEDS):
            r = refs[seed][1]
            assert len(det.geometry()) == r.noct
            for o in range(r.noct):
                for s in range(r.ms):
                    for kind, nm in ((0, "Lt"), (2, "Lx"), (3, "Ly"), (1, "det")):
                        msg = differ(f"image {i} {selection} {nm}({o},{s})", det.plane(kind, o, s, i).view(np.int32), okz.plane(r, kind, o, s), None)
                        if msg:
                            fails.append(msg)
        assert not fails, "\n".join(fails[:12])
        for i, seed in enumerate(PIPE_SEEDS):
            assert_points_equal(allp[i, :min(nums[i], PIPE_MAX_PTS)], refs[seed][1].points)
    finally:
        det.close()
