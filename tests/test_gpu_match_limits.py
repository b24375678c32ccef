"""GPU suite: the matchers at the limits of their packed keys -- the families of tests/match_limits.py through hak_match,
hak_match_knn2, their batch forms, hak_match_guided and hak_match_epipolar, under the three kernel selections, with a context and without one, bit for bit against the
expectations that tests/test_match_limits_cpu.py holds to the oracle.  Before it compares, every case asserts with the library's own
launch plan (hak_op_match_shape) that the call takes the path the case was made for: the vector-pipe kernels on 2^20 - 1 rows, one
block walking 2047 chunks, 512 slices, a slice count that is no multiple of 8, 1024 finish blocks, the switch at 393 025 rows.
Compared per call: the four match fields, the 2-NN list field by field and its count, the device copy of records and list against
the host copy, the bytes of the train set after the call.  Measured times: profiles/match_limits.txt."""
import ctypes as C

import numpy as np
import pytest

import match_limits as ml
from match_limits import assert_fields, assert_list, family, plan_of, seam_rows

pytestmark = pytest.mark.gpu
RATIO = (4, 5)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(params=["0", "qt2", "1"], ids=["k_match_mfma", "k_match_mfma 64-query waves", "k_match (VALU)"])
def match_kernel(request, monkeypatch):
    """the matcher kernels (as in test_gpu_pipeline.py): the matrix-core one (32-query waves; HAK_MATCH_QT=2: 64-query waves) and
    the vector-pipe one (HAK_MATCH_VALU=1); both variables are read per call"""
    monkeypatch.setenv("HAK_MATCH_VALU", "1" if request.param == "1" else "0")
    monkeypatch.setenv("HAK_MATCH_QT", "2" if request.param == "qt2" else "1")
    monkeypatch.delenv("HAK_MATCH_SLICES", raising=False)
    return request.param


@pytest.fixture
def context(request, ah):
    """None (the scratch comes from the per-device pool) or a context (its own scratch and stream)"""
    if not request.param:
        yield None
        return
    det = ah.Akazer()
    det.init((320, 240, 384), max_pts=1000)
    yield det.ctx
    det.close()


def upload(torch, recs):
    return torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).cuda()


def download(ah, t, dtype=None):
    return np.frombuffer(t.cpu().numpy().tobytes(), dtype or ah.POINT_DTYPE)


def run_match(ah, torch, F, ctx, want=None):
    """hak_match on the family -> the host copy of the records (all comparisons of the module docstring made)"""
    d1, d2 = upload(torch, F.queries), upload(torch, F.train)
    out = F.queries.copy()
    ah.check(ah.lib.hak_match(ctx, d1.data_ptr(), len(F.queries), d2.data_ptr(), len(F.train), out.ctypes.data))
    assert_fields(out, F.expect_match() if want is None else want, F.name + " hak_match")
    assert download(ah, d1).tobytes() == out.tobytes(), "device records != host copy"
    assert download(ah, d2).tobytes() == F.train.tobytes(), "the train set was written"
    del d1, d2
    return out


def run_knn2(ah, torch, F, ctx, cross):
    n1 = len(F.queries)
    d1, d2 = upload(torch, F.queries), upload(torch, F.train)
    d_out = torch.zeros(n1 * 32, dtype=torch.uint8, device="cuda")
    h_out = np.zeros(n1, ah.MATCH_PAIR_DTYPE)
    h_pts = F.queries.copy()
    cnt = C.c_int(-1)
    ah.check(ah.lib.hak_match_knn2(ctx, d1.data_ptr(), n1, d2.data_ptr(), len(F.train), RATIO[0], RATIO[1], int(cross), 0,
                                   h_pts.ctypes.data, d_out.data_ptr(), C.byref(cnt), h_out.ctypes.data))
    want, wlst = F.expect_knn2(RATIO, cross)
    what = f"{F.name} hak_match_knn2 cross={cross}"
    assert cnt.value == len(wlst), (what, cnt.value, len(wlst))
    assert_list(h_out[:cnt.value], wlst, what)
    assert_fields(h_pts, want, what)
    assert download(ah, d_out, ah.MATCH_PAIR_DTYPE)[:cnt.value].tobytes() == h_out[:cnt.value].tobytes(), "device list != host copy"
    assert download(ah, d1).tobytes() == h_pts.tobytes(), "device records != host copy"
    assert download(ah, d2).tobytes() == F.train.tobytes(), "the train set was written"
    del d1, d2, d_out
    return h_pts, h_out[:cnt.value]


# ------------------------------------------------------------------ index_bits
@pytest.mark.parametrize("n1,context", [(33, False), (129, False), (129, True)], indirect=["context"],
                         ids=["33 queries", "129 queries", "129 queries, context"])
def test_index_bits(ah, torch, match_kernel, n1, context):
    """2^20 - 1 train rows: every index bit of the key in k_match (sliced: the atomicMin merge and k_match_finish), in k_knn2 and in
    the reverse search's records"""
    F = family("index_bits", ml.NMAX, n1)
    p = plan_of(0, n1, ml.NMAX)
    assert p["kernel"] == 1 and p["slices"] > 1, p                 # beyond MM_MAX_ROWS whatever the selection; sliced
    assert plan_of(1, n1, ml.NMAX)["kernel"] == 1
    assert plan_of(1, ml.NMAX, n1)["kernel"] == (1 if match_kernel == "1" else 0)      # the reverse search
    print("path:", match_kernel, p)
    run_match(ah, torch, F, context)
    run_knn2(ah, torch, F, context, True)
    if n1 == 129:
        run_knn2(ah, torch, F, context, False)
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ chunks
@pytest.mark.parametrize("mode,context", [("unsliced", False), ("default", False), ("default", True), ("odd", False)],
                         indirect=["context"], ids=["unsliced", "default", "default, context", "odd"])
@pytest.mark.parametrize("n2", [ml.MM_MAX_ROWS, ml.MM_MAX_ROWS - 1])
def test_chunks(ah, torch, monkeypatch, match_kernel, n2, mode, context):
    """MM_MAX_ROWS rows (2047 whole chunks) and one fewer (2046 and a tail of 191 rows): one block walking them all, 512 slices by
    the default rule, and 98 slices, whose merge pads with `fill`"""
    a, b = seam_rows(monkeypatch, n2)
    F = family("chunks", n2, (a["rows_per_slice"], b["rows_per_slice"]))
    match_kernel_env = {"0": ("0", "1"), "qt2": ("0", "2"), "1": ("1", "1")}[match_kernel]
    monkeypatch.setenv("HAK_MATCH_VALU", match_kernel_env[0])       # (seam_rows asked the rule for the matrix-core kernel)
    monkeypatch.setenv("HAK_MATCH_QT", match_kernel_env[1])
    if mode != "default":
        monkeypatch.setenv("HAK_MATCH_SLICES", "1" if mode == "unsliced" else "100")
    n1 = len(F.queries)
    for search in (0, 1):
        p = plan_of(search, n1, n2)
        if match_kernel == "1":
            assert p["kernel"] == 1, p
            continue
        assert p["kernel"] == 0 and p["gx"] == 1, p
        if mode == "unsliced":
            assert p["slices"] == 1 and p["chunks_per_slice"] == 2047, p
        elif mode == "default":
            assert p["slices"] == (512 if match_kernel == "0" else 256), p
        else:
            assert p["slices"] == b["slices"] and p["slices"] % 8 and p["rows_per_slice"] == b["rows_per_slice"], p
    print("path:", match_kernel, mode, p)
    run_match(ah, torch, F, context)
    run_knn2(ah, torch, F, context, True)
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ switch
@pytest.mark.parametrize("n2", [ml.MM_MAX_ROWS, ml.MM_MAX_ROWS + 1, ml.NMAX])
def test_switch_to_the_vector_pipe(ah, torch, monkeypatch, n2):
    """the matrix-core kernel up to MM_MAX_ROWS rows, the vector-pipe kernels from the next row on -- and the same records either way"""
    F = family("index_bits", n2, 129)
    monkeypatch.setenv("HAK_MATCH_QT", "1")
    monkeypatch.delenv("HAK_MATCH_SLICES", raising=False)
    monkeypatch.setenv("HAK_MATCH_VALU", "0")
    for search in (0, 1):
        assert plan_of(search, 129, n2)["kernel"] == (0 if n2 == ml.MM_MAX_ROWS else 1), (search, n2)
    got = run_match(ah, torch, F, None)
    pts, lst = run_knn2(ah, torch, F, None, True)
    monkeypatch.setenv("HAK_MATCH_VALU", "1")
    assert plan_of(0, 129, n2)["kernel"] == 1
    assert run_match(ah, torch, F, None).tobytes() == got.tobytes()
    pts1, lst1 = run_knn2(ah, torch, F, None, True)
    assert pts1.tobytes() == pts.tobytes() and lst1.tobytes() == lst.tobytes()
    torch.cuda.empty_cache()


def test_more_than_the_key_holds_is_refused(ah, torch):
    """2^20 points on a side are refused with a message before a buffer is touched: real one-record buffers, the large count"""
    big = 1 << 20
    one = ml.index_bits(4096, 33).queries[:1].copy()
    one["match"] = 1234
    d1, d2 = upload(torch, one), upload(torch, one)
    d_out = torch.full((32,), 0x5A, dtype=torch.uint8, device="cuda")
    h_pts, h_out = one.copy(), np.full(1, 0x5A5A5A5A, np.int32).repeat(8).view(ah.MATCH_PAIR_DTYPE).copy()
    M = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    Fm = (C.c_float * 9)(0, 0, 0, 0, 0, -1, 0, 1, 0)
    cnt = C.c_int(-5)

    def untouched():
        assert download(ah, d1).tobytes() == one.tobytes() and download(ah, d2).tobytes() == one.tobytes()
        assert h_pts.tobytes() == one.tobytes() and (download(ah, d_out, np.uint8) == 0x5A).all()
        assert (h_out.view(np.int32) == 0x5A5A5A5A).all() and cnt.value == -5

    assert ah.lib.hak_match(None, d1.data_ptr(), 1, d2.data_ptr(), big, h_pts.ctypes.data) != 0
    assert "2^20 - 1 train points" in ah.lib.hak_last_error().decode()
    untouched()
    for n1, n2 in ((1, big), (big, 1)):
        assert ah.lib.hak_match_knn2(None, d1.data_ptr(), n1, d2.data_ptr(), n2, 4, 5, 1, 0, h_pts.ctypes.data, d_out.data_ptr(),
                                     C.byref(cnt), h_out.ctypes.data) != 0
        assert "2^20 - 1 points" in ah.lib.hak_last_error().decode()
        untouched()
        for fn, model in ((ah.lib.hak_match_guided, M), (ah.lib.hak_match_epipolar, Fm)):
            assert fn(None, d1.data_ptr(), n1, d2.data_ptr(), n2, model, 3.0, 4, 5, 1, 0, h_pts.ctypes.data, d_out.data_ptr(),
                      C.byref(cnt), h_out.ctypes.data) != 0
            assert "2^20 - 1 points" in ah.lib.hak_last_error().decode()
            untouched()
    # the batch entries on a context whose max_pts is 2^20 (full-size buffers: the capacity is the record stride)
    det = ah.Akazer()
    det.init((320, 240, 384), max_pts=big, batch=2)
    pts = torch.full((2 * big * 104,), 0x11, dtype=torch.uint8, device="cuda")
    num = torch.ones(2, dtype=torch.int32, device="cuda")
    out = torch.full((big * 32,), 0x22, dtype=torch.uint8, device="cuda")
    cnts = torch.full((1,), -5, dtype=torch.int32, device="cuda")
    model = torch.zeros(16, dtype=torch.float32, device="cuda")
    calls = [lambda: ah.lib.hak_match_batch(det.ctx, pts.data_ptr(), num.data_ptr(), 1),
             lambda: ah.lib.hak_match_knn2_batch(det.ctx, pts.data_ptr(), num.data_ptr(), 1, 4, 5, 1, 0, out.data_ptr(), cnts.data_ptr()),
             lambda: ah.lib.hak_match_guided_batch(det.ctx, pts.data_ptr(), num.data_ptr(), 1, model.data_ptr(), 3.0, 4, 5, 1, 0,
                                                   out.data_ptr(), cnts.data_ptr()),
             lambda: ah.lib.hak_match_epipolar_batch(det.ctx, pts.data_ptr(), num.data_ptr(), 1, model.data_ptr(), 3.0, 4, 5, 1, 0,
                                                     out.data_ptr(), cnts.data_ptr())]
    for call in calls:
        assert call() != 0
        assert "max_pts must stay below 2^20" in ah.lib.hak_last_error().decode()
    ah.check(ah.lib.hak_sync(det.ctx))
    assert bool((pts == 0x11).all()) and bool((out == 0x22).all()) and int(cnts[0]) == -5
    det.close()
    del pts, out
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ many_queries
@pytest.mark.parametrize("n2,context", [(64, False), (300, False), (300, True)], indirect=["context"], ids=["64", "300", "300, context"])
def test_many_queries(ah, torch, match_kernel, n2, context):
    """2^20 - 1 queries: the forward grid capped at 4096 looping blocks, the reverse search with the long train set (its records
    carry query indices with every high bit), 1024 finish blocks of k_knn2_finish_a / _b, whose list positions the list comparison
    holds for every accepted query: the first, the last and every 64th block, a block that accepts all 1024 and blocks with none"""
    F = family("many_queries", n2)
    for search in (0, 1):
        p = plan_of(search, ml.NMAX, n2)
        assert (p["kernel"], p["gx"], p["slices"], p["finish_blocks"]) == (1 if match_kernel == "1" else 0, 4096, 1, 1024), p
    r = plan_of(1, n2, ml.NMAX)
    assert r["kernel"] == 1 and r["finish_blocks"] == 1, r          # the reverse search: beyond MM_MAX_ROWS
    print("path:", match_kernel, p, "reverse", r)
    run_match(ah, torch, F, context)
    run_knn2(ah, torch, F, context, False)
    run_knn2(ah, torch, F, context, True)
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ the gated matchers
@pytest.mark.parametrize("long_queries,context", [(False, False), (True, False), (True, True)], indirect=["context"],
                         ids=["64 x 2^20-1", "2^20-1 x 64", "2^20-1 x 64, context"])
@pytest.mark.parametrize("matcher", ["guided", "epipolar"])
def test_gated(ah, torch, match_kernel, matcher, long_queries, context):
    """hak_match_guided / hak_match_epipolar on skinny pairs: forward keys whose two gated candidates differ in one index bit
    14 .. 19 (long train axis), reverse keys merged with atomicMin over queries that differ in those bits (long query axis, with 1024
    finish blocks), against the statements evaluated block-wise (ml.gated_blockwise), with and without the cross-check"""
    G = family("gated", int(long_queries))
    n1, n2 = len(G.pts1), len(G.pts2)
    p = plan_of(1, n1, n2)
    assert p["finish_blocks"] == (1024 if long_queries else 1), p
    print("path:", matcher, n1, n2, "finish blocks", p["finish_blocks"])
    M = ml.H_IDENTITY if matcher == "guided" else ml.F_ROWS
    call = ah.lib.hak_match_guided if matcher == "guided" else ah.lib.hak_match_epipolar
    for cross in (True, False):
        wout, wlst, _ = ml.gated_statement(matcher, long_queries, cross)
        d1, d2 = upload(torch, G.pts1), upload(torch, G.pts2)
        d_out = torch.full((n1 * 32,), 0xEE, dtype=torch.uint8, device="cuda")
        h_out = np.zeros(n1, ah.MATCH_PAIR_DTYPE)
        h_pts = G.pts1.copy()
        cnt = C.c_int(-1)
        ah.check(call(context, d1.data_ptr(), n1, d2.data_ptr(), n2, M.ctypes.data_as(C.POINTER(C.c_float)), ml.GATED_RADIUS,
                      ml.GATED_RATIO[0], ml.GATED_RATIO[1], int(cross), 0, h_pts.ctypes.data, d_out.data_ptr(), C.byref(cnt),
                      h_out.ctypes.data))
        what = f"{matcher} {n1} x {n2} cross={cross}"
        assert cnt.value == len(wlst), (what, cnt.value, len(wlst))
        assert_list(h_out[:cnt.value], wlst, what)
        assert_fields(h_pts, wout, what)
        lst = download(ah, d_out, ah.MATCH_PAIR_DTYPE)
        assert lst[:cnt.value].tobytes() == h_out[:cnt.value].tobytes(), "device list != host copy"
        assert (lst[cnt.value:].view(np.uint8) == 0xEE).all(), "written past the count"
        assert download(ah, d1).tobytes() == h_pts.tobytes(), "device records != host copy"
        assert download(ah, d2).tobytes() == G.pts2.tobytes(), "the train set was written"
        del d1, d2, d_out
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ batch leg
@pytest.mark.parametrize("mp", [ml.MM_MAX_ROWS, ml.MM_MAX_ROWS + 1])
def test_batch_capacity_at_the_switch(ah, torch, monkeypatch, mp):
    """device-side counts: a context whose max_pts is MM_MAX_ROWS takes the matrix-core kernel with 8 slices cut inside the kernel;
    one more point of capacity alone sends the same pair to the vector-pipe kernels.  Twice: the scratch is back in its initial state"""
    monkeypatch.setenv("HAK_MATCH_VALU", "0")
    monkeypatch.setenv("HAK_MATCH_QT", "1")
    a, b = seam_rows(monkeypatch, ml.MM_MAX_ROWS)
    F = family("chunks", ml.MM_MAX_ROWS, (a["rows_per_slice"], b["rows_per_slice"]))
    n1, n2 = len(F.queries), len(F.train)
    p = plan_of(0, 0, 0, 1, True, mp)
    assert (p["kernel"], p["slices"], p["rows_per_slice"]) == ((0, 8, 0) if mp == ml.MM_MAX_ROWS else (1, 1, 0)), p
    assert plan_of(1, 0, 0, 1, True, mp)["kernel"] == p["kernel"]
    print("path:", p)
    det = ah.Akazer()
    det.init((320, 240, 384), max_pts=mp, batch=2)
    host = np.zeros((2, mp), ah.POINT_DTYPE)
    host[0, :n1], host[1, :n2] = F.queries, F.train
    d_num = torch.from_numpy(np.array([n1, n2], np.int32)).cuda()
    d_out = torch.zeros(mp * 32, dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    want1 = F.expect_match()
    want2, wlst = F.expect_knn2(RATIO, True)
    for batch_knn in (False, True):
        d_pts = upload(torch, host)
        for _ in range(2):
            if batch_knn:
                ah.check(ah.lib.hak_match_knn2_batch(det.ctx, d_pts.data_ptr(), d_num.data_ptr(), 1, RATIO[0], RATIO[1], 1, 0,
                                                     d_out.data_ptr(), d_cnt.data_ptr()))
            else:
                ah.check(ah.lib.hak_match_batch(det.ctx, d_pts.data_ptr(), d_num.data_ptr(), 1))
            ah.check(ah.lib.hak_sync(det.ctx))
            got = download(ah, d_pts).reshape(2, mp)
            assert_fields(got[0, :n1], want2 if batch_knn else want1, f"batch knn={batch_knn}")
            assert got[1].tobytes() == host[1].tobytes(), "the train set was written"
            if batch_knn:
                assert int(d_cnt[0]) == len(wlst)
                assert_list(download(ah, d_out, ah.MATCH_PAIR_DTYPE)[:len(wlst)], wlst, "batch list")
        del d_pts
    det.close()
    torch.cuda.empty_cache()
