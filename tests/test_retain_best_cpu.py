"""CPU suite: the strongest-N selection (hak_set_retain_best) -- its numpy statement tests/retain_best_ref.py on hand cases, and the
entry points of every layer (C ABI, Python, C++ drop-in, demo) without a GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import retain_best_ref as rb
from conftest import ROOT

f32 = np.float32


def test_ties_across_the_threshold_go_to_the_smaller_raster_index():
    r = np.array([1, 3, 3, 2, 3, 1], f32)
    assert rb.retained(r, 2).tolist() == [1, 2]
    assert rb.retained(r, 3).tolist() == [1, 2, 4]
    assert rb.retained(r, 4).tolist() == [1, 2, 3, 4]
    assert rb.retained(r, 5).tolist() == [0, 1, 2, 3, 4]
    assert rb.retained(np.full(7, 0.25, f32), 3).tolist() == [0, 1, 2]       # all equal: the raster-order prefix


def test_single_survivor_and_no_overflow():
    assert rb.retained(np.array([5, 9, 9, 2], f32), 1).tolist() == [1]
    r = np.array([0.5, 0.1, 0.9], f32)
    assert rb.retained(r, 3).tolist() == [0, 1, 2]
    assert rb.retained(r, 10).tolist() == [0, 1, 2]
    assert rb.retained(np.zeros(0, f32), 4).tolist() == []


def test_float_key_orders_zero_negative_and_negative_zero():
    r = np.array([0.0, -0.0, -1.0, 1e-30, -1e-30], f32)
    k = rb.key_float(r)
    assert k[1] == 0x7FFFFFFF and k[0] == 0x80000000                     # -0.0 ranks just below +0.0
    assert k[2] < k[4] < k[1] < k[0] < k[3]
    assert rb.retained(r, 1).tolist() == [3]
    assert rb.retained(r, 2).tolist() == [0, 3]
    assert rb.retained(r, 3).tolist() == [0, 1, 3]
    assert rb.retained(r, 4).tolist() == [0, 1, 3, 4]


def test_int_key_is_signed_order():
    v = np.array([-5, 0, 7, -2 ** 31, 2 ** 31 - 1], np.int64)
    k = rb.key_int(v)
    assert k[3] == 0 and k[4] == 0xFFFFFFFF and k[0] < k[1] < k[2]
    assert rb.retained(v, 2, fast=True).tolist() == [2, 4]
    assert rb.retained(v, 4, fast=True).tolist() == [0, 1, 2, 4]
    # a FAST record holds the integer as float32: same key
    assert np.array_equal(rb.key_int(np.array([-5, 0, 7, 2020], f32)), rb.key_int(np.array([-5, 0, 7, 2020])))
    with pytest.raises(AssertionError):
        rb.key_int(np.array([1.5], f32))


def test_float_key_is_the_float_order():
    rng = np.random.default_rng(3)
    v = np.concatenate([rng.standard_normal(500) * 10.0 ** rng.integers(-30, 30, 500), [np.inf, -np.inf, 1e-45, -1e-45]]).astype(f32)
    v = v[v != 0]
    k = rb.key_float(v)
    assert np.array_equal(np.argsort(k, kind="stable"), np.argsort(v, kind="stable"))


@pytest.mark.parametrize("seed", range(20))
def test_statement_equals_a_plain_sort(seed):
    rng = np.random.default_rng(seed)
    S = int(rng.integers(1, 300))
    r = rng.choice(np.array([0.001, 0.002, 0.5, 0.75, 3.0, -2.0], f32), S)       # many ties
    C = int(rng.integers(1, S + 2))
    want = sorted(sorted(range(S), key=lambda i: (-float(r[i]), i))[:C])
    assert rb.retained(r, C).tolist() == want
    # records in, records out
    pts = np.zeros(S, [("x", "<f4"), ("response", "<f4")])
    pts["x"], pts["response"] = np.arange(S), r
    assert rb.retain(pts, C)["x"].tolist() == want


# ------------------------------------------------------------------------------------- entry points
def test_header_declares_and_library_exports_hak_set_retain_best(ah):
    hdr = open(os.path.join(ROOT, "include", "hipakaze.h")).read()
    assert re.search(r"int\s+hak_set_retain_best\s*\(\s*hak_ctx\s*\*\s*ctx\s*,\s*int\s+on\s*\)\s*;", hdr)
    assert "hak_set_retain_best" in ah.SYMBOLS
    f = getattr(C.CDLL(ah.LIB_PATH), "hak_set_retain_best")
    assert f is not None
    assert ah.lib.hak_set_retain_best(None, 1) != 0                          # a null context is refused, no device needed
    assert b"null context" in ah.lib.hak_last_error()


def test_python_entry_points(ah):
    assert callable(getattr(ah.Akazer, "set_retain_best", None))
    sig = inspect.signature(ah.Akazer.init)
    assert "retain_best" in sig.parameters and sig.parameters["retain_best"].default is False
    det = ah.Akazer()                                                         # no context yet: the flag is remembered
    det.set_retain_best(True)
    assert det._retain_best is True
    det.set_retain_best(False)
    assert det._retain_best is False


def test_cpp_entry_points():
    hdr = open(os.path.join(ROOT, "include", "akaze.h")).read()
    assert re.search(r"void\s+setRetainBest\s*\(\s*bool\s+on\s*\)\s*;", hdr)
    so = os.path.join(ROOT, "cuda-akaze_amd", "libakaze_hip.so")
    assert b"_ZN5akaze6Akazer13setRetainBestEb" in open(so, "rb").read()
    demo = os.path.join(ROOT, "cuda-akaze_amd", "hipakaze_demo")
    assert b"--retain-best" in open(demo, "rb").read()
    stub = open(os.path.join(ROOT, "cuda-akaze_amd", "host", "asan", "stub_hipakaze.cpp")).read()
    assert "int hak_set_retain_best(hak_ctx* c, int on)" in stub
