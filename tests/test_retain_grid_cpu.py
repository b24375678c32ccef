"""CPU suite: the grid selection (hak_set_retain_grid) -- its numpy statement tests/retain_grid_ref.py on hand cases and on random
inputs, the position recipe the GPU suite relies on (the oracle's own maps), and the entry points of every layer without a GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import retain_best_ref as rb
import retain_grid_ref as rg
from conftest import ROOT

f32 = np.float32


def raster(pts, w, dtype=f32):
    """(x, y, response) triples -> x, y, response arrays in raster order"""
    pts = sorted(pts, key=lambda p: p[1] * w + p[0])
    return np.array([p[0] for p in pts]), np.array([p[1] for p in pts]), np.array([p[2] for p in pts], dtype)


def test_no_overflow_keeps_everything():
    x, y, r = raster([(3, 1, 0.1), (40, 2, 0.5), (9, 30, 0.2)], 64)
    assert rg.retained(x, y, r, 64, 3, 16).tolist() == [0, 1, 2]
    assert rg.retained(x, y, r, 64, 10, 16).tolist() == [0, 1, 2]
    assert rg.retained(x[:0], y[:0], r[:0], 64, 4, 16).tolist() == []


def test_one_crowded_cell_and_three_sparse_ones():
    # w = 64, G = 32: cells 0 (crowded, 6 survivors), 1, 2, 3 (one each).  C = 6: q = 1 would keep 4, q = 2 keeps 5, q = 3 keeps 6,
    # q = 4 keeps 7 -> q = 3, R = 0: the sparse cells keep everything, the crowded one its three best
    x, y, r = raster([(1, 1, 0.6), (5, 1, 0.1), (9, 1, 0.5), (1, 5, 0.2), (5, 5, 0.4), (9, 5, 0.3), (40, 3, 0.01), (3, 40, 0.02),
                      (50, 50, 0.03)], 64)           # raster order: (1,1) (5,1) (9,1) (40,3) (1,5) (5,5) (9,5) (3,40) (50,50)
    assert rg.quota([6, 1, 1, 1], 6) == (3, 0)
    assert rg.retained(x, y, r, 64, 6, 32).tolist() == [0, 2, 3, 5, 7, 8]
    # strongest-N would have dropped the sparse cells
    assert rb.retained(r, 6).tolist() == [0, 1, 2, 4, 5, 6]


def test_remaining_places_ties_between_cells_go_to_the_smaller_raster_index():
    # four cells of two survivors each: C = 6 -> q = 1, R = 2; the rank-1 candidates of all four cells have the same response,
    # so the two with the smaller raster index win (cells 0 and 1)
    x, y, r = raster([(1, 1, 0.9), (2, 9, 0.5), (40, 1, 0.9), (41, 9, 0.5), (1, 40, 0.9), (2, 49, 0.5), (40, 40, 0.9), (41, 49, 0.5)], 64)
    assert list(zip(x, y))[2:4] == [(2, 9), (41, 9)] and (x[7], y[7]) == (41, 49)
    assert rg.quota([2, 2, 2, 2], 6) == (1, 2)
    assert rg.retained(x, y, r, 64, 6, 32).tolist() == [0, 1, 2, 3, 4, 5]
    # a stronger candidate in the last cell beats the tie
    r2 = r.copy()
    r2[7] = 0.6
    assert rg.retained(x, y, r2, 64, 6, 32).tolist() == [0, 1, 2, 4, 5, 7]


def test_exactly_no_place_remains():
    x, y, r = raster([(1, 1, 3), (5, 1, 2), (9, 1, 1), (40, 1, 1), (44, 1, 2), (48, 1, 3)], 64)
    assert rg.quota([3, 3], 4) == (2, 0)
    assert rg.retained(x, y, r, 64, 4, 32).tolist() == [0, 1, 4, 5]


def test_all_responses_equal():
    # 3 x 3 cells of four survivors each, C = 20: q = 2, R = 2 -- in every cell the first two in raster order, then the rank-2
    # candidates of the first two cells
    pos = [(cx * 16 + dx, cy * 16 + dy) for cy in range(3) for cx in range(3) for dx, dy in ((1, 1), (9, 1), (1, 9), (9, 9))]
    x, y, r = raster([(px, py, 0.25) for px, py in pos], 48)
    k = rg.retained(x, y, r, 48, 20, 16)
    kept = set(zip(x[k].tolist(), y[k].tolist()))
    want = {(cx * 16 + dx, cy * 16 + 1) for cy in range(3) for cx in range(3) for dx in (1, 9)} | {(1, 9), (17, 9)}
    assert kept == want


def test_negative_responses_and_negative_zero():
    x, y, r = raster([(1, 1, -0.0), (5, 1, -1.0), (9, 1, 0.0), (13, 1, -1e-30), (40, 1, -5.0)], 64)
    assert np.signbit(r[0]) and not np.signbit(r[2])
    # cell 0: 0.0 > -0.0 > -1e-30 > -1.0; C = 3: q = 1 keeps 2, q = 2 keeps 3 -> q = 2, R = 0
    assert rg.retained(x, y, r, 64, 3, 32).tolist() == [0, 2, 4]
    # C = 2: q = 1, R = 0
    assert rg.retained(x, y, r, 64, 2, 32).tolist() == [2, 4]
    # C = 4: q = 2 keeps 3, q = 3 keeps 4 -> q = 3
    assert rg.retained(x, y, r, 64, 4, 32).tolist() == [0, 2, 3, 4]


def test_fast_int_keys():
    x, y, v = raster([(1, 1, -7), (5, 1, 2000), (9, 1, 65), (40, 1, -2 ** 31), (44, 1, 2 ** 31 - 1)], 64, np.int64)
    assert rg.retained(x, y, v, 64, 2, 32, fast=True).tolist() == [1, 4]
    assert rg.retained(x, y, v, 64, 3, 32, fast=True).tolist() == [1, 2, 4]          # q = 1, R = 1: 65 (cell 0) beats -2^31
    # a FAST record holds the integer as float32
    assert rg.retained(x, y, np.array([-7, 2000, 65, -3, 9], f32), 64, 3, 32, fast=True).tolist() == [1, 2, 4]


def test_partial_last_column_and_row_of_cells():
    # w = 70, h = 50, G = 32: ncx = 3, the last column is 6 px wide, the last row 18 px tall; cell of (65, 40) = 1 * 3 + 2
    assert rg.cells([65, 63, 64, 0], [40, 31, 32, 49], 70, 32).tolist() == [5, 1, 5, 3]
    x, y, r = raster([(60, 1, 0.1), (62, 3, 0.2), (65, 1, 0.3), (68, 3, 0.4), (65, 40, 0.5), (68, 45, 0.6)], 70)
    # raster order: (60,1) (65,1) (62,3) (68,3) (65,40) (68,45)
    # cells 1: {(60,1), (62,3)}, 2: {(65,1), (68,3)}, 5: {(65,40), (68,45)}; C = 4: q = 1, R = 1 -> candidates 0.1, 0.2, 0.5
    assert rg.retained(x, y, r, 70, 4, 32).tolist() == [2, 3, 4, 5]


def test_clamp_below_the_number_of_occupied_cells():
    # five occupied cells, C = 2: q = 0, only candidates (the best of every cell) compete
    x, y, r = raster([(1, 1, 0.3), (5, 5, 0.9), (20, 1, 0.5), (36, 1, 0.7), (52, 1, 0.1), (1, 20, 0.8)], 64)
    # raster order: (1,1) (20,1) (36,1) (52,1) (5,5) (1,20)
    assert rg.quota([2, 1, 1, 1, 1], 2) == (0, 2)
    assert rg.retained(x, y, r, 64, 2, 16).tolist() == [4, 5]
    assert rg.retained(x, y, r, 64, 1, 16).tolist() == [4]


@pytest.mark.parametrize("seed", range(20))
def test_properties_on_random_inputs(seed):
    rng = np.random.default_rng(seed)
    w, h = int(rng.integers(40, 300)), int(rng.integers(40, 300))
    G = int(rng.choice([8, 13, 24, 32, 64, 128]))
    S = int(rng.integers(1, min(400, w * h // 4)))
    flat = np.sort(rng.choice(w * h, S, replace=False))
    x, y = flat % w, flat // w
    fast = bool(seed & 1)
    r = rng.choice(np.array([-3, 0, 65, 66, 900]), S) if fast else rng.choice(np.array([-1.0, -0.0, 0.0, 0.001, 0.5, 0.75], f32), S)
    C = int(rng.integers(1, S + 3))
    k = rg.retained(x, y, r, w, C, G, fast)
    assert len(k) == min(S, C) and np.all(np.diff(k) > 0)
    if S <= C:
        return
    cell = rg.cells(x, y, w, G)
    ids, counts = np.unique(cell, return_counts=True)
    q, R = rg.quota(counts, C)
    assert np.minimum(counts, q).sum() + R == C and 0 <= R < (counts > q).sum()
    key = rg.K(r, fast).astype(np.int64)
    plus = 0
    for c, n in zip(ids, counts):
        members = np.flatnonzero(cell == c)
        ranking = sorted(members.tolist(), key=lambda i: (-key[i], flat[i]))
        kept = [i for i in ranking if i in set(k.tolist())]
        assert len(kept) in (min(n, q), q + 1)
        assert kept == ranking[:len(kept)]                                    # a prefix of the cell's ranking
        plus += len(kept) == q + 1 and n > q
    assert plus == R


def test_position_recipe_lines_up_with_the_oracle_list(okz):
    """the integer positions come from the oracle's own maps (retain_grid_ref.oracle_positions): same list, float and FAST"""
    from akaze_hip import synth
    w, h = 320, 240
    u8 = synth.scene(w, h, 1, nshapes=120)
    p = 384
    r = okz.detect_and_compute(synth.to_float(u8, p), w, okz.default_params(), max_pts=1 << 16, keep_arena=True)
    x, y = rg.line_up(rg.oracle_positions(okz, r, w), r.points)
    assert len(x) > 100 and np.abs(r.points["x"] - x).max() <= 8.0 and np.any(r.points["x"] != x)
    rf = okz.fast_detect_and_compute(u8, max_pts=1 << 16, keep_arena=True)
    xf, yf = rg.line_up(rg.oracle_positions(okz, rf, w, fast=True), rf.points)
    assert len(xf) > 100


# ------------------------------------------------------------------------------------- entry points
def test_header_declares_and_library_exports_hak_set_retain_grid(ah):
    hdr = open(os.path.join(ROOT, "include", "hipakaze.h")).read()
    assert re.search(r"int\s+hak_set_retain_grid\s*\(\s*hak_ctx\s*\*\s*ctx\s*,\s*int\s+G\s*\)\s*;", hdr)
    assert "hak_set_retain_grid" in ah.SYMBOLS
    assert getattr(C.CDLL(ah.LIB_PATH), "hak_set_retain_grid") is not None
    for G in (32, 0, 7, 1000):                                                # a null context is refused first, no device needed
        assert ah.lib.hak_set_retain_grid(None, G) != 0
        assert b"null context" in ah.lib.hak_last_error()


def test_python_entry_points(ah):
    assert callable(getattr(ah.Akazer, "set_retain_grid", None))
    sig = inspect.signature(ah.Akazer.init)
    assert "retain_grid" in sig.parameters and sig.parameters["retain_grid"].default == 0
    det = ah.Akazer()                                                         # no context yet: the cell size is remembered
    det.set_retain_grid(32)
    assert det._retain_grid == 32
    det.set_retain_grid(0)
    assert det._retain_grid == 0
    for G in (7, 129, -1):                                                    # refused before any device is touched
        with pytest.raises(ValueError):
            det.set_retain_grid(G)
    assert det._retain_grid == 0


def test_cpp_entry_points():
    hdr = open(os.path.join(ROOT, "include", "akaze.h")).read()
    assert re.search(r"void\s+setRetainGrid\s*\(\s*int\s+G\s*\)\s*;", hdr)
    so = os.path.join(ROOT, "cuda-akaze_amd", "libakaze_hip.so")
    assert b"_ZN5akaze6Akazer13setRetainGridEi" in open(so, "rb").read()
    demo = os.path.join(ROOT, "cuda-akaze_amd", "hipakaze_demo")
    assert b"--retain-grid" in open(demo, "rb").read()
    stub = open(os.path.join(ROOT, "cuda-akaze_amd", "host", "asan", "stub_hipakaze.cpp")).read()
    assert "int hak_set_retain_grid(hak_ctx* c, int G)" in stub
