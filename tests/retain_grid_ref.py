"""numpy statement of the grid selection (hak_set_retain_grid, include/hipakaze.h; cuda-akaze_amd/csrc/kernels_grid_select.hip).

Input: the unclamped keypoint list of an image in raster order (what a call with room for every NMS survivor returns), the INTEGER
full-resolution position (x, y) of every entry before refinement, the image width w, the image's clamp C and the cell size G.
Output: the indices of the records a call with the mode on keeps, ascending (the records are emitted in raster order, each
byte-identical to its unclamped counterpart).

  S <= C: every index.
  S >  C: survivor i lies in cell (y_i // G) * ncx + x_i // G, ncx = ceil(w / G).  Inside a cell and between cells alike survivors
          rank by (K(response word) descending, then the smaller raster index y * w + x); K is retain_best_ref's.
          1. q = the largest integer >= 0 with sum_c min(n_c, q) <= C            (n_c: survivors of cell c)
          2. every cell keeps its min(n_c, q) highest-ranked survivors
          3. R = C - sum_c min(n_c, q) places remain
          4. the candidates: the rank-q survivor (0-based) of every cell with n_c > q
          5. the R highest-ranked candidates are kept as well

Records hold refined coordinates, from which the integer position cannot be recovered; oracle_positions() takes it from the
oracle's own full-resolution maps.
"""
import numpy as np

from retain_best_ref import key_float, key_int


def K(response, fast=False):
    return key_int(response) if fast else key_float(response)


def quota(counts, C):
    """(q, R) of the per-cell survivor counts under clamp C, by plain search"""
    counts = np.asarray(counts, np.int64)
    q = 0
    while np.minimum(counts, q + 1).sum() <= C:
        q += 1
        assert q <= counts.max(), "no overflow: there is no quota"
    return q, int(C - np.minimum(counts, q).sum())


def cells(x, y, w, G):
    x, y = np.asarray(x), np.asarray(y)
    assert np.array_equal(x, x.astype(np.int64)) and np.array_equal(y, y.astype(np.int64)), "integer positions"
    ncx = -(-w // G)
    return (y.astype(np.int64) // G) * ncx + x.astype(np.int64) // G


def retained(x, y, response, w, C, G, fast=False):
    """indices (ascending) into the unclamped raster-order list of the records an image keeps under clamp C and cell size G"""
    x, y, response = np.asarray(x), np.asarray(y), np.asarray(response)
    S = len(response)
    assert C >= 1 and 8 <= G <= 128 and len(x) == len(y) == S
    if S <= C:
        return np.arange(S)
    raster = np.asarray(y).astype(np.int64) * w + np.asarray(x).astype(np.int64)
    assert np.all(np.diff(raster) > 0), "the list must be in raster order of the integer positions"
    k = K(response, fast).astype(np.int64)
    cell = cells(x, y, w, G)
    ids, counts = np.unique(cell, return_counts=True)
    q, R = quota(counts, C)
    keep, cand = [], []
    for c in ids:
        members = np.flatnonzero(cell == c)
        ranked = members[np.lexsort((raster[members], -k[members]))]      # K descending, then raster index ascending
        keep.extend(ranked[:q])
        if len(ranked) > q:
            cand.append(ranked[q])
    cand = np.array(cand, np.int64)
    assert R < max(len(cand), 1) or (R == 0 and len(cand) == 0)
    if R:
        keep.extend(cand[np.lexsort((raster[cand], -k[cand]))][:R])
    out = np.sort(np.array(keep, np.int64))
    assert len(out) == C
    return out


def retain(points, x, y, w, C, G, fast=False):
    """the records themselves (a copy), in raster order; x, y: their integer positions before refinement"""
    return points[retained(x, y, points["response"], w, C, G, fast)].copy()


def oracle_positions(okz, result, w, psz=28, fast=False, big=1 << 19):
    """the unrefined survivors (integer x, y, raster order) of an oracle run made with keep_arena=True: the oracle's NMS on the
    full-resolution response, size and layer maps that sit at the head of the kept arena (osizes[0] words each, the layer map
    int32).  psz: min over octaves of borders[o][0] * 2^o, 28 at the default parameters.  The caller checks that the list lines up
    with the run's keypoint list (line_up)."""
    n = int(result.osizes[0])
    h = n // int(result.owhps[2])
    shape = (h, int(result.owhps[2]))
    a = result.arena
    resp = np.ascontiguousarray(a[:n]).reshape(shape)
    size = np.ascontiguousarray(a[n:2 * n]).view(np.float32).reshape(shape)
    layer = np.ascontiguousarray(a[2 * n:3 * n]).view(np.int32).reshape(shape)
    pts, total = okz.nms(resp, size, layer, w, psz, big, fast=fast)
    assert total == len(pts)
    return pts


def line_up(unrefined, full):
    """asserts that the unrefined survivor list is the unclamped keypoint list entry by entry; returns the integer (x, y)"""
    assert len(unrefined) == len(full), (len(unrefined), len(full))
    for f in ("response", "octave", "size"):
        assert np.array_equal(unrefined[f], full[f]), f
    x, y = unrefined["x"].astype(np.int64), unrefined["y"].astype(np.int64)
    assert np.array_equal(x, unrefined["x"]) and np.array_equal(y, unrefined["y"])
    return x, y
