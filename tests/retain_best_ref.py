"""numpy statement of the strongest-N selection (hak_set_retain_best, include/hipakaze.h; cuda-akaze_amd/csrc/kernels_select.hip).

Input: the unclamped keypoint list of an image in raster order -- what a call with room for every NMS survivor returns, the
oracle's okz.detect_and_compute / okz.fast_detect_and_compute with a large max_pts -- and the image's clamp C.  Output: the
indices of the records a call with the mode on keeps, ascending (the records are emitted in raster order, each byte-identical
to its unclamped counterpart).

  S <= C: every index.
  S >  C: the C survivors ranking highest by (K(response word), then the smaller raster index).  The list is in raster order of
          the integer positions before refinement, so the list index IS the raster rank: ties go to the smaller index.
  K: float path (bits u of the response) u >> 31 ? ~u : u | 0x80000000; FAST path (int32 response, stored in the record as a
     float that holds the integer exactly) u ^ 0x80000000.  Unsigned order of K = the response's order.
"""
import numpy as np


def key_float(response):
    """K of float32 responses (any sign, -0.0 included) as uint32"""
    u = np.ascontiguousarray(response, np.float32).view(np.uint32)
    return np.where(u >> np.uint32(31) != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key_int(response):
    """K of int32 responses (the FAST path's integer response word) as uint32"""
    v = np.asarray(response)
    if v.dtype.kind == "f":                                        # a record's response field: float32 of the integer
        iv = v.astype(np.int64)
        assert np.array_equal(iv.astype(v.dtype), v), "FAST responses must be integers"
        v = iv
    u = v.astype(np.int64).astype(np.int32).view(np.uint32)
    return (u ^ np.uint32(0x80000000)).astype(np.uint32)


def retained(points_or_responses, C, fast=False):
    """indices (ascending) of the records an image keeps under clamp C; input: records (POINT_DTYPE) or their responses"""
    v = points_or_responses
    if getattr(v, "dtype", None) is not None and v.dtype.names and "response" in v.dtype.names:
        v = v["response"]
    v = np.asarray(v)
    S = len(v)
    assert C >= 1
    if S <= C:
        return np.arange(S)
    k = key_int(v) if fast else key_float(v)
    idx = np.arange(S)
    order = np.lexsort((idx, -k.astype(np.int64)))                # K descending, then index ascending
    return np.sort(order[:C])


def retain(points, C, fast=False):
    """the records themselves (a copy), in raster order"""
    return points[retained(points, C, fast)].copy()
