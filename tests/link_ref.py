"""numpy statement of hak_link_tracks (include/hipakaze.h): joins the match list A of images (I0, I1), with a 3-D point per match,
and the match list B of images (I1, I2) on their shared image into 3-D to 2-D correspondences, byte for byte.

The checker only -- the product never calls it."""
import numpy as np

from pnp_ref import CORR3D_DTYPE

NONE = np.int64(0x7F7F7F7F)


def link_tracks(A, maskA, xyzA, B, max_index):
    """A, B: MATCH_PAIR structured arrays; maskA: nA bytes or None; xyzA: (nA, 3) float32 -> CORR3D array in ascending m"""
    nA = len(A)
    xyz = np.asarray(xyzA, np.float32).reshape(nA, 3)
    tab = np.full(max_index, NONE, np.int64)                           # train -> the smallest a
    train = A["train"].astype(np.int64)
    use = (train >= 0) & (train < max_index)
    if maskA is not None:
        use &= np.asarray(maskA).reshape(nA) != 0
    np.minimum.at(tab, train[use], np.arange(nA, dtype=np.int64)[use])
    q = B["query"].astype(np.int64)
    ok = (q >= 0) & (q < max_index)
    a = tab[np.where(ok, q, 0)]
    ok &= a != NONE
    m = np.nonzero(ok)[0]
    out = np.zeros(len(m), CORR3D_DTYPE)
    a = a[m]
    out["X"], out["Y"], out["Z"] = xyz[a, 0], xyz[a, 1], xyz[a, 2]
    out["u"], out["v"] = B["x2"][m], B["y2"][m]
    out["src3d"], out["src2d"] = a, m
    return out
