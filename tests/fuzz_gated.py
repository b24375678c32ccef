"""Randomised sentinel parity run of the two gated matchers: hak_match_guided / hak_match_guided_batch (kernels_guided.hip) and
hak_match_epipolar / hak_match_epipolar_batch (kernels_epipolar.hip) against their numpy statements (guided_match_ref.match_guided,
epipolar_match_ref.match_epipolar), bit for bit.

Test infrastructure.  `python tests/fuzz_gated.py --cases 3000 --seed 3` on the GPU box.

Why sentinels.  The kernels' results depend on the grid only through the conservative search window, and the output exposes only
j1, d1, d2 and rev(j1): a candidate the window skips changes nothing unless it is one of the two nearest, so random descriptors
would pass a window that drops points at the edge of a band.  Every eligible query i (in domain, with a model, whose band or disc
can be aimed at) therefore gets three train points of its own:
  A    query i's descriptor exactly (d = 0), B the same with one bit flipped (d = 1), each at an independent position along the
       line (epipolar) or direction in the disc (guided) at u * radius from the line / the projection, u from {0.5, 0.9, 0.999}
  out  a d = 0 copy at 1.001 * radius: only the exact gate may reject it
so that the statement's answer for i is (A, 0, 1) and losing A, B or admitting `out` changes a compared field.  Positions are
computed in float64 from the float32 (a, b, c) / (px, py) of the statement and rounded to float32; what is in or out is what the
statement says, never what the generator intended (tests/test_gated_fuzz_cpu.py measures both sides).  A share of the positions
is pushed onto the ends of the train cloud's box and onto multiples of the cell side the bin kernel will choose
(max(r', extent / 64): computed here only to aim points -- the result never depends on it).  Sentinels are train points and
would move that box, so it is fixed first: two fill points sit on the corners of a box that holds every sentinel to come, and the
grid aimed at is the grid of the finished train set (asserted case by case in tests/test_gated_fuzz_cpu.py).  For the same reason
a one-cell grid (tiny) and projections that all land in border cells (H far) cannot hold sentinels: 40 % of those cases run `plain`,
without sentinels, in their stated grid shape.

Regimes, each axis drawn independently (draw_case): set sizes, the train and the query cloud (image, offset to +-16000, thin, tiny,
clustered, stretched by far / non-finite points, integer lattice), radius, ratio, cross-check, max_dist, context or none; F from
two-view geometry with the epipole inside / near / far / at infinity, affine F at the listed angles, F scaled by 2^k (den on both
sides of 2^-100, r2 den up to inf), lines that miss everything; H identity / mild / strong (wz changes sign inside the query
cloud), scaled by 2^k, projecting far outside the train box and beyond 2^20.  Blocks of eight consecutive indices may hold a group
of 2-6 cases that share matcher, radius, ratio, cross-check and max_dist and ALSO go through the batch entry point as one ragged
call, with one broken record (hypothesis = -1 or a NaN entry) and NaN records past the counts.

Measured on an MI355X box (profiles/fuzz_gated.txt): 3 000 cases and their 168 batch groups in 47 s, 16 ms per case, nearly all of
it the numpy statement and the generator."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("cuda-akaze_amd", "tests", ""):
    p = os.path.join(ROOT, sub)
    if p not in sys.path:
        sys.path.insert(0, p)

import epipolar_match_ref as er  # noqa: E402
import guided_match_ref as gr  # noqa: E402

FIELDS = ("match", "distance", "match_x", "match_y")
L = 16384.0
BUDGET = 1_000_000                   # n1 * n2 of a case: the dense statement stays fast
MAX_PTS = 3200                       # capacity of the batch leg's context: n1 <= 1500, n2 <= 1500 fill + 3 n1 within the budget
TRAIN_KINDS = ("image", "offset", "thin", "tiny", "clustered", "stretched", "lattice")
QUERY_KINDS = ("image", "image", "offset", "thin", "clustered", "stretched")
F_KINDS = ("epi_inside", "epi_near", "epi_far", "epi_inf", "affine")
H_KINDS = ("identity", "mild", "strong", "far", "beyond")
ANGLES = ("0", "90", "45", "45+", "45-", "1e-6", "90-1e-6", "1e-3", "90-1e-3")
SCALES = ("none", "none", "moderate", "floor", "big", "big")
U = (0.5, 0.9, 0.999)
RADII = (1e-3, 300.0, 1e4)
LATTICE_AB = ((0, 1), (1, 0), (3, 4), (4, 3), (1, 1), (5, 12), (-4, 3))
LATTICE_R = (1.0, 2.0, 5.0, 13.0)


def _pick(rng, seq):
    return seq[int(rng.integers(len(seq)))]


def draw_group(seed, block):
    """the batch group of the eight indices 8 block .. 8 block + 7, or None: a pure function of (seed, block)"""
    rng = np.random.default_rng([seed, block, 78])
    if rng.random() >= 0.5:
        return None
    size = int(rng.integers(2, 7))
    start = 8 * block + int(rng.integers(0, 8 - size + 1))
    return dict(start=start, size=size, matcher=_pick(rng, ("guided", "epipolar")), radius=_draw_radius(rng),
                ratio=_pick(rng, ((1, 1), (4, 5), (1000, 1))), cross=int(rng.integers(2)), max_dist=_pick(rng, (0, 40, 512)),
                bad=start + int(rng.integers(size)), bad_kind=_pick(rng, ("hypothesis", "nan")))


def _draw_radius(rng):
    if rng.random() < 0.15:
        return float(_pick(rng, RADII))
    return float(np.float32(np.exp(rng.uniform(np.log(0.01), np.log(64.0)))))


def _draw_size(rng, lo):
    kind = _pick(rng, ("small", "medium", "large"))
    n = int({"small": rng.integers(lo, 65), "medium": rng.integers(64, 601), "large": rng.integers(600, 1501)}[kind])
    if rng.random() < 0.33:
        n = max(lo, _pick(rng, (64, 256, 1024)) + _pick(rng, (-1, 0, 1)))
    return n


def draw_case(seed, index):
    """the parameters of case `index`: a pure function of (seed, index)"""
    rng = np.random.default_rng([seed, index, 77])
    c = dict(index=index, matcher=_pick(rng, ("guided", "epipolar")), n1=_draw_size(rng, 1), n2=_draw_size(rng, 0),
             train=_pick(rng, TRAIN_KINDS), query=_pick(rng, QUERY_KINDS), radius=_draw_radius(rng),
             ratio=_pick(rng, ((1, 1), (4, 5), (1000, 1))), cross=int(rng.integers(2)), max_dist=_pick(rng, (0, 40, 512)),
             ctx=bool(rng.random() < 0.5), fkind=_pick(rng, F_KINDS + ("affine", "affine")), hkind=_pick(rng, H_KINDS), angle=_pick(rng, ANGLES),
             scale=_pick(rng, SCALES), cmiss=bool(rng.random() < 0.05), exact_epipole=bool(rng.random() < 0.5),
             dup=_pick(rng, (0.0, 0.0, 0.2, 0.5)), special=bool(rng.random() < 0.4), seed=int(rng.integers(1 << 30)),
             group=None, bad=None, empty=False, plain=False)
    keep = bool(rng.random() < 0.4)
    if rng.random() < 0.04:                                             # an empty train set: no sentinels either
        c["n2"], c["empty"] = 0, True
    if rng.random() < 0.04:
        c["n1"] = 1
    g = draw_group(seed, index // 8)
    if g is not None and g["start"] <= index < g["start"] + g["size"]:
        for k in ("matcher", "radius", "ratio", "cross", "max_dist"):
            c[k] = g[k]
        c["group"] = (g["start"], g["size"])
        c["bad"] = g["bad_kind"] if g["bad"] == index else None
    if c["train"] == "lattice":                                         # integer coordinates, integer-valued model and radius
        if c["group"] is None:                                          # (a group's radius is the group's)
            c["radius"] = float(LATTICE_R[c["seed"] % len(LATTICE_R)])
        c["query"], c["scale"], c["cmiss"] = "lattice", "none", False
    if c["train"] == "tiny" and c["matcher"] == "epipolar":             # lines of far-apart queries would all miss a tiny cloud
        c["query"] = "tiny"
    # sentinels are train points: they stretch the bin kernel's box.  A one-cell grid (tiny) and projections that all land in border
    # cells (H far) cannot hold with them, so a share of those cases runs plain, without sentinels, and keeps its grid shape
    c["plain"] = keep and (c["train"] == "tiny" or (c["matcher"] == "guided" and c["hkind"] == "far" and c["train"] != "lattice"))
    c["regime"] = "lattice" if c["train"] == "lattice" else c["fkind"] if c["matcher"] == "epipolar" else c["hkind"]
    return c


# ---------------------------------------------------------------------------------------------------------- clouds and models
def _frame(rng, kind, radius):
    """(cx, cy, w, h) of a cloud"""
    w, h = rng.uniform(640, 1920), rng.uniform(480, 1080)
    cx, cy = w / 2, h / 2
    if kind == "offset":
        cx, cy = rng.uniform(-16000, 16000), rng.uniform(-16000, 16000)
        if rng.random() < 0.5:                                           # across the bound of the domain on one axis
            if rng.random() < 0.5:
                cx = _pick(rng, (-1.0, 1.0)) * rng.uniform(15800, 16384)
            else:
                cy = _pick(rng, (-1.0, 1.0)) * rng.uniform(15800, 16384)
    elif kind == "thin":
        if rng.random() < 0.5:
            w = _pick(rng, (0.0, rng.uniform(0, 1)))
        else:
            h = _pick(rng, (0.0, rng.uniform(0, 1)))
    elif kind == "tiny":
        w = h = radius * rng.uniform(0.0, 0.5)
    elif kind == "lattice":
        w, h = 48.0, 36.0
        cx, cy = 24.0 + int(rng.integers(0, 200)), 18.0 + int(rng.integers(0, 200))
    return float(cx), float(cy), float(w), float(h)


def _cloud(rng, kind, n, fr):
    cx, cy, w, h = fr
    x = rng.uniform(cx - w / 2, cx + w / 2, n)
    y = rng.uniform(cy - h / 2, cy + h / 2, n)
    if kind == "lattice":
        x, y = np.floor(x), np.floor(y)
    if kind == "clustered" and n:
        k = rng.random(n) < 0.8
        bx, by = rng.uniform(cx - w / 2, cx + w / 2), rng.uniform(cy - h / 2, cy + h / 2)
        x[k], y[k] = bx + rng.uniform(-10, 10, int(k.sum())), by + rng.uniform(-10, 10, int(k.sum()))
    x, y = x.astype(np.float32), y.astype(np.float32)
    if kind == "stretched" and n:
        far = (2.0 ** rng.uniform(15, 20), -2.0 ** rng.uniform(15, 20), 2.0 ** 20, 2.0 ** 20 + 1, 2.0 ** rng.uniform(20, 60), 1e30, np.inf,
               -np.inf, np.nan)
        for _ in range(int(rng.integers(1, 4))):
            j = int(rng.integers(n))
            if rng.random() < 0.5:
                x[j] = _pick(rng, far)
            else:
                y[j] = _pick(rng, far)
    return x, y


def _specials(rng, x, y):
    """a share of queries at the bound of the domain, just beyond it, or non-finite"""
    e = np.float32(L)
    vals = (e, -e, np.nextafter(e, np.float32(np.inf)), -np.nextafter(e, np.float32(np.inf)), np.nextafter(e, np.float32(0)),
            np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf))
    for i in np.nonzero(rng.random(len(x)) < 0.05)[0]:
        if rng.random() < 0.5:
            x[i] = _pick(rng, vals)
        else:
            y[i] = _pick(rng, vals)


def _rot(rng, deg):
    ax, ay, az = np.deg2rad(rng.uniform(-deg, deg, 3))
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def _cross(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def affine_ab(angle):
    """float32 (a, b) of the parallel lines at a listed angle (the lines run along (cos, sin): their normal is (-sin, cos))"""
    one = np.float32(1.0)
    s45 = np.float32(np.sqrt(0.5))
    up, dn = np.nextafter(s45, one), np.nextafter(s45, np.float32(0))
    tab = {"0": (0.0, 1.0), "90": (1.0, 0.0), "45": (-s45, s45), "45+": (-np.nextafter(up, one), dn), "45-": (-dn, np.nextafter(up, one))}
    if angle in tab:
        a, b = tab[angle]
    else:
        th = float(angle.split("-", 1)[1]) if angle.startswith("90-") else float(angle)
        a, b = (-np.sin(th), np.cos(th)) if not angle.startswith("90-") else (-np.cos(th), np.sin(th))
    return np.float32(a), np.float32(b)


def _make_F(rng, c, qf, tf, info):
    """row-major float32 F[9]: the line of a query runs through the train cloud where the regime allows it"""
    qc, tc = np.array(qf[:2]), np.array(tf[:2])
    d = tc - qc
    if c["train"] == "lattice":
        a, b = LATTICE_AB[c["seed"] % len(LATTICE_AB)]
        dx, dy = np.round(d)
        F = np.array([0, 0, a, 0, 0, b, -a, -b, -(a * dx + b * dy) + int(rng.integers(-3, 4))], np.float64)
    elif c["fkind"] == "affine":
        a, b = (float(v) for v in affine_ab(c["angle"]))
        F = np.array([0, 0, a, 0, 0, b, -a, -b, -(a * d[0] + b * d[1])], np.float64)
    elif c["fkind"] == "epi_inside" and c["exact_epipole"]:
        e1 = np.round(qc + rng.uniform(-0.4, 0.4, 2) * np.array(qf[2:]))
        di = np.round(d)
        e2 = e1 + di
        F = np.array([0, -1, e1[1], 1, 0, -e1[0], -e2[1], e2[0], e2[0] * di[1] - e2[1] * di[0]], np.float64)
        info["epipole"] = e1
    else:
        f = rng.uniform(500, 3000)
        K1 = np.array([[f, 0, qc[0]], [0, f, qc[1]], [0, 0, 1.0]])
        K2 = np.array([[f, 0, tc[0]], [0, f, tc[1]], [0, 0, 1.0]])
        ext = max(qf[2], qf[3], 1.0)
        if c["fkind"] == "epi_inf":
            R = np.eye(3)
            ph = rng.uniform(0, 2 * np.pi)
            Cc = np.array([np.cos(ph), np.sin(ph), 0.0])
        else:
            R = _rot(rng, 4.0)
            ph = rng.uniform(0, 2 * np.pi)
            dist = {"epi_inside": rng.uniform(0, 0.4), "epi_near": rng.uniform(0.7, 3.0), "epi_far": rng.uniform(20, 200)}[c["fkind"]] * ext
            ep = qc + dist * np.array([np.cos(ph), np.sin(ph)])
            if c["fkind"] == "epi_inside":
                ep = np.clip(ep, qc - np.array(qf[2:]) / 2, qc + np.array(qf[2:]) / 2).astype(np.float32).astype(np.float64)
                info["epipole"] = ep
            Cc = np.linalg.solve(K1, np.array([ep[0], ep[1], 1.0]))
        t = -R @ Cc
        F = (np.linalg.inv(K2).T @ _cross(t) @ R @ np.linalg.inv(K1)).reshape(9)
        F = F / np.abs(F).max()
    F = F.astype(np.float32)
    if c["cmiss"]:                                                       # |c| so large that every line misses the box by more than 2^40
        s = max(float(np.abs(F[[0, 1, 2, 3, 4, 5]]).max()), 1e-6) * max(1.0, float(np.abs(qc).max()) + 2000)
        F[8] = np.float32(s * 2.0 ** 46)
    return F


def _scale_pow(rng, c, M, q):
    """the exponent k of the 2^k the model is scaled by"""
    if c["scale"] == "none":
        return 0
    if c["matcher"] == "guided":
        return int(rng.integers(-60, 61)) if c["scale"] != "moderate" else int(rng.integers(-12, 13))
    if c["scale"] == "moderate":
        return int(rng.integers(-30, 31))
    den = er.line(q, M)[3]
    den = den[np.isfinite(den) & (den > 0)]
    lg = float(np.log2(np.median(den))) if len(den) else 0.0
    if c["scale"] == "floor":                                            # den on both sides of 2^-100
        return int(round((-100.0 - lg) / 2)) + int(rng.integers(-1, 2))
    r2 = float(np.float32(c["radius"]) * np.float32(c["radius"]))
    top = min((127.5 - lg) / 2, 126.0 - float(np.log2(max(np.abs(M).max(), 1e-30))))
    if r2 > 1.0 and rng.random() < 0.8:                                  # r2 den around 2^128: inf for a share of the queries
        return int(np.floor(min(top, (128.0 - lg - np.log2(max(r2, 1e-30))) / 2 + rng.uniform(-1, 1))))
    return int(np.floor(top - rng.uniform(0, 3)))                        # just below overflow of den


def _make_H(rng, c, qf, tf, info):
    qc, tc = np.array(qf[:2]), np.array(tf[:2])
    d = tc - qc
    if c["hkind"] == "far":
        d = d + _pick(rng, (-1.0, 1.0)) * np.array([rng.uniform(3e4, 5e5), rng.uniform(0, 5e5)])
    elif c["hkind"] == "beyond":
        d = d + _pick(rng, (-1.0, 1.0)) * np.array([2.0 ** rng.uniform(20, 23), rng.uniform(0, 2.0 ** 21)])[:: _pick(rng, (1, -1))]
    if c["train"] == "lattice":
        dx, dy = np.round(d)
        return np.array([1, 0, dx, 0, 1, dy, 0, 0, 1], np.float32)
    Tq = np.array([[1, 0, -qc[0]], [0, 1, -qc[1]], [0, 0, 1.0]])
    Tt = np.array([[1, 0, qc[0] + d[0]], [0, 1, qc[1] + d[1]], [0, 0, 1.0]])
    P = np.eye(3)
    if c["hkind"] != "identity":
        P[:2, :2] += rng.uniform(-0.05, 0.05, (2, 2))
        P[:2, 2] = rng.uniform(-5, 5, 2)
        P[2, :2] = rng.uniform(-1e-4, 1e-4, 2)
    if c["hkind"] == "strong":                                           # wz = 1 + g . (x - qc) is zero on a line through the query cloud
        ph = rng.uniform(0, 2 * np.pi)
        dist = rng.uniform(0.05, 0.3) * max(min(qf[2], qf[3]), 1.0)
        P[2, :2] = -np.array([np.cos(ph), np.sin(ph)]) / dist
    H = (Tt @ P @ Tq).reshape(9)
    return (H / (np.abs(H[8]) if H[8] != 0 else 1.0)).astype(np.float32)


def cell_side(matcher, radius, tx, ty):
    """the cell side and origin k_guided_bin will choose for these train points (used only to aim sentinels)"""
    rp = float(np.float32(radius * 1.0001 + 0.01)) if matcher == "epipolar" else float(np.float32(radius) * np.float32(1.0001))
    ok = (np.abs(tx) <= 2.0 ** 20) & (np.abs(ty) <= 2.0 ** 20)
    if not ok.any():
        return rp, 0.0, 0.0
    ex, ey = float(tx[ok].max()) - float(tx[ok].min()), float(ty[ok].max()) - float(ty[ok].min())
    return max(rp, max(ex, ey) / 64.0), float(tx[ok].min()), float(ty[ok].min())


def grid_shape(matcher, radius, tx, ty):
    """(nx, ny) of the grid k_guided_bin will build: floor(extent / side) + 1 cells per axis, at most 64"""
    side = cell_side(matcher, radius, tx, ty)[0]
    ok = (np.abs(tx) <= 2.0 ** 20) & (np.abs(ty) <= 2.0 ** 20)
    if not ok.any():
        return 1, 1
    ex, ey = float(tx[ok].max()) - float(tx[ok].min()), float(ty[ok].max()) - float(ty[ok].min())
    return int(min(np.floor(ex / side) + 1, 64)), int(min(np.floor(ey / side) + 1, 64))


def _clip_line(a, b, cc, box):
    """parameter range of the line a x + b y + cc = 0 inside box = (x0, x1, y0, y1): (point, direction, t0, t1) or None"""
    s2 = a * a + b * b
    p0 = np.array([-a * cc / s2, -b * cc / s2])
    dv = np.array([-b, a]) / np.sqrt(s2)
    t0, t1 = -np.inf, np.inf
    for k, (lo, hi) in enumerate(((box[0], box[1]), (box[2], box[3]))):
        if abs(dv[k]) < 1e-300:
            if not lo <= p0[k] <= hi:
                return None
            continue
        ta, tb = (lo - p0[k]) / dv[k], (hi - p0[k]) / dv[k]
        t0, t1 = max(t0, min(ta, tb)), min(t1, max(ta, tb))
    if not (np.isfinite(t0) and np.isfinite(t1)) or t0 > t1:
        return None
    return p0, dv, t0, t1


def make_case(c, dtype=None):
    """the point sets, the model and the sentinel book-keeping of a drawn case:
    dict(q, t, M, radius, sent = (ns, 4) int array of {query, A, B, out} indices, one row per eligible query in the order of
    `eligible`, uA, uB, watch, grid = the (side, ox, oy) the sentinels were aimed at, grid_real = the same of the finished train set,
    flags)"""
    from akaze_hip import synth
    if dtype is None:
        import akaze_hip
        dtype = akaze_hip.POINT_DTYPE
    rng = np.random.default_rng(c["seed"])
    radius, matcher = c["radius"], c["matcher"]
    n1, nfill = c["n1"], c["n2"]
    if n1 * nfill > 0.5 * BUDGET:
        nfill = int(0.5 * BUDGET / n1)
    tf = _frame(rng, c["train"], radius)
    qf = _frame(rng, c["query"], radius)
    tx, ty = _cloud(rng, c["train"], nfill, tf)
    qx, qy = _cloud(rng, c["query"], n1, qf)
    if c["special"]:
        _specials(rng, qx, qy)
    q = synth.random_descriptors(n1, (c["seed"] + 1) % 100003, dtype)
    q["x"], q["y"] = qx, qy
    info = {}
    M = _make_F(rng, c, qf, tf, info) if matcher == "epipolar" else _make_H(rng, c, qf, tf, info)
    if "epipole" in info and n1 >= 2:                                    # one query AT the epipole, one a float32 step away
        q["x"][0], q["y"][0] = info["epipole"]
        q["x"][1], q["y"][1] = np.nextafter(np.float32(info["epipole"][0]), np.float32(np.inf)), info["epipole"][1]
    k = _scale_pow(rng, c, M, q)
    M = (M.astype(np.float64) * 2.0 ** k).astype(np.float32)
    M = np.where(np.isfinite(M), M, np.float32(0)).astype(np.float32)
    dom = (np.abs(tx) <= L) & (np.abs(ty) <= L)
    if dom.any():
        box = [float(tx[dom].min()), float(tx[dom].max()), float(ty[dom].min()), float(ty[dom].max())]
    else:
        box = [tf[0] - tf[2] / 2, tf[0] + tf[2] / 2, tf[1] - tf[3] / 2, tf[1] + tf[3] / 2]
    pad = min(radius, 64.0)
    box = [max(box[0] - pad, -L), min(box[1] + pad, L), max(box[2] - pad, -L), min(box[3] + pad, L)]

    # ---- eligible queries and their sentinel positions (float64 from the statement's float32 words)
    room = max(0, int((BUDGET / n1 - nfill - 2) // 3))                   # how many queries can have their three points
    sx, sy, uA, uB = [], [], [], []
    with np.errstate(all="ignore"):
        if matcher == "epipolar":
            a, b, cc, den = er.line(q, M)
            okq = (np.abs(q["x"]) <= L) & (np.abs(q["y"]) <= L) & (den >= er.DEN_MIN) & np.isfinite(den) & np.isfinite(cc)
        else:
            px, py, wz = gr.project(q, M)
            okq = (wz > 0) & np.isfinite(px) & np.isfinite(py) & (np.abs(px) < 2.0 ** 40) & (np.abs(py) < 2.0 ** 40)
    # ---- the grid is fixed BEFORE aiming: two fill points on the corners of a box that holds every sentinel to come (the padded box
    # plus 1.001 radius for the epipolar lines, the projections plus 1.001 radius for the discs, within the 2^20 the bin kernel's box
    # admits), so that cell_side() here is what k_guided_bin will choose for the finished train set
    sentinels = not c["empty"] and not c["plain"] and room > 0 and bool(okq.any())
    if sentinels:
        B20 = 2.0 ** 20
        fin = (np.abs(tx) <= B20) & (np.abs(ty) <= B20)
        g = [np.inf, -np.inf, np.inf, -np.inf]
        if fin.any():
            g = [float(tx[fin].min()), float(tx[fin].max()), float(ty[fin].min()), float(ty[fin].max())]
        reach = 1.002 * radius
        if matcher == "epipolar":
            g = [min(g[0], box[0] - reach), max(g[1], box[1] + reach), min(g[2], box[2] - reach), max(g[3], box[3] + reach)]
        else:
            near = okq & (np.abs(px) <= B20 + 2 * radius) & (np.abs(py) <= B20 + 2 * radius)
            if near.any():
                g = [min(g[0], float(px[near].min()) - reach), max(g[1], float(px[near].max()) + reach),
                     min(g[2], float(py[near].min()) - reach), max(g[3], float(py[near].max()) + reach)]
        if np.isfinite(g).all():
            lo = np.clip(np.array([g[0], g[2]]), -B20, B20)
            hi = np.clip(np.array([g[1], g[3]]), -B20, B20)
            if c["train"] == "lattice":
                lo, hi = np.floor(lo) - 1, np.ceil(hi) + 1
            lo32, hi32 = lo.astype(np.float32), hi.astype(np.float32)
            for _ in range(4):                                            # outward by a few float32 steps: past any rounded sentinel
                lo32 = np.maximum(np.nextafter(lo32, np.float32(-np.inf)), np.float32(-B20))
                hi32 = np.minimum(np.nextafter(hi32, np.float32(np.inf)), np.float32(B20))
            tx, ty = np.append(tx, [lo32[0], hi32[0]]).astype(np.float32), np.append(ty, [lo32[1], hi32[1]]).astype(np.float32)
            nfill += 2
    side, ox, oy = cell_side(matcher, radius, tx, ty)
    eligible = []
    dead = (np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf)) + \
        ((np.nextafter(np.float32(L), np.float32(np.inf)), np.float32(-1e30)) if matcher == "epipolar" else ())
    for i in rng.permutation(np.nonzero(okq)[0] if sentinels else []):
        us = [_pick(rng, U), _pick(rng, U), 1.001]
        pos = []
        if matcher == "epipolar":
            ai, bi, ci = float(a[i]), float(b[i]), float(cc[i])
            # (a, b, c) / s computed on scaled words: the squares of float32 values near 2^+-64 leave float64's range otherwise
            e2 = np.frexp(max(abs(ai), abs(bi)))[1]
            an, bn, cn = np.ldexp(ai, -e2), np.ldexp(bi, -e2), np.ldexp(ci, -e2)
            seg = _clip_line(an, bn, cn, box)
            if seg is None:
                continue
            p0, dv, t0, t1 = seg
            nrm = np.array([an, bn]) / np.hypot(an, bn)
            for u in us:
                r = rng.random()
                t = rng.uniform(t0, t1)
                off = nrm * (u * radius * _pick(rng, (-1.0, 1.0)))
                if r < 0.15:
                    t = _pick(rng, (t0, t1))                              # an end of the box
                elif r < 0.45:                                            # the sentinel itself onto a cell boundary, on either axis
                    ax = int(rng.integers(2))
                    if abs(dv[ax]) > 1e-9:
                        o = (ox, oy)[ax]
                        kk = np.round(((p0 + t * dv + off)[ax] - o) / side)
                        tb = (o + kk * side - p0[ax] - off[ax]) / dv[ax]
                        if t0 <= tb <= t1:
                            t = tb
                pt = p0 + t * dv + off
                if np.abs(pt).max() > L:                                  # the other side of the line, if that one is in the domain
                    pt = p0 + t * dv - off
                pos.append(pt)
        else:
            pxi, pyi = float(px[i]), float(py[i])
            for u in us:
                ph = rng.uniform(0, 2 * np.pi)
                pt = np.array([pxi + u * radius * np.cos(ph), pyi + u * radius * np.sin(ph)])
                if rng.random() < 0.4:                                    # onto a cell boundary in x or y, keeping the distance
                    ax = int(rng.integers(2))
                    ctr, o = np.array([pxi, pyi]), (ox, oy)[ax]
                    xb = o + np.round((ctr[ax] - o) / side) * side
                    if abs(xb - ctr[ax]) < 0.95 * u * radius:
                        pt = ctr.copy()
                        pt[ax] = xb
                        pt[1 - ax] += _pick(rng, (-1.0, 1.0)) * np.sqrt((u * radius) ** 2 - (xb - ctr[ax]) ** 2)
                pos.append(pt)
        if len(eligible) >= room:                                           # no room for its three points within the budget: the query
            q["x" if rng.random() < 0.5 else "y"][i] = _pick(rng, dead)   # leaves the domain instead of going unwatched
            continue
        eligible.append(int(i))
        uA.append(us[0])
        uB.append(us[1])
        for pt in pos:
            sx.append(pt[0])
            sy.append(pt[1])

    # ---- the train set: fill (random descriptors, a share of exact duplicates), then A, B, out of every served query
    ns = len(eligible)
    t = synth.random_descriptors(max(nfill + 3 * ns, 1), c["seed"] % 100003, dtype)[:nfill + 3 * ns]
    t["x"][:nfill], t["y"][:nfill] = tx, ty
    if nfill > 4 and c["dup"] > 0:
        kd = int(nfill * c["dup"])
        t["features"][rng.choice(nfill, kd, replace=False)] = t["features"][rng.integers(0, nfill, kd)]
    sent = np.zeros((ns, 4), np.int64)
    if ns:
        place = nfill + rng.permutation(ns)                              # A at a random slot of the first block: the smallest index
        sent[:, 0] = eligible
        sent[:, 1], sent[:, 2], sent[:, 3] = place, nfill + ns + rng.permutation(ns), nfill + 2 * ns + rng.permutation(ns)
        with np.errstate(all="ignore"):
            for kk in range(3):
                t["x"][sent[:, 1 + kk]] = np.array(sx[kk::3]).astype(np.float32)
                t["y"][sent[:, 1 + kk]] = np.array(sy[kk::3]).astype(np.float32)
        feats = q["features"][sent[:, 0]]
        t["features"][sent[:, 1]] = feats
        t["features"][sent[:, 3]] = feats
        flip = feats.copy()
        bit = rng.integers(0, 486, ns)
        flip[np.arange(ns), bit >> 3] ^= (1 << (bit & 7)).astype(np.uint8)
        t["features"][sent[:, 2]] = flip
    q["_pad"], t["_pad"] = 0xAB, 0xCD
    q["match"], q["distance"], q["match_x"], q["match_y"] = 7, 7, 7.0, 7.0
    # whether float32 can tell 0.999 / 1.001 radius from radius at these coordinates (tests/test_gated_fuzz_cpu.py)
    big = max(abs(box[0]), abs(box[1])) + max(abs(box[2]), abs(box[3]))
    if matcher == "guided" and len(eligible):
        with np.errstate(all="ignore"):
            big = float(np.nanmax(np.abs(px[eligible]) + np.abs(py[eligible])))
    watch = np.ones(len(eligible), bool)                                 # r2 den = inf cuts the band where e e overflows instead
    if matcher == "epipolar" and len(eligible):
        with np.errstate(all="ignore"):
            watch = np.isfinite(np.float32(radius) * np.float32(radius) * er.line(q[eligible], M)[3])
    return dict(q=q, t=t, M=M, radius=radius, sent=sent, watch=watch, uA=np.array(uA), uB=np.array(uB), eligible=np.array(eligible, np.int64),
                nfill=nfill, pow2=k, resolved=bool(1e-3 * radius >= 2.0 ** -24 * big), coarse=bool(radius < 8 * 2.0 ** -23 * big),
                epipole="epipole" in info and n1 >= 2, grid=(side, ox, oy), grid_real=cell_side(matcher, radius, t["x"], t["y"]),
                unwatched=int(okq.sum()) if c["plain"] else 0)


def statement(c, m, model=True, ratio=None, cross=None, max_dist=None, dist=None):
    f = gr.match_guided if c["matcher"] == "guided" else er.match_epipolar
    return f(m["q"], m["t"], m["M"], m["radius"], c["ratio"] if ratio is None else ratio, bool(c["cross"]) if cross is None else cross,
             c["max_dist"] if max_dist is None else max_dist, dist=dist, model=model)


# ---------------------------------------------------------------------------------------------------------------- the GPU legs
def _upload(torch, recs):
    return torch.from_numpy(np.ascontiguousarray(recs).view(np.uint8).reshape(-1).copy()).cuda() if len(recs) else \
        torch.zeros(128, dtype=torch.uint8, device="cuda")


def _compare(what, got, dev, lst, cnt, tail_clean, wout, wlist, fails):
    for f in FIELDS:
        if got is not None and not np.array_equal(got[f].view(np.uint32), wout[f].view(np.uint32)):
            bad = np.nonzero(got[f].view(np.uint32) != wout[f].view(np.uint32))[0]
            fails.append(f"{what}: field {f} differs at {bad.size} of {len(wout)} queries (first {bad[:6].tolist()})")
        elif not np.array_equal(dev[f].view(np.uint32), wout[f].view(np.uint32)):
            bad = np.nonzero(dev[f].view(np.uint32) != wout[f].view(np.uint32))[0]
            fails.append(f"{what}: device records, field {f} differs at {bad.size} of {len(wout)} queries (first {bad[:6].tolist()})")
    if cnt != len(wlist):
        fails.append(f"{what}: {cnt} accepted, statement {len(wlist)}")
    elif not np.array_equal(lst[:cnt].view(np.uint8), np.ascontiguousarray(wlist).view(np.uint8)):
        fails.append(f"{what}: the match list differs")
    if not tail_clean:
        fails.append(f"{what}: written past the count")


def run_case(ah, torch, det, c, m=None, want=None):
    """the single call of one case against the statement -> (failure lines, accepted, sentinel queries)"""
    m = make_case(c, ah.POINT_DTYPE) if m is None else m
    q, t = m["q"], m["t"]
    n1, n2 = len(q), len(t)
    wout, wlist, _ = statement(c, m) if want is None else want
    fails = []
    d1, d2 = _upload(torch, q), _upload(torch, t)
    d_out = torch.full((max(n1, 1) * 32,), 0xEE, dtype=torch.uint8, device="cuda")
    h_out = np.zeros(max(n1, 1), ah.MATCH_PAIR_DTYPE)
    out = q.copy()
    cnt = C.c_int(-1)
    Mh = np.ascontiguousarray(m["M"], np.float32)
    call = ah.lib.hak_match_guided if c["matcher"] == "guided" else ah.lib.hak_match_epipolar
    ah.check(call(det.ctx if c["ctx"] else None, d1.data_ptr(), n1, d2.data_ptr(), n2, Mh.ctypes.data_as(C.POINTER(C.c_float)),
                  float(m["radius"]), c["ratio"][0], c["ratio"][1], c["cross"], c["max_dist"], out.ctypes.data, d_out.data_ptr(),
                  C.byref(cnt), h_out.ctypes.data))
    dev = d1.cpu().numpy().view(ah.POINT_DTYPE)[:n1]
    lst_dev = d_out.cpu().numpy().view(ah.MATCH_PAIR_DTYPE)
    k = cnt.value
    if not 0 <= k <= n1:
        return [f"single: count {k} outside 0..{n1}"], 0, len(m["sent"])
    if not np.array_equal(lst_dev[:k].view(np.uint8), h_out[:k].view(np.uint8)):
        fails.append("single: the host copy of the list differs from the device's")
    _compare("single", out, dev, lst_dev, k, bool((lst_dev[k:].view(np.uint8) == 0xEE).all()), wout, wlist, fails)
    if not np.array_equal(d2.cpu().numpy()[:n2 * 104], np.ascontiguousarray(t).view(np.uint8).reshape(-1)):
        fails.append("single: the train set was written")
    return fails, len(wlist), len(m["sent"])


def run_group(ah, torch, det, cases, made):
    """the batch leg: the cases of one group as one ragged call; one record is broken; records past the counts hold NaN"""
    npairs, mp = len(cases), MAX_PTS
    c0 = cases[0]
    guided = c0["matcher"] == "guided"
    rdt = ah.HOMOGRAPHY_DTYPE if guided else ah.FUNDAMENTAL_DTYPE
    host = np.zeros((2 * npairs, mp), ah.POINT_DTYPE)
    host["x"], host["y"] = np.nan, np.nan
    num = np.zeros(2 * npairs, np.int32)
    recs = np.zeros(npairs, rdt)
    name = "H" if guided else "F"
    for k, (c, m) in enumerate(zip(cases, made)):
        n1, n2 = len(m["q"]), len(m["t"])
        host[2 * k, :n1], host[2 * k + 1, :n2] = m["q"], m["t"]
        num[2 * k], num[2 * k + 1] = n1, n2
        recs[k][name], recs[k]["hypothesis"], recs[k]["inliers"], recs[k]["n"] = m["M"], 3 + k, 10, 20
        if c["bad"] == "hypothesis":
            recs[k]["hypothesis"] = -1
        elif c["bad"] == "nan":
            recs[k][name][(c["seed"] >> 3) % 9] = np.nan
    d_pts, d_num, d_rec = _upload(torch, host), torch.from_numpy(num).cuda(), _upload(torch, recs)
    d_out = torch.full((npairs * mp * 32,), 0xEE, dtype=torch.uint8, device="cuda")
    d_cnt = torch.full((npairs,), -7, dtype=torch.int32, device="cuda")
    call = ah.lib.hak_match_guided_batch if guided else ah.lib.hak_match_epipolar_batch
    ah.check(call(det.ctx, d_pts.data_ptr(), d_num.data_ptr(), npairs, d_rec.data_ptr(), float(c0["radius"]), c0["ratio"][0], c0["ratio"][1],
                  c0["cross"], c0["max_dist"], d_out.data_ptr(), d_cnt.data_ptr()))
    ah.check(ah.lib.hak_sync(det.ctx))
    got = d_pts.cpu().numpy().view(ah.POINT_DTYPE).reshape(2 * npairs, mp)
    lists = d_out.cpu().numpy().view(ah.MATCH_PAIR_DTYPE).reshape(npairs, mp)
    cnts = d_cnt.cpu().numpy()
    fails = []
    if not np.array_equal(got[1::2].view(np.uint8), host[1::2].view(np.uint8)):
        fails.append("batch: a train set was written")
    for k, (c, m) in enumerate(zip(cases, made)):
        n1 = len(m["q"])
        wout, wlist, _ = statement(c, m, model=c["bad"] is None)
        kk = int(cnts[k])
        if not 0 <= kk <= n1:
            fails.append(f"batch pair {k} (#{c['index']}): count {kk} outside 0..{n1}")
            continue
        tail = bool((lists[k, kk:].view(np.uint8) == 0xEE).all()) and \
            np.array_equal(got[2 * k, n1:].view(np.uint8), host[2 * k, n1:].view(np.uint8))
        _compare(f"batch pair {k} (#{c['index']}{', broken record' if c['bad'] else ''})", None, got[2 * k, :n1], lists[k], kk, tail, wout,
                 wlist, fails)
    return fails


def describe(c, m):
    return (f"{c['matcher']:8s} {len(m['q']):4d} x {len(m['t']):<5d} train={c['train']:9s} query={c['query']:9s} {c['regime']:10s}"
            f"{(' ' + c['angle']) if c['regime'] == 'affine' else ''} 2^{m['pow2']} r={c['radius']:.4g} ratio={c['ratio']} cross={c['cross']} "
            f"max_dist={c['max_dist']} {'ctx' if c['ctx'] else 'pool'}{' cmiss' if c['cmiss'] and c['matcher'] == 'epipolar' else ''}"
            f"{' group' + str(c['group']) if c['group'] else ''}")


def run(cases, seed, only=None, verbose=True, out=sys.stdout, matcher=None):
    """cases 0 .. cases - 1 of `seed` (or the one case `only`, with its group); matcher: only the cases of that matcher.
    Returns the failing case indices."""
    import torch
    import akaze_hip as ah
    det = ah.Akazer()
    det.init((320, 240, 384), max_pts=MAX_PTS, batch=12)
    failed, nacc, nsent, nq, ngroups, t0 = [], 0, 0, 0, 0, time.time()
    idx = [only] if only is not None else list(range(cases))
    ran = 0
    for i in idx:
        c = draw_case(seed, i)
        if matcher is not None and c["matcher"] != matcher:
            continue
        ran += 1
        m = make_case(c, ah.POINT_DTYPE)
        fails, na, ns = run_case(ah, torch, det, c, m)
        g = c["group"]
        if g is not None and (only is not None or i == g[0] + g[1] - 1):     # the group's last case: the batch leg
            gc = [draw_case(seed, j) for j in range(g[0], g[0] + g[1])]
            if only is not None or g[0] + g[1] <= cases:
                gm = [m if j == i else make_case(cj, ah.POINT_DTYPE) for j, cj in zip(range(g[0], g[0] + g[1]), gc)]
                fails += run_group(ah, torch, det, gc, gm)
                ngroups += 1
        nacc, nsent, nq = nacc + na, nsent + ns, nq + len(m["q"])
        if verbose or fails:
            print(f"{'FAIL' if fails else 'ok  '} #{i:<4d} {describe(c, m)}  [{na} accepted, {ns} sentinel queries]", file=out, flush=True)
        for f in fails[:8]:
            print("       " + f, file=out, flush=True)
        if fails:
            failed.append(i)
    det.close()
    print(f"== seed {seed}: {ran} cases{' (' + matcher + ')' if matcher else ''} + {ngroups} batch groups, {len(failed)} failed {failed}; "
          f"{nq} queries, {nsent} with sentinels, {nacc} accepted matches, all compared with the statements in {time.time() - t0:.0f} s",
          file=out, flush=True)
    return failed


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=300)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--only", type=int, default=None)
    ap.add_argument("--quiet", action="store_true")
    a = ap.parse_args()
    sys.exit(1 if run(a.cases, a.seed, a.only, not a.quiet) else 0)
