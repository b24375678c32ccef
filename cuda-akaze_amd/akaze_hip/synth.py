"""Seeded synthetic test scenes: the reference's data/img1.png / img2.png are not
in its checkout, so every benchmark / parity input at 1080p, 4K and 720p is generated here.

scene(w, h, seed)  -> uint8 image: smooth background gradient + random rectangles / discs / line
                     segments of random contrast + Gaussian noise, lightly blurred.
pair(w, h, seed)   -> (img1, img2): img2 = img1 warped by a fixed small homography
                     (3 deg rotation, 1.05 scale, 20 px shift), bilinear.
to_float(u8)       -> float32 in [0,1] exactly as main.cpp:149 (convertTo(CV_32FC1, 1.0/255.0)).
random_descriptors -> AkazePoint arrays for the 10k x 10k matcher config.
two_view_matches(n_in, n_out, seed) -> (records, inlier flags, F_true): matches of a 3-D point cloud seen by two pinhole
                     cameras with a known relative pose, plus uniformly random outlier records.
three_view_scene(seed, n, noise_px, outlier_share) -> K, the two relative poses and the match lists of (I0, I1) and (I1, I2)
                     over shared keypoint indices of I1, for the track-linking and absolute-pose stages.
three_view_keypoints(seed, n, noise_px, lookalike_share) -> the same cameras as three KEYPOINT sets with descriptors and
                     look-alike keypoints in the third image, for projection-guided matching.
"""
import numpy as np


def scene(w, h, seed, nshapes=None):
    rng = np.random.default_rng(seed)
    if nshapes is None:
        nshapes = max(25, int(175 * (w * h) / (1920.0 * 1080.0)))
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    img = 0.35 + 0.25 * (xx / w) + 0.15 * (yy / h)
    for _ in range(nshapes):
        kind = rng.integers(0, 3)
        cx, cy = rng.uniform(0, w), rng.uniform(0, h)
        amp = rng.uniform(0.08, 0.45) * (1 if rng.random() < 0.5 else -1)
        if kind == 0:       # rectangle
            rw, rh = rng.uniform(8, 0.12 * w), rng.uniform(8, 0.12 * h)
            x0, x1 = int(max(0, cx - rw / 2)), int(min(w, cx + rw / 2))
            y0, y1 = int(max(0, cy - rh / 2)), int(min(h, cy + rh / 2))
            img[y0:y1, x0:x1] += amp
        elif kind == 1:     # disc
            r = rng.uniform(5, 0.06 * min(w, h) + 6)
            x0, x1 = int(max(0, cx - r)), int(min(w, cx + r + 1))
            y0, y1 = int(max(0, cy - r)), int(min(h, cy + r + 1))
            if x1 > x0 and y1 > y0:
                sub = (xx[y0:y1, x0:x1] - cx) ** 2 + (yy[y0:y1, x0:x1] - cy) ** 2 <= r * r
                img[y0:y1, x0:x1] += amp * sub
        else:               # thick line segment
            ang = rng.uniform(0, np.pi)
            ln = rng.uniform(20, 0.15 * w)
            th = rng.uniform(1.5, 5.0)
            dx, dy = np.cos(ang), np.sin(ang)
            r = ln / 2 + th
            x0, x1 = int(max(0, cx - r)), int(min(w, cx + r + 1))
            y0, y1 = int(max(0, cy - r)), int(min(h, cy + r + 1))
            if x1 > x0 and y1 > y0:
                px = xx[y0:y1, x0:x1] - cx
                py = yy[y0:y1, x0:x1] - cy
                along = px * dx + py * dy
                across = -px * dy + py * dx
                img[y0:y1, x0:x1] += amp * ((np.abs(along) <= ln / 2) & (np.abs(across) <= th))
    img += rng.normal(0.0, 0.01, size=img.shape).astype(np.float32)
    # light 3x3 binomial blur (camera-like edges)
    p = np.pad(img, 1, mode="edge")
    img = (p[:-2, :-2] + 2 * p[:-2, 1:-1] + p[:-2, 2:] + 2 * p[1:-1, :-2] + 4 * p[1:-1, 1:-1] + 2 * p[1:-1, 2:] +
           p[2:, :-2] + 2 * p[2:, 1:-1] + p[2:, 2:]) / 16.0
    return np.clip(np.rint(img * 255.0), 0, 255).astype(np.uint8)


def warp(u8, angle_deg=3.0, scale=1.05, shift=(20.0, 20.0)):
    h, w = u8.shape
    a = np.deg2rad(angle_deg)
    ca, sa = np.cos(a) * scale, np.sin(a) * scale
    cx, cy = w / 2.0, h / 2.0
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    # inverse map: destination pixel -> source coordinate
    X, Y = xx - cx - shift[0], yy - cy - shift[1]
    det = ca * ca + sa * sa
    sx = (ca * X + sa * Y) / det + cx
    sy = (-sa * X + ca * Y) / det + cy
    sx = np.clip(sx, 0, w - 1.001)
    sy = np.clip(sy, 0, h - 1.001)
    x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    fx, fy = sx - x0, sy - y0
    f = u8.astype(np.float64)
    out = (f[y0, x0] * (1 - fx) * (1 - fy) + f[y0, x0 + 1] * fx * (1 - fy) +
           f[y0 + 1, x0] * (1 - fx) * fy + f[y0 + 1, x0 + 1] * fx * fy)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def pair(w, h, seed, nshapes=None):
    a = scene(w, h, seed, nshapes)
    return a, warp(a)


def to_float(u8, pitch=None):
    """uint8 -> float32 [0,1] (main.cpp:149), optionally padded to `pitch` columns."""
    f = (u8.astype(np.float64) * (1.0 / 255.0)).astype(np.float32)
    if pitch is None or pitch == u8.shape[1]:
        return np.ascontiguousarray(f)
    out = np.zeros((u8.shape[0], pitch), np.float32)
    out[:, :u8.shape[1]] = f
    return out


def random_descriptors(n, seed, dtype, planted_from=None, nplanted=0, maxflip=40):
    """n AkazePoints with uniformly random 486-bit descriptors (byte 60: top 2 bits zero)."""
    rng = np.random.default_rng(seed)
    pts = np.zeros(n, dtype)
    pts["features"] = rng.integers(0, 256, size=(n, 61), dtype=np.uint8)
    pts["features"][:, 60] &= 0x3F
    pts["x"] = rng.uniform(0, 1920, n).astype(np.float32)
    pts["y"] = rng.uniform(0, 1080, n).astype(np.float32)
    pts["match"] = -7
    if planted_from is not None and nplanted > 0:
        src = rng.choice(len(planted_from), nplanted, replace=False)
        dst = rng.choice(n, nplanted, replace=False)
        f = planted_from["features"][src].copy()
        for i in range(nplanted):
            bits = rng.choice(486, rng.integers(0, maxflip + 1), replace=False)
            for b in bits:
                f[i, b >> 3] ^= np.uint8(1 << (b & 7))
        pts["features"][dst] = f
    return pts


def two_view_matches(n_in, n_out, seed, w=1920, h=1080, focal=1500.0, noise=0.0, depth=(4.0, 12.0)):
    """Matches of a two-view scene for the fundamental-matrix tests and the timing tool, pure numpy.

    n_in 3-D points, uniformly random in the first camera's frustum at depths `depth`, are projected into two pinhole cameras
    (focal length `focal` px, principal point at the image centre) with a fixed relative pose (a rotation of a few degrees about
    all three axes and a baseline that is mostly sideways); only points that fall inside both w x h images are kept.  `noise` px of
    Gaussian noise is added to both projections.  n_out outlier records have both ends uniformly random in the image.  The
    records are shuffled.
    -> (records (n_in + n_out, 4) float32 {x1, y1, x2, y2}, inlier flags (n_in + n_out,) bool,
        F_true (3, 3) float64 with (x2 y2 1) F (x1 y1 1)^T = 0, Frobenius norm 1)"""
    rng = np.random.default_rng(seed)
    K = np.array([[focal, 0.0, w / 2.0], [0.0, focal, h / 2.0], [0.0, 0.0, 1.0]])
    ax, ay, az = np.deg2rad([2.0, -5.0, 1.5])
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    R = Rz @ Ry @ Rx
    t = np.array([-1.0, 0.05, 0.1])
    p1 = np.zeros((0, 2))
    p2 = np.zeros((0, 2))
    while len(p1) < n_in:                                              # rejection: keep the points both cameras see
        m = 2 * n_in + 16
        z = rng.uniform(depth[0], depth[1], m)
        px = np.stack([rng.uniform(0, w, m), rng.uniform(0, h, m), np.ones(m)], axis=1)
        X = (np.linalg.solve(K, px.T) * z).T                            # camera-1 coordinates
        X2 = X @ R.T + t
        q = X2 @ K.T
        q = q[:, :2] / q[:, 2:]
        keep = (X2[:, 2] > 0.5) & (q[:, 0] >= 0) & (q[:, 0] < w) & (q[:, 1] >= 0) & (q[:, 1] < h)
        p1 = np.concatenate([p1, px[keep, :2]])
        p2 = np.concatenate([p2, q[keep]])
    p1, p2 = p1[:n_in], p2[:n_in]
    if noise > 0.0:
        p1 = p1 + rng.normal(0.0, noise, p1.shape)
        p2 = p2 + rng.normal(0.0, noise, p2.shape)
    o = np.stack([rng.uniform(0, w, n_out), rng.uniform(0, h, n_out), rng.uniform(0, w, n_out), rng.uniform(0, h, n_out)], axis=1)
    recs = np.concatenate([np.concatenate([p1, p2], axis=1), o]).astype(np.float32)
    flags = np.concatenate([np.ones(n_in, bool), np.zeros(n_out, bool)])
    perm = rng.permutation(n_in + n_out)
    tx = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
    Ki = np.linalg.inv(K)
    F = Ki.T @ tx @ R @ Ki
    return recs[perm], flags[perm], F / np.linalg.norm(F)


def rotation_zyx(angles_deg):
    """R = Rz Ry Rx for (ax, ay, az) in degrees, as two_view_matches builds its fixed rotation"""
    ax, ay, az = np.deg2rad(np.asarray(angles_deg, np.float64))
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def two_view_scene(n_in, n_out, seed, angles_deg=(2.0, -5.0, 1.5), baseline=(-1.0, 0.05, 0.1), w=1920, h=1080, focal=1500.0,
                   noise=0.0, depth=(4.0, 12.0), swap=False):
    """two_view_matches with the relative pose chosen by the caller, for the pose-recovery tests and the timing tool, pure numpy.

    The second camera sees X2 = R X1 + t with R = rotation_zyx(angles_deg) and t = baseline (any length > 0; `depth` is in the
    same unit).  Points, noise, outliers and the shuffle as in two_view_matches.  swap = True exchanges the two images: the
    records become {x2, y2, x1, y1} and the pose its inverse (R^T, -R^T t).
    -> (records (n_in + n_out, 4) float32, inlier flags (n_in + n_out,) bool, F_true (3, 3) float64 of Frobenius norm 1,
        K (3, 3) float64, R (3, 3) float64, t (3,) float64 of unit length,
        z (n_in + n_out,) float64: the planted depth in the FIRST image's camera in units of the baseline length, NaN for outliers)"""
    rng = np.random.default_rng(seed)
    K = np.array([[focal, 0.0, w / 2.0], [0.0, focal, h / 2.0], [0.0, 0.0, 1.0]])
    R = rotation_zyx(angles_deg)
    t = np.asarray(baseline, np.float64).reshape(3)
    length = float(np.linalg.norm(t))
    assert length > 0.0
    p1, p2, z1, z2 = np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(0), np.zeros(0)
    for _ in range(400):                                                # rejection: keep the points both cameras see
        if len(p1) >= n_in:
            break
        m = 2 * n_in + 16
        z = rng.uniform(depth[0], depth[1], m)
        px = np.stack([rng.uniform(0, w, m), rng.uniform(0, h, m), np.ones(m)], axis=1)
        X = (np.linalg.solve(K, px.T) * z).T                            # camera-1 coordinates
        X2 = X @ R.T + t
        q = X2 @ K.T
        with np.errstate(all="ignore"):
            q = q[:, :2] / q[:, 2:]
        keep = (X2[:, 2] > 0.5) & (q[:, 0] >= 0) & (q[:, 0] < w) & (q[:, 1] >= 0) & (q[:, 1] < h)
        p1, p2 = np.concatenate([p1, px[keep, :2]]), np.concatenate([p2, q[keep]])
        z1, z2 = np.concatenate([z1, z[keep]]), np.concatenate([z2, X2[keep, 2]])
    assert len(p1) >= n_in, "the two cameras share too little of the scene"
    p1, p2, z1, z2 = p1[:n_in], p2[:n_in], z1[:n_in], z2[:n_in]
    if noise > 0.0:
        p1 = p1 + rng.normal(0.0, noise, p1.shape)
        p2 = p2 + rng.normal(0.0, noise, p2.shape)
    if swap:
        p1, p2, z1 = p2, p1, z2
        R, t = R.T, -(R.T @ t)
    o = np.stack([rng.uniform(0, w, n_out), rng.uniform(0, h, n_out), rng.uniform(0, w, n_out), rng.uniform(0, h, n_out)], axis=1)
    recs = np.concatenate([np.concatenate([p1, p2], axis=1), o]).astype(np.float32)
    flags = np.concatenate([np.ones(n_in, bool), np.zeros(n_out, bool)])
    zs = np.concatenate([z1 / length, np.full(n_out, np.nan)])
    perm = rng.permutation(n_in + n_out)
    tx = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
    Ki = np.linalg.inv(K)
    F = Ki.T @ tx @ R @ Ki
    return recs[perm], flags[perm], F / np.linalg.norm(F), K, R, t / length, zs[perm]


MATCH_DTYPE = np.dtype([("query", "<i4"), ("train", "<i4"), ("distance", "<i4"), ("second", "<i4"),
                        ("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4")])      # hak_match_pair


def three_view_scene(seed, n, noise_px=0.0, outlier_share=0.0, angles01=(2.0, -5.0, 1.5), t01=(-1.0, 0.05, 0.1),
                     angles12=(-1.5, -4.0, 2.0), t12=(-0.9, -0.1, 0.25), w=1920, h=1080, focal=1500.0, depth=(4.0, 12.0)):
    """Three pinhole views of one point cloud as two match lists that share the middle image, for the track-linking and
    absolute-pose tests and the timing tool, built beside two_view_scene, pure numpy.

    n 3-D points, uniformly random in the first camera's frustum at depths `depth`, that all three cameras see; camera 1 sees
    X1 = R01 X0 + t01, camera 2 sees X2 = R12 X1 + t12 (R = rotation_zyx(angles), t in the unit of `depth`, any length > 0).
    Every image has 2 n keypoints in a random order: the n projections, with `noise_px` of Gaussian noise added once per keypoint
    (so image 1's records are the same in both lists), and n spurious ones, uniformly random in the image.  List A holds one match
    per point from image 0 (query) to image 1 (train), list B one per point from image 1 (query) to image 2 (train), both in
    ascending query order as hak_match_knn2 writes them; a share `outlier_share` of each list, chosen independently, has its train
    end replaced by a randomly chosen other keypoint of that image (so train indices may repeat).
    -> (K (3, 3) float64, (R01, t01), (R12, t12), A, B: MATCH_DTYPE arrays of n records,
        flagsA, flagsB: (n,) bool, True for a correct match,
        X0: (n, 3) float64, the point behind each record of A in the FIRST camera's frame,
        pointA, pointB: (n,) int64, which point each record of A and of B belongs to)"""
    rng = np.random.default_rng(seed)
    K = np.array([[focal, 0.0, w / 2.0], [0.0, focal, h / 2.0], [0.0, 0.0, 1.0]])
    R01, R12 = rotation_zyx(angles01), rotation_zyx(angles12)
    t01, t12 = np.asarray(t01, np.float64).reshape(3), np.asarray(t12, np.float64).reshape(3)

    def project(X):
        q = X @ K.T
        with np.errstate(all="ignore"):
            return q[:, :2] / q[:, 2:]

    def inside(X, p):
        return (X[:, 2] > 0.5) & (p[:, 0] >= 0) & (p[:, 0] < w) & (p[:, 1] >= 0) & (p[:, 1] < h)

    X0 = np.zeros((0, 3))
    for _ in range(400):                                                # rejection: keep the points all three cameras see
        if len(X0) >= n:
            break
        m = 2 * n + 16
        z = rng.uniform(depth[0], depth[1], m)
        px = np.stack([rng.uniform(0, w, m), rng.uniform(0, h, m), np.ones(m)], axis=1)
        X = (np.linalg.solve(K, px.T) * z).T
        X1 = X @ R01.T + t01
        X2 = X1 @ R12.T + t12
        X0 = np.concatenate([X0, X[inside(X1, project(X1)) & inside(X2, project(X2))]])
    assert len(X0) >= n, "the three cameras share too little of the scene"
    X0 = X0[:n]
    X1 = X0 @ R01.T + t01
    X2 = X1 @ R12.T + t12
    pos, index = [], []
    for X in (X0, X1, X2):
        p = project(X)
        if noise_px > 0.0:
            p = p + rng.normal(0.0, noise_px, p.shape)
        spurious = np.stack([rng.uniform(0, w, n), rng.uniform(0, h, n)], axis=1)
        order = rng.permutation(2 * n)                                  # keypoint index of point j: order[j]; spurious: order[n + j]
        allp = np.zeros((2 * n, 2))
        allp[order] = np.concatenate([p, spurious])
        pos.append(allp)
        index.append(order[:n])

    def matches(a, b):
        lst = np.zeros(n, MATCH_DTYPE)
        good = np.ones(n, bool)
        good[rng.permutation(n)[:int(round(outlier_share * n))]] = False
        other = (index[b] + 1 + rng.integers(0, max(2 * n - 1, 1), n)) % (2 * n)      # any keypoint but the right one
        train = np.where(good, index[b], other)
        lst["query"], lst["train"] = index[a], train
        lst["distance"], lst["second"] = 20, 60
        lst["x1"], lst["y1"] = pos[a][index[a], 0], pos[a][index[a], 1]
        lst["x2"], lst["y2"] = pos[b][train, 0], pos[b][train, 1]
        by_query = np.argsort(lst["query"], kind="stable")
        return lst[by_query], good[by_query], by_query

    A, flagsA, pointA = matches(0, 1)
    B, flagsB, pointB = matches(1, 2)
    return K, (R01, t01), (R12, t12), A, B, flagsA, flagsB, X0[pointA], pointA.astype(np.int64), pointB.astype(np.int64)


FLEN = 61                                                                   # descriptor bytes, 486 bits used
POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("octave", "<i4"), ("response", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                        ("features", "u1", (FLEN,)), ("_pad", "u1", (3,)),
                        ("match", "<i4"), ("distance", "<i4"), ("match_x", "<f4"), ("match_y", "<f4")])      # hak_point


def three_view_keypoints(seed, n, noise_px=0.5, lookalike_share=0.3, angles01=(2.0, -5.0, 1.5), t01=(-1.0, 0.05, 0.1),
                         angles12=(-1.5, -4.0, 2.0), t12=(-0.9, -0.1, 0.25), w=1920, h=1080, focal=1500.0, depth=(4.0, 12.0),
                         lookalike_images=(2,)):
    """Three pinhole views of one point cloud as three KEYPOINT sets with descriptors, for the projection-guided matching tests and
    the timing tool, built beside three_view_scene (its cameras, its cloud recipe, its 2 n keypoints per image), pure numpy.  (The
    random draws are not three_view_scene's: the same seed gives another scene.)

    n 3-D points that all three cameras see.  Every point has a base descriptor of 486 random bits; its keypoint in each image is
    its projection, with `noise_px` of Gaussian noise, and carries the base with 5 .. 30 random bits flipped.  The other n keypoints
    of an image are spurious: uniformly random positions, random descriptors.  For a share `lookalike_share` of the points, one
    spurious keypoint of the THIRD image only is a look-alike: wherever it happens to lie, its descriptor is the point's base with
    0 .. 35 bits flipped -- what makes a whole-image ratio test drop, or mismatch, the point there (lookalike_images = (0, 1, 2)
    plants look-alikes, for a share of the points drawn per image, in every image).  Keypoints are in a random order.
    -> (K (3, 3) float64, (R01, t01), (R12, t12), [pts0, pts1, pts2]: POINT_DTYPE arrays of 2 n records (match fields -1),
        index: (3, n) int64, the keypoint of point j in image i, X0: (n, 3) float64, the points in the FIRST camera's frame,
        lookalike: (n,) int64, the look-alike keypoint of point j in image 2, or -1)"""
    rng = np.random.default_rng(seed)
    K = np.array([[focal, 0.0, w / 2.0], [0.0, focal, h / 2.0], [0.0, 0.0, 1.0]])
    R01, R12 = rotation_zyx(angles01), rotation_zyx(angles12)
    t01, t12 = np.asarray(t01, np.float64).reshape(3), np.asarray(t12, np.float64).reshape(3)

    def project(X):
        q = X @ K.T
        with np.errstate(all="ignore"):
            return q[:, :2] / q[:, 2:]

    def inside(X, p):
        return (X[:, 2] > 0.5) & (p[:, 0] >= 0) & (p[:, 0] < w) & (p[:, 1] >= 0) & (p[:, 1] < h)

    def flipped(base, lo, hi):
        """every row of the (m, 486) bit array with lo .. hi of its bits flipped"""
        out = base.copy()
        for r in range(len(out)):
            out[r, rng.choice(486, size=int(rng.integers(lo, hi + 1)), replace=False)] ^= 1
        return out

    X0 = np.zeros((0, 3))
    for _ in range(400):                                                # rejection: keep the points all three cameras see
        if len(X0) >= n:
            break
        m = 2 * n + 16
        z = rng.uniform(depth[0], depth[1], m)
        px = np.stack([rng.uniform(0, w, m), rng.uniform(0, h, m), np.ones(m)], axis=1)
        X = (np.linalg.solve(K, px.T) * z).T
        X1 = X @ R01.T + t01
        X2 = X1 @ R12.T + t12
        X0 = np.concatenate([X0, X[inside(X1, project(X1)) & inside(X2, project(X2))]])
    assert len(X0) >= n, "the three cameras share too little of the scene"
    X0 = X0[:n]
    X1 = X0 @ R01.T + t01
    X2 = X1 @ R12.T + t12
    base = rng.integers(0, 2, size=(n, 486), dtype=np.uint8)
    nlook = int(round(lookalike_share * n))
    lookalike = np.full(n, -1, np.int64)
    sets, index = [], []
    for i, X in enumerate((X0, X1, X2)):
        p = project(X)
        if noise_px > 0.0:
            p = p + rng.normal(0.0, noise_px, p.shape)
        spurious = np.stack([rng.uniform(0, w, n), rng.uniform(0, h, n)], axis=1)
        bits = np.concatenate([flipped(base, 5, 30), rng.integers(0, 2, size=(n, 486), dtype=np.uint8)])
        order = rng.permutation(2 * n)                                  # keypoint index of point j: order[j]; spurious: order[n + j]
        if i in lookalike_images and nlook:
            who = rng.permutation(n)[:nlook]                            # spurious keypoint k looks like point who[k]
            bits[n:n + nlook] = flipped(base[who], 0, 35)
            if i == 2:
                lookalike[who] = order[n:n + nlook]
        pts = np.zeros(2 * n, POINT_DTYPE)
        pts["x"][order], pts["y"][order] = np.concatenate([p, spurious]).T
        pts["features"][order] = np.packbits(np.pad(bits, ((0, 0), (0, 2))), axis=1, bitorder="little")
        pts["size"], pts["response"] = 4.0, 0.01
        pts["match"], pts["distance"], pts["match_x"], pts["match_y"] = -1, -1, -1.0, -1.0
        sets.append(pts)
        index.append(order[:n].astype(np.int64))
    return K, (R01, t01), (R12, t12), sets, np.stack(index), X0, lookalike


def four_view_scene(seed, n, noise_px=0.0, outlier_share=0.0, angles01=(2.0, -5.0, 1.5), t01=(-1.0, 0.05, 0.1),
                    angles12=(-1.5, -4.0, 2.0), t12=(-0.9, -0.1, 0.25), angles23=(1.0, -3.0, -1.0), t23=(-0.8, 0.1, 0.15),
                    w=1920, h=1080, focal=1500.0, depth=(4.0, 12.0)):
    """Four pinhole views of one point cloud as three match lists, each sharing an image with the next, for the triangulation
    tests and the timing tool: three_view_scene's recipe with a third relative pose and a third list, built beside it, pure numpy.

    n 3-D points, uniformly random in the first camera's frustum at depths `depth`, that all four cameras see; camera 1 sees
    X1 = R01 X0 + t01, camera 2 sees X2 = R12 X1 + t12, camera 3 sees X3 = R23 X2 + t23.  Keypoints, noise, spurious keypoints,
    the order of a list and its wrong matches as in three_view_scene; list C holds one match per point from image 2 (query) to
    image 3 (train).  (The random draws are not three_view_scene's: the same seed gives another scene.)
    -> (K (3, 3) float64, (R01, t01), (R12, t12), A, B: MATCH_DTYPE arrays of n records, flagsA, flagsB: (n,) bool,
        X0: (n, 3) float64, the point behind each record of A in the FIRST camera's frame, pointA, pointB: (n,) int64
        -- what three_view_scene returns -- and then
        (R23, t23), C: MATCH_DTYPE array of n records, flagsC: (n,) bool, pointC: (n,) int64)"""
    rng = np.random.default_rng(seed)
    K = np.array([[focal, 0.0, w / 2.0], [0.0, focal, h / 2.0], [0.0, 0.0, 1.0]])
    poses = [(rotation_zyx(a), np.asarray(t, np.float64).reshape(3)) for a, t in ((angles01, t01), (angles12, t12), (angles23, t23))]

    def project(X):
        q = X @ K.T
        with np.errstate(all="ignore"):
            return q[:, :2] / q[:, 2:]

    def inside(X, p):
        return (X[:, 2] > 0.5) & (p[:, 0] >= 0) & (p[:, 0] < w) & (p[:, 1] >= 0) & (p[:, 1] < h)

    def views(X):
        out = [X]
        for R, t in poses:
            out.append(out[-1] @ R.T + t)
        return out

    X0 = np.zeros((0, 3))
    for _ in range(400):                                                # rejection: keep the points all four cameras see
        if len(X0) >= n:
            break
        m = 2 * n + 16
        z = rng.uniform(depth[0], depth[1], m)
        px = np.stack([rng.uniform(0, w, m), rng.uniform(0, h, m), np.ones(m)], axis=1)
        X = (np.linalg.solve(K, px.T) * z).T
        seen = np.ones(m, bool)
        for Xv in views(X)[1:]:
            seen &= inside(Xv, project(Xv))
        X0 = np.concatenate([X0, X[seen]])
    assert len(X0) >= n, "the four cameras share too little of the scene"
    X0 = X0[:n]
    pos, index = [], []
    for X in views(X0):
        p = project(X)
        if noise_px > 0.0:
            p = p + rng.normal(0.0, noise_px, p.shape)
        spurious = np.stack([rng.uniform(0, w, n), rng.uniform(0, h, n)], axis=1)
        order = rng.permutation(2 * n)                                  # keypoint index of point j: order[j]; spurious: order[n + j]
        allp = np.zeros((2 * n, 2))
        allp[order] = np.concatenate([p, spurious])
        pos.append(allp)
        index.append(order[:n])

    def matches(a, b):
        lst = np.zeros(n, MATCH_DTYPE)
        good = np.ones(n, bool)
        good[rng.permutation(n)[:int(round(outlier_share * n))]] = False
        other = (index[b] + 1 + rng.integers(0, max(2 * n - 1, 1), n)) % (2 * n)      # any keypoint but the right one
        train = np.where(good, index[b], other)
        lst["query"], lst["train"] = index[a], train
        lst["distance"], lst["second"] = 20, 60
        lst["x1"], lst["y1"] = pos[a][index[a], 0], pos[a][index[a], 1]
        lst["x2"], lst["y2"] = pos[b][train, 0], pos[b][train, 1]
        by_query = np.argsort(lst["query"], kind="stable")
        return lst[by_query], good[by_query], by_query.astype(np.int64)

    A, flagsA, pointA = matches(0, 1)
    B, flagsB, pointB = matches(1, 2)
    Cl, flagsC, pointC = matches(2, 3)
    return K, poses[0], poses[1], A, B, flagsA, flagsB, X0[pointA], pointA, pointB, poses[2], Cl, flagsC, pointC
