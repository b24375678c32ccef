"""The guarded arena of the write-contract tests (tests/test_gpu_plane_guard.py; numpy only, no GPU import): named image planes of
`nimg` images in ONE flat buffer, every word that is not an input pixel poisoned, and two checks on the buffer a kernel leaves behind.

Layout of one image slot (elements of `dtype`, float32 or int32):

    [front guard | plane 0: h rows of pitch p | guard | plane 1 ... | back guard]

A plane is (name, w, h, p) or (name, w, h, p, 2): the second form is the interleaved {Lx, Ly} plane of the Hessian kernels, rows of
2 p elements whose owned columns are [0, 2 w).  Planes of one arena may differ in shape (a decimating operator's source and
destination).  The image stride `stride` is the slot size, a multiple of 4 elements; image i's slot starts at i * stride, and
`offset(name)` is a plane's first element inside its slot, also a multiple of 4 when every pitch is (the streaming kernels store
16-byte groups).  All planes of a call share one allocation, as the kernels that address their output planes as 32-bit offsets from
the lowest one require.

Fill: everything that is not an input pixel holds the poison word -- the guards, the pad columns [w, p) of EVERY row (input planes
included: a tap that reads column w reads poison) and the whole of every plane that was not `put`.  float32: POISON_F32, a quiet NaN
with the payload 0x5A5A5, compared by bits (a kernel that computes with it propagates a NaN into its result, where the comparison with
the oracle -- which is given zero padding -- finds it); int32: POISON_I32 = 0x5A5A5A5A, the sentinel of tests/test_gpu_strip_seams.py.

Guard size: GUARD_ROWS = 32 rows of the widest row of the arena, in front of, between and behind the planes.  That is more than any
kernel's deepest reach beyond the rows it stores, so that an overrun of a whole halo stays inside the allocation and becomes a failed
assertion, not a fault:
    k_hessian_stream<V, S>  warms up 4 S + 2 rows per row segment: 18 at dilation S = 4 (kernels_hessian_stream.hip)
    k_fed_sf / k_fed_multi  warm up NS + 4 rows at NS fused steps: 12 at NS = 8 (kernels_fedsf.hip, kernels_fed.hip)
    k_base_stream           2 + R rows, R <= 4; the tile kernels' halos are at most 4 S = 16 (k_hessian_fused) and 36 + 2 steps
                            of k_level_tile, which never leave LDS
32 is the next power of two above 18.

Checks on a buffer `after` the call (same size, downloaded):
    violations(after, written)  every changed word outside the owned pixels [0, h) x [0, w) of the planes named in `written`,
                                classified by where it lies (CLASSES); planes not named must come back exactly as they went in,
                                inputs and all-poison planes alike
    unwritten(after, name)      owned pixels of a plane that still hold the poison
"""
import numpy as np

GUARD_ROWS = 32
POISON_F32_BITS = 0x7FC5A5A5            # quiet NaN (bit 22 set), payload 0x5A5A5
POISON_I32 = 0x5A5A5A5A
POISON_U8 = 0xA5                        # pad columns of the uint8 images two FAST operators read

# where a changed word lies
PAD = "pad column of an owned row"      # columns [w, p) of a row [0, h) of a written plane
BELOW = "row below the plane"           # the first half of the guard behind a plane (the back guard: all of it)
FRONT = "front guard"                   # the second half of the guard in front of a plane (the slot's front guard: all of it)
OTHER_PLANE = "another plane's slot"    # any word of the rows of a plane the call was not to write
OTHER_IMAGE = "another image's slot"    # any word of the slot of an image the call was not given
CLASSES = (PAD, BELOW, FRONT, OTHER_PLANE, OTHER_IMAGE)
_OWNED, _PAD, _BELOW, _FRONT = 0, 1, 2, 3


def poison(dtype):
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return np.array([POISON_F32_BITS], np.uint32).view(np.float32)[0]
    if dtype == np.int32:
        return np.int32(POISON_I32)
    raise TypeError("the guarded arena holds float32 or int32 planes")


def align4(n):
    return (n + 3) // 4 * 4


def align64(n):
    return (n + 63) // 64 * 64


def pitches(w):
    """the pitches every width is crossed with: align4(w) (no padding when w % 4 == 0), that plus 4, and the context's align64(w)"""
    return sorted({align4(w), align4(w) + 4, align64(w)})


def padded_u8(a, sp):
    """dense (..., h, w) uint8 -> pitch sp with POISON_U8 in the pad columns"""
    out = np.full(a.shape[:-1] + (sp,), POISON_U8, np.uint8)
    out[..., :a.shape[-1]] = a
    return out


class Violation:
    def __init__(self, cls, plane, image, row, col, got):
        self.cls, self.plane, self.image, self.row, self.col, self.got = cls, plane, image, row, col, got

    def __repr__(self):
        return f"<{self.cls}: plane {self.plane!r} image {self.image} row {self.row} col {self.col} = {self.got:#010x}>"


class Report(list):
    """the first few violations of every class, as a list; `count` changed words in all, `classes` {class: count}"""
    count = 0
    classes = {}

    def __str__(self):
        return f"{self.count} words written outside the owned pixels {self.classes}: {list(self)}"


class Arena:
    def __init__(self, dtype, planes, nimg=1, guard_rows=GUARD_ROWS):
        self.dtype = np.dtype(dtype)
        self.poison = poison(dtype)
        self.nimg = nimg
        if guard_rows < GUARD_ROWS:
            raise ValueError(f"guards are at least {GUARD_ROWS} rows")
        self.planes = {}
        self.order = []
        for spec in planes:
            name, w, h, p = spec[:4]
            lanes = spec[4] if len(spec) > 4 else 1
            if lanes not in (1, 2) or not 0 < w <= p or h < 1 or name in self.planes:
                raise ValueError(f"bad plane {spec!r}")
            self.planes[name] = dict(w=w * lanes, h=h, row=p * lanes, lanes=lanes, index=len(self.order))
            self.order.append(name)
        self.guard = guard_rows * align4(max(q["row"] for q in self.planes.values()))
        off = self.guard
        for name in self.order:
            q = self.planes[name]
            q["off"] = off
            off += q["h"] * q["row"] + self.guard
        self.stride = align4(off)
        self.size = self.stride * nimg
        # per word of a slot: the plane it is told by (index), where it lies with respect to it, its row and its column
        self._plane = np.zeros(self.stride, np.int16)
        self._where = np.zeros(self.stride, np.int8)
        self._row = np.zeros(self.stride, np.int32)
        self._col = np.zeros(self.stride, np.int32)
        last = len(self.order) - 1
        for k, name in enumerate(self.order):
            q = self.planes[name]
            o, n, r = q["off"], q["h"] * q["row"], q["row"]
            i = np.arange(n)
            self._plane[o:o + n] = k
            self._row[o:o + n], self._col[o:o + n] = i // r, i % r
            self._where[o:o + n] = np.where(i % r < q["w"], _OWNED, _PAD)
            # the guard in front: all of the slot's front guard, else the second half of the guard shared with the plane before
            lo = 0 if k == 0 else o - self.guard + self.guard // 2
            j = np.arange(lo - o, 0)
            self._plane[lo:o], self._where[lo:o] = k, _FRONT
            self._row[lo:o], self._col[lo:o] = j // r, j % r               # (negative rows: rows in front of the plane)
            # the guard behind: all of the back guard (and the slot's alignment tail), else the first half
            hi = self.stride if k == last else o + n + self.guard // 2
            j = np.arange(n, n + hi - (o + n))
            self._plane[o + n:hi], self._where[o + n:hi] = k, _BELOW
            self._row[o + n:hi], self._col[o + n:hi] = j // r, j % r
        self.init = np.full(self.size, self.poison, self.dtype)

    # ---- geometry
    def offset(self, name):
        return self.planes[name]["off"]

    def address(self, base, name, image=0):
        """byte address of a plane of image `image` in a device copy of the buffer at `base`"""
        return base + 4 * (image * self.stride + self.offset(name))

    def rows(self, buf, name):
        """view (nimg, h, row length) of a plane's rows in `buf`, pad columns included"""
        q = self.planes[name]
        slots = np.asarray(buf).reshape(self.nimg, self.stride)
        return slots[:, q["off"]:q["off"] + q["h"] * q["row"]].reshape(self.nimg, q["h"], q["row"])

    def owned(self, buf, name):
        """view (nimg, h, w) of a plane's owned pixels in `buf` (interleaved: (nimg, h, 2 w))"""
        return self.rows(buf, name)[:, :, :self.planes[name]["w"]]

    # ---- fill
    def put(self, name, data):
        """input pixels: data (nimg, h, w) or, for one image, (h, w); interleaved planes (.., h, 2 w).  The pad columns stay poisoned"""
        q = self.planes[name]
        data = np.asarray(data)
        if data.dtype != self.dtype:
            raise TypeError(f"{name}: {data.dtype} into an arena of {self.dtype}")
        self.owned(self.init, name)[...] = data.reshape(self.nimg, q["h"], q["w"])
        return self

    def buffer(self):
        """a fresh copy of the filled buffer, to upload"""
        return self.init.copy()

    # ---- checks
    def _bits(self, a):
        a = np.ascontiguousarray(a)
        if a.dtype != self.dtype or a.size != self.size:
            raise ValueError("not a buffer of this arena")
        return a.reshape(-1).view(np.uint32)

    def violations(self, after, written, images=None, first=4):
        """changed words outside the owned pixels of the planes in `written` (of the images in `images`; None: all)"""
        for name in written:
            if name not in self.planes:
                raise KeyError(name)
        wr = np.zeros(len(self.order), bool)
        wr[[self.planes[n]["index"] for n in written]] = True
        given = np.zeros(self.nimg, bool)
        given[list(range(self.nimg) if images is None else images)] = True
        changed = (self._bits(after) != self._bits(self.init)).reshape(self.nimg, self.stride)
        free = (wr[self._plane] & (self._where == _OWNED))[None, :] & given[:, None]
        img, pos = np.nonzero(changed & ~free)
        where, plane = self._where[pos], self._plane[pos]
        # by location: an image the call was not given; else the guards; else the rows of a plane it was not to write; else padding
        code = np.where(~given[img], 4, np.where(where == _BELOW, 1, np.where(where == _FRONT, 2, np.where(~wr[plane], 3, 0))))
        rep = Report()
        rep.count, rep.classes = int(len(pos)), {}
        bits = self._bits(after).reshape(self.nimg, self.stride)
        for c, cls in enumerate(CLASSES):
            hit = np.nonzero(code == c)[0]
            if len(hit):
                rep.classes[cls] = int(len(hit))
            for t in hit[:first].tolist():
                i, k = int(img[t]), int(pos[t])
                rep.append(Violation(cls, self.order[int(plane[t])], i, int(self._row[k]), int(self._col[k]), int(bits[i, k])))
        return rep

    def unwritten(self, after, name, images=None):
        """owned pixels of plane `name` that still hold the poison: [(image, row, column)]"""
        bits = self.owned(self._bits(after), name)
        left = np.argwhere(bits == np.array([self.poison]).view(np.uint32)[0])
        keep = range(self.nimg) if images is None else images
        return [tuple(int(v) for v in t) for t in left if t[0] in keep]
