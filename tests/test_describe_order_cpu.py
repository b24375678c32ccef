"""The gather-order table of the planned MLDB kernel (HakTables::dsc_ord, built by hak_describe_plan; host code, no GPU) through
hak_describe_order_query / hak_describe_order_bin.

The table decides which 64 samples of the window share one gather instruction of k_describe_runs; the kernel puts every value back at
its window index before it sums, so no result depends on it (tests/test_gpu_describe_gather.py).  What is asserted here is what the
table is for: every row is a permutation, carries the offsets of the samples it names, runs along image rows at the bin's centre
angle, and makes a gather instruction touch clearly fewer distinct 128-byte lines than the window order does."""
import numpy as np
import pytest

PLANNED = (4, 5, 6, 7, 9, 10)           # the sizes k_describe_runs serves (tests/test_abi_cpu.py)
f32 = np.float32


def _window(patsize):
    size3, size4 = int(np.ceil(2.0 * patsize / 3.0)), int(np.ceil(0.5 * patsize))
    return max(3 * size3, 4 * size4)


def _fields(slots):
    w = slots.reshape(-1).astype(np.int64)
    sb = lambda v: np.where(v > 127, v - 256, v)
    return sb(w & 0xFF), sb((w >> 8) & 0xFF), (w >> 16) & 1, (w >> 17) & 0x1FF, w >> 26


@pytest.mark.parametrize("patsize", PLANNED)
def test_rows_are_permutations_sorted_along_image_rows(ah, patsize):
    win = _window(patsize)
    nsmp = win * win
    nb, _ = ah.describe_order(patsize, 0)
    assert nb == 32
    for row in range(nb + 1):
        got, slots = ah.describe_order(patsize, row)
        assert got == nb
        l, k, have, i, rest = _fields(slots)
        assert not rest.any()
        assert sorted(i.tolist()) == list(range(7 * 64))                    # samples and pads: every staging word written once
        assert have[:nsmp].all() and not have[nsmp:].any()                  # the pads come last ...
        assert (i[nsmp:] >= nsmp).all() and not l[nsmp:].any() and not k[nsmp:].any()   # ... and gather at the keypoint
        s = i[:nsmp]
        assert np.array_equal(l[:nsmp], s % win - patsize) and np.array_equal(k[:nsmp], s // win - patsize)
        if row == nb:                                                       # the window order: slot = sample
            assert np.array_equal(i, np.arange(7 * 64))
            continue
        a = row * 2.0 * np.pi / nb
        v = k[:nsmp] * np.sin(a) + l[:nsmp] * np.cos(a)
        u = k[:nsmp] * np.cos(a) - l[:nsmp] * np.sin(a)
        dv, du = np.diff(v), np.diff(u)
        assert (dv > -1e-4).all()                                           # image row non-decreasing (keys rounded to 2^-16)
        assert (du[np.abs(dv) < 1e-4] > 0).all()                            # within one image row: column increasing
        if row == 0:                                                        # upright: exactly row-major in the image
            assert np.array_equal(s, sorted(s.tolist(), key=lambda q: (q % win, q // win)))


def test_unplanned_sizes_and_rows_outside_report_zero(ah):
    for patsize in (8, 11, 12):
        assert ah.describe_order(patsize, 0)[0] == 0
    assert ah.describe_order(10, -1)[0] == 0 and ah.describe_order(10, 33)[0] == 0


def test_every_float_lands_in_a_bin(ah):
    nb = ah.describe_order(10, 0)[0]
    edge = [f32((b + 0.5) * 2 * np.pi / nb) for b in range(nb)]
    angles = [f32(b * 2 * np.pi / nb) for b in range(nb)]
    angles += [np.nextafter(e, f32(s)) for e in edge for s in (-np.inf, np.inf)] + edge
    angles += [f32(v) for v in (0.0, -0.0, np.pi, -np.pi, -1.0, -6.0, 1e30, -1e30, 2.0 ** 31, -2.0 ** 31, 1e-45, np.inf, -np.inf, np.nan)]
    angles.append(np.nextafter(f32(2 * np.pi), f32(0)))
    for a in angles:
        assert 0 <= ah.describe_order_bin(float(a)) < nb, a
    for b in range(nb):                                                     # a centre goes to its own bin, its neighbourhood too
        assert ah.describe_order_bin(float(angles[b])) == b
        assert ah.describe_order_bin(float(angles[b]) + 0.4 * 2 * np.pi / nb) == b
    assert ah.describe_order_bin(float(np.nextafter(f32(2 * np.pi), f32(0)))) == 0


def _lines_per_instruction(slots, xf, yf, scale, angle, pitch=1920, w=1920, h=1080):
    """distinct 128-byte lines per gather instruction of one keypoint, summed over its 7 Lt and 7 {Lx, Ly} gathers; positions as
    k_describe_runs forms them (akazed.cu:1921-1922), in float32"""
    l, k, _, _, _ = _fields(slots)
    l, k = l.astype(f32), k.astype(f32)
    si, co = f32(np.sin(angle)), f32(np.cos(angle))
    xp = (f32(xf) + f32(scale) * (k * co - l * si) + f32(0.5)).astype(np.int64).clip(0, w - 1)
    yp = (f32(yf) + f32(scale) * (k * si + l * co) + f32(0.5)).astype(np.int64).clip(0, h - 1)
    px = (yp * pitch + xp).reshape(7, 64)
    return sum(len(set((px[n] * b // 128).tolist())) for n in range(7) for b in (4, 8))


def test_table_order_touches_fewer_lines_than_window_order(ah):
    """A condition on the table, not a timing: over seeded keypoints (scales 2, 3, 4; uniform angles; pitch 1920) the mean number of
    distinct 128-byte lines per gather instruction is at most 0.80 of the window order's (the table gives about 0.73)."""
    nb, window = ah.describe_order(10, 32)
    rows = [ah.describe_order(10, b)[1] for b in range(nb)]
    rng = np.random.default_rng(20)
    tab = win = 0
    for scale in (2, 3, 4):
        for _ in range(200):
            xf, yf, a = rng.uniform(100, 1820), rng.uniform(100, 980), f32(rng.uniform(0, 2 * np.pi))
            tab += _lines_per_instruction(rows[ah.describe_order_bin(float(a))], xf, yf, scale, a)
            win += _lines_per_instruction(window, xf, yf, scale, a)
    print(f"lines per keypoint: table order {tab / 600:.1f}, window order {win / 600:.1f}, ratio {tab / win:.3f}")
    assert tab <= 0.80 * win
    # upright (angle 0 -> row 0) gains the most
    up_t = sum(_lines_per_instruction(rows[0], 400.3 + 7 * j, 300.6 + 5 * j, 3, f32(0)) for j in range(50))
    up_w = sum(_lines_per_instruction(window, 400.3 + 7 * j, 300.6 + 5 * j, 3, f32(0)) for j in range(50))
    assert up_t <= 0.80 * up_w
