// kernels_epipolar.hip -- epipolar guided matching: re-match a pair under its estimated fundamental matrix (hak_match_epipolar,
// gfx950, wave64).
//
// The rule is the contract in include/hipakaze.h (numpy statement: tests/epipolar_match_ref.py): query i has the line
// (a, b, c) = F (x, y, 1)^T in image 2 and is searched only among the train points closer than `radius` to that line; 2-NN ratio
// test and cross-check inside that band.  The train points are binned by kernels_guided.hip's k_guided_bin (hak_launch_guided_bin:
// the same grid of at most 64 x 64 cells, the same scratch), the reverse keys are turned into records by its k_guided_rev, and the
// accept rule and the compaction are the 2-NN matcher's finish kernels, unchanged.  The view of the scratch, the step a passer
// goes through (gd_pass) and the launch sequence are gated_common.h's, shared with the other two gated searches.  New here:
//   k_epipolar_search  one query per thread: the line, then a walk along the line's major axis -- grid rows for a mostly vertical
//                      line (|a| >= |b|), grid columns otherwise; per row (column) the interval of the other coordinate the band can
//                      reach, the cells of that interval, the exact float32 gate on every listed candidate, 16 x (v_xor, v_bcnt)
//                      per passer; two smallest hak_mkey(d, j) forward, atomicMin of hak_mkey(d, i) on the train point's word
// As in kernels_guided.hip the grid only decides WHICH candidates a query looks at and the exact gate decides which count, so the
// result is independent of the binning iff every j with G(i, j) is visited, and visited once (the two smallest keys of a stream
// must not see a key twice): a query walks distinct rows (columns), and every point is listed in exactly one cell.
//
// The conservative window.  Notation: u = 2^-24, L = 16384, s = sqrt(a a + b b) over the reals, "in domain" as the rule says.
// (1) A passer is close to the float32 line.  Let j pass G(i, j) and E = a x2 + b y2 + c over the reals.
//     Rounding is monotone, so fl(e e) < fl(r2 den) implies e e < r2 den over the reals (e, r2, den the float32 values).
//     r2 = fl(radius radius) <= radius^2 (1 + u) (+ 2^-150 where it is subnormal).  den = fl(fl(a a) + fl(b b)) <=
//     (s^2 (1 + u) + 2^-149)(1 + u), and den >= 2^-100 makes the absolute term a 2^-48 relative one: den <= s^2 (1 + 2^-22) and
//     s >= 2^-50.01.  Hence |e| < radius s (1 + 2^-21) + 2^-70 s.
//     e = fl(fl(fl(a x2) + fl(b y2)) + c): |E - e| <= u |e| + u |t1 + t2| + u (|a x2| + |b y2|) + 2^-149 with t = the rounded
//     products, |t1 + t2| <= (|a x2| + |b y2|)(1 + u) + 2^-149 and |a x2| + |b y2| <= (|a| + |b|) L <= sqrt(2) s L (nothing
//     overflows: a finite den bounds |a|, |b| by 2^64).  So |E| / s < radius (1 + 2^-20) + 2 sqrt(2) u L (1 + u) + 2^-98
//     < radius (1 + 2^-20) + 0.0028: the true distance of a passer from the line (a, b, c).
//     The search uses R = radius * 1.0001 + 0.01 in float64: R >= radius (1 + 2^-20) + 0.0028 + 0.007.
// (2) Major axis.  Say |a| >= |b| (rows; the other case exchanges the axes).  The line is x = m y + q, m = -b / a, |m| <= 1,
//     q = -c / a, and |E| < R s means |x2 - (m y2 + q)| < R s / |a| = R sqrt(1 + m m).  So a point with y2 in [Y0, Y1] that
//     passes has x2 in [min(m Y0, m Y1) + q - Rv, max(m Y0, m Y1) + q + Rv] with Rv = R sqrt(1 + m m) + 0.01.
// (3) The y-interval of a grid row.  In-domain points are finite with |coordinate| <= L < 2^20, so k_guided_bin's box holds them:
//     d = y2 - oy lies in [0, ey] over the reals, and their cell is gd_cell's value without its clamp doing anything but
//     folding the top edge into the last row.  With S = 1 / inv over the reals, v = fl(fl(d) inv) lies in d inv (1 +- u)^2, so
//     floor(v) = cy gives cy S (1 - 2u) <= d < (cy + 1) S (1 + 3u).  The last row also takes d up to ey, and ey <= ny S (1 + 3u):
//     for ny < 64 because floor(fl(fl(ey) inv)) = ny - 1, for ny = 64 because the bin kernel's side is >= fl(ey) / 64 and
//     inv = fl(1 / side).  So every in-domain point of row cy has y2 in [oy + cy S - mg, oy + (cy + 1) S + mg] for any
//     mg >= 3u 64 S; the kernel takes mg = 2^-15 S + 0.001 (2.6 times that, and the absolute part for the float64 arithmetic
//     below).  The same holds for the columns, and for the box as a whole: x2 in [ox - mg, ox + nx S + mg].
// (4) The window's own arithmetic is float64 on values below 2^40 wherever it matters: S, m, q, the row interval and the ends
//     m Y + q carry relative errors of a few 2^-53.  Where |q| <= 2^40 that is below 0.0005 px in x; where |q| > 2^40 the line
//     is beyond 2^39 for every y of the box (|m y| <= 2^21) and the computed interval is as well, so the row is skipped, rightly.
//     The interval is clamped to [-20000, 20000] (x2 itself lies in [-L, L]) and its ends are rounded to float32: at most
//     2^-10 px each.  Both losses are inside the 0.007 + 0.01 that R and Rv carry.
// (5) From an interval to cells: x2 is a float32 with xlo <= x2 <= xhi for the float32 ends, and gd_cell is non-decreasing, so
//     gd_cell(xlo) <= cell(x2) <= gd_cell(xhi) -- whatever the grid's origin and cell side are.  A row whose interval misses
//     the box of (3), or that lies wholly outside [-L, L] in y, has no in-domain point to offer and is skipped.
// Together: every in-domain j that passes G(i, j) sits in a cell of the row of its y2 that the walk of that row covers.
// Points that are not in domain are listed somewhere (border cells beyond 2^20, cell 0 for NaN) and fail the exact gate.
//
// Cost: a 1080p pair with 2 260 points has cells of 30 px and about one point per cell; a query walks up to 64 rows of about
// three cells each (the homography gate: 3 x 3 cells), tests the float32 gate on every listed candidate and loads the
// descriptors of the few passers.
#include "gated_common.h"

#define EP_L 16384.f             // |coordinate| bound of the rule's domain
#define EP_DEN_MIN 0x1p-100f     // floor on den = a a + b b

__global__ __launch_bounds__(256) void k_epipolar_search(const hak_point* __restrict__ pts1_base, const hak_point* __restrict__ pts2_base,
                                                          const int* __restrict__ n1_dev, int n1_host, long stride1, long stride2,
                                                          int count_stride, const hak_fundamental* __restrict__ d_F, hak_fundamental Fval,
                                                          double R, float r2, int cross, HakGuidedScratch sc, int4* __restrict__ fwd_base,
                                                          long fwd_stride)
{
    const int pair = blockIdx.y;
    const int n1 = n1_dev ? min(n1_dev[pair * count_stride], n1_host) : n1_host;     // (device counts: n1_host is the capacity)
    const hak_point* pts1 = pts1_base + (long)pair * stride1;
    const hak_point* pts2 = pts2_base + (long)pair * stride2;
    int4* fwd = fwd_base + (long)pair * fwd_stride;
    const GdView view = gd_view(sc, pair);
    const GdGrid& g = view.g;
    const hak_fundamental fr = d_F ? d_F[pair] : Fval;
    const bool model = gd_model(fr.F, fr.hypothesis);
    const double S = 1.0 / (double)g.inv;
    const double mg = S * 0x1p-15 + 1e-3;

    for (int i = blockIdx.x * 256 + threadIdx.x; i < n1; i += gridDim.x * 256) {
        const float x = pts1[i].x, y = pts1[i].y;
        // the line: float32, no FMA (the library is built with -ffp-contract=off)
        const float a = (fr.F[0] * x + fr.F[1] * y) + fr.F[2];
        const float b = (fr.F[3] * x + fr.F[4] * y) + fr.F[5];
        const float c = (fr.F[6] * x + fr.F[7] * y) + fr.F[8];
        const float den = a * a + b * b;
        const float r2den = r2 * den;
        GdQuery qs;
        // the rule's domain (every compare is false for NaN); a non-finite c passes no candidate (e is inf or NaN): no search
        if (model && fabsf(x) <= EP_L && fabsf(y) <= EP_L && den >= EP_DEN_MIN && den < INFINITY && fabsf(c) < INFINITY) {
            hak_desc_load(pts1 + i, qs.qd);
            auto scan = [&](int kbeg, int kend) {
                for (int k = kbeg; k < kend; k++) {
                    const float2 t = view.xy[k];
                    const float e = (a * t.x + b * t.y) + c;
                    if (fabsf(t.x) <= EP_L && fabsf(t.y) <= EP_L && (e * e) < r2den)                // the exact gate
                        gd_pass(qs, view, pts2, k, cross, i);
                }
            };
            // major coordinate p (walked: y for rows), minor coordinate v = m p + q
            const bool rows = fabsf(a) >= fabsf(b);
            const double A = rows ? a : b, B = rows ? b : a;
            const double m = -B / A, q = -(double)c / A;
            const double Rv = R * sqrt(1.0 + m * m) + 0.01;
            const float op = rows ? g.oy : g.ox, ov = rows ? g.ox : g.oy;
            const int np = rows ? g.ny : g.nx, nv = rows ? g.nx : g.ny;
            const double box0 = (double)ov - mg, box1 = (double)ov + nv * S + mg;
            for (int cp = 0; cp < np; cp++) {
                const double p0 = (double)op + cp * S - mg, p1 = (double)op + (cp + 1) * S + mg;
                if (p1 < -(double)EP_L || p0 > (double)EP_L) continue;
                const double va = m * p0 + q, vb = m * p1 + q;
                double vlo = fmin(va, vb) - Rv, vhi = fmax(va, vb) + Rv;
                if (!(vlo <= box1 && vhi >= box0)) continue;
                vlo = fmax(vlo, -20000.0);
                vhi = fmin(vhi, 20000.0);
                if (vlo > vhi) continue;
                const int cv0 = gd_cell((float)vlo, ov, g.inv, nv), cv1 = gd_cell((float)vhi, ov, g.inv, nv);
                if (rows)                                                     // cells cv0 .. cv1 of a row are consecutive in the sorted list
                    scan(view.off[cp * g.nx + cv0], view.off[cp * g.nx + cv1 + 1]);
                else
                    for (int cv = cv0; cv <= cv1; cv++) scan(view.off[cv * g.nx + cp], view.off[cv * g.nx + cp + 1]);
            }
        }
        fwd[i] = hak_knn_record(qs.best, qs.second);
    }
}

// the forward search of npairs pairs into fwd ({j1, d1, d2, 0} per query) and, cross != 0, rev(j) into sc.rev ({i, d, 512, 0}).
// With device-side counts (pair k: n1_dev / n2_dev[k * count_step]) n1_host / n2_host carry the capacity of the sets.  d_F: one
// record per pair on the device, or NULL: h_F[9] (host) serves the only pair.
void hak_launch_epipolar(hipStream_t st, const hak_point* pts1, const hak_point* pts2, const int* n1_dev, const int* n2_dev, int count_step,
                         int n1_host, int n2_host, long stride1, long stride2, int npairs, const hak_fundamental* d_F, const float* h_F,
                         float radius, int cross, const HakGuidedScratch& sc, int4* fwd, long fwd_stride)
{
    const double R = (double)radius * 1.0001 + 0.01;
    const float r2 = radius * radius;
    hak_fundamental fv{};
    if (!d_F)
        for (int k = 0; k < 9; k++) fv.F[k] = h_F[k];
    // (cells no smaller than the band's half-width)
    gd_launch(st, pts2, n2_dev, n2_host, stride2, count_step, npairs, (float)R, cross, sc, n1_host, [&](dim3 grid) {
        k_epipolar_search<<<grid, 256, 0, st>>>(pts1, pts2, n1_dev, n1_host, stride1, stride2, count_step, d_F, fv, R, r2, cross, sc, fwd,
                                                fwd_stride);
    });
}
