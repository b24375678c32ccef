/*
 * asan_main.c -- runs the CPU oracle (float path, integer FAST path, both matchers) under AddressSanitizer + UBSan on a few
 * seeded scenes, including odd sizes, a clamp below the keypoint count, no-descriptor and upright runs (SURVEY.md 5:
 * "sanitizers on the CPU build"), and every stage function of the FAST path once on int32 planes far outside the uint8 range
 * (run_stages), and the six point functions on keypoints planted on the limits and corners of every level's accepted domain, turned to
 * the diagonals (run_points; tests/keypoint_stage.py has the full case list).  TEST INFRASTRUCTURE ONLY, like everything in
 * oracle/: `make -C oracle asan`.
 * Signed wrap-around in the FAST path is spelled out with unsigned arithmetic there, so UBSan's signed-overflow check stays on.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

typedef struct { float x, y; int octave; float response, size, angle; unsigned char features[61]; int match, distance; float match_x, match_y; } Pt;
typedef struct { int noctaves, max_scale; float per, kcontrast, soffset; int reordering; float derivative_factor, dthreshold;
                 int diffusivity, descriptor_pattern_size, upright; } Prm;
typedef struct { int query, train, distance, second; float x1, y1, x2, y2; } MatchPair;

long okz_arena_floats(int w, int h, int p, int noctaves, int max_scale);
long fkz_arena_ints(int w, int h, int p, int noctaves, int max_scale);
int okz_detect_and_compute(const float* image, int w, int h, int p, const Prm* prm, Pt* pts, int max_pts, int desc, float* tmem, float* kc);
int fkz_detect_and_compute(const unsigned char* image, int w, int h, int sp, int p, const Prm* prm, Pt* pts, int max_pts, int desc, int* tmem, int* kc);
void okz_match(Pt* pts1, int n1, const Pt* pts2, int n2);
int okz_match_knn2(Pt* pts1, int n1, const Pt* pts2, int n2, int ratio_num, int ratio_den, int cross, int max_dist, MatchPair* out);
int okz_sizeof_point(void);
void fkz_gauss_taps(float var, int radius, int* ik);
void fkz_conv_u8(const unsigned char* src, int sp, int* dst, int w, int h, int p, const int* k, int R);
void fkz_conv_int(const int* src, int* dst, int w, int h, int p, const int* k, int R);
void fkz_down_smooth(const int* src, int* dst, int* smooth, int sw, int sh, int sp, int dw, int dh, int dp, const int* k);
int fkz_kcontrast(const int* smooth, int w, int h, int p, float per, int* hmax_out, int* hist_out);
void fkz_flow(const int* src, int* dst, int type, int kcontrast, int w, int h, int p);
void fkz_nld_step(const int* src, const int* flow, int* dst, float tau, int w, int h, int p);
void fkz_hessian(const int* src, int* dxo, int* dyo, int* det, int step, int w, int h, int p);

int okz_layout(int w, int h, int p, int noctaves, int max_scale, int* owhps, int* osizes, int* offsets);
int okz_schedule(const Prm* prm, int noct, float* sizes, int* sigma_size, float* borders);
void okz_orient_weights(float* tab);
void okz_compare_indices(int* idx1, int* idx2);
void okz_derivate(const float* src, float* dxo, float* dyo, int step, int w, int h, int p);
void okz_hessian(const float* dx, const float* dy, float* det, int step, int w, int h, int p);
void okz_refine_point(Pt* pt, const float* det, int o, int p);
void okz_orient_point(Pt* pt, const float* dxd, const float* dyd, int o, int w, int h, int p, const float* wtab);
void okz_describe_point(Pt* pt, const float* imd, const float* dxd, const float* dyd, int o, int w, int h, int p, int patsize, const int* idx1, const int* idx2);
void fkz_refine(Pt* pt, const int* det, int o, int p);
void fkz_orient(Pt* pt, const int* dxd, const int* dyd, int o, int w, int h, int p, const float* wtab);
void fkz_describe(Pt* pt, const int* imd, const int* dxd, const int* dyd, int o, int w, int h, int p, int patsize, const int* idx1, const int* idx2);

static unsigned rng_state;
static unsigned rnd(void) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

/* gradient + rectangles + discs + a little noise: enough structure for a few hundred keypoints */
static void scene(unsigned char* u8, int w, int h, unsigned seed, int shift)
{
    rng_state = seed * 2654435761u + 1;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) u8[(size_t)y * w + x] = (unsigned char)(60 + (x + shift) * 80 / w + y * 40 / h);
    int nshapes = 20 + w * h / 4000;
    for (int s = 0; s < nshapes; s++) {
        int cx = (int)(rnd() % (unsigned)w) + shift, cy = (int)(rnd() % (unsigned)h), r = 3 + (int)(rnd() % 14), v = (int)(rnd() % 256), disc = rnd() & 1;
        for (int y = cy - r; y <= cy + r; y++)
            for (int x = cx - r; x <= cx + r; x++)
                if (x >= 0 && x < w && y >= 0 && y < h && (!disc || (x - cx) * (x - cx) + (y - cy) * (y - cy) <= r * r))
                    u8[(size_t)y * w + x] = (unsigned char)v;
    }
    for (size_t i = 0; i < (size_t)w * h; i++) { int v = u8[i] + (int)(rnd() % 5) - 2; u8[i] = (unsigned char)(v < 0 ? 0 : v > 255 ? 255 : v); }
}

static int run_case(int w, int h, const Prm* prm, int max_pts, int desc)
{
    int p = (w + 127) / 128 * 128, n[2], nf[2];
    unsigned char* u8 = malloc((size_t)w * h);
    float* img = malloc(sizeof(float) * (size_t)h * p);
    float* arena = malloc(sizeof(float) * (size_t)okz_arena_floats(w, h, p, prm->noctaves, prm->max_scale));
    int* iarena = malloc(sizeof(int) * (size_t)fkz_arena_ints(w, h, p, prm->noctaves, prm->max_scale));
    Pt* pts[2], *fpts[2];
    for (int k = 0; k < 2; k++) {
        pts[k] = malloc(sizeof(Pt) * (size_t)max_pts);              /* exactly max_pts records: an overrun is an ASan error */
        fpts[k] = malloc(sizeof(Pt) * (size_t)max_pts);
        scene(u8, w, h, 7u + (unsigned)(w * 31 + h), k * 3);
        for (int y = 0; y < h; y++)
            for (int x = 0; x < p; x++) img[(size_t)y * p + x] = x < w ? u8[(size_t)y * w + x] * (float)(1.0 / 255.0) : 0.f;
        float kc; int ikc;
        n[k] = okz_detect_and_compute(img, w, h, p, prm, pts[k], max_pts, desc, arena, &kc);
        nf[k] = fkz_detect_and_compute(u8, w, h, w, p, prm, fpts[k], max_pts, desc, iarena, &ikc);
    }
    okz_match(pts[0], n[0], pts[1], n[1]);
    okz_match(fpts[0], nf[0], fpts[1], nf[1]);
    okz_match(pts[0], n[0], pts[1], n[1] < 5 ? n[1] : 5);           /* n2 < 16 (D10) */
    okz_match(pts[0], n[0], pts[1], 0);
    MatchPair* out = malloc(sizeof(MatchPair) * (size_t)(n[0] > 0 ? n[0] : 1));
    int acc = okz_match_knn2(pts[0], n[0], pts[1], n[1], 4, 5, 1, 96, out);
    printf("  %4d x %-4d oct %d ms %d diff %d pat %2d upright %d max_pts %5d desc %d: float %d / %d, FAST %d / %d, knn2 %d\n", w, h, prm->noctaves,
           prm->max_scale, prm->diffusivity, prm->descriptor_pattern_size, prm->upright, max_pts, desc, n[0], n[1], nf[0], nf[1], acc);
    free(out);
    for (int k = 0; k < 2; k++) { free(pts[k]); free(fpts[k]); }
    free(u8); free(img); free(arena); free(iarena);
    return n[0] + nf[0];
}

/* Every FAST stage function once on int32 planes far outside what a uint8 image yields (tests/fast_domain.py has the full-size
 * generators): `ramp_blown`, the scene times an amplitude that rises from 2^6 to 2^22 across the plane, and `full_range`, random
 * int32 with INT_MIN / INT_MAX / -1 / 0 on the border.  The statement claims to cover any int32 value and contrast factors
 * 0 .. 46340: wrapping products, a negative sum of squares under sqrt, a saturating conversion -- none of it may be undefined here. */
static long run_stages(int w, int h, int full_range)
{
    int p = (w + 63) / 64 * 64, dw = w / 2, dh = h / 2, dp = (dw + 63) / 64 * 64;
    size_t n = (size_t)h * p;
    unsigned char* u8 = malloc((size_t)w * h);
    int *a = calloc(n, sizeof(int)), *sm = calloc(n, sizeof(int)), *g = calloc(n, sizeof(int)), *o1 = calloc(n, sizeof(int));
    int *o2 = calloc(n, sizeof(int)), *o3 = calloc(n, sizeof(int)), *d1 = calloc((size_t)dh * dp, sizeof(int)), *d2 = calloc((size_t)dh * dp, sizeof(int));
    scene(u8, w, h, 11u + (unsigned)full_range, 0);
    static const int special[4] = {(int)0x80000000, 0x7FFFFFFF, -1, 0};
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            if (full_range) {
                unsigned v = rnd() ^ (rnd() << 7);
                int edge = y == 0 || y == h - 1 || x == 0 || x == w - 1;
                a[(size_t)y * p + x] = edge ? special[(x + y) & 3] : (int)v;
            } else {
                int shift = 6 + 16 * x / (w - 1);                              /* amplitude 2^6 .. 2^22: 255 << 22 < 2^31 */
                a[(size_t)y * p + x] = (int)((unsigned)u8[(size_t)y * w + x] << shift);
            }
        }
    int k1[8] = {0}, kb[8] = {0}, hist[300], hmax = 0;
    long sum = 0;
    fkz_gauss_taps(1.f, 2, k1);
    fkz_gauss_taps(3.2f, 5, kb);
    fkz_conv_u8(u8, w, o1, w, h, p, kb, 5);
    fkz_conv_int(a, sm, w, h, p, k1, 2);
    fkz_conv_int(a, o1, w, h, p, kb, 5);
    fkz_down_smooth(a, d1, d2, w, h, p, dw, dh, dp, k1);
    int kc = fkz_kcontrast(sm, w, h, p, 0.7f, &hmax, hist);
    sum += fkz_kcontrast(a, w, h, p, 0.7f, &hmax, hist) + hist[0];
    static const int kcs[4] = {0, 1, 46340, -1};                              /* -1: the plane's own */
    for (int type = 0; type < 4; type++)
        for (int i = 0; i < 4; i++) {
            fkz_flow(a, g, type, kcs[i] < 0 ? kc : kcs[i], w, h, p);
            fkz_nld_step(a, g, o1, 41.f, w, h, p);                             /* stepfac * step wraps (F1) */
            fkz_nld_step(o1, g, o2, 0.07f, w, h, p);
            sum += o2[(size_t)(h / 2) * p + w / 2];
        }
    for (int step = 1; step <= 6; step++) {
        fkz_hessian(a, o1, o2, o3, step, w, h, p);
        sum += o3[(size_t)(h / 2) * p + w / 2];
    }
    printf("  stage functions on a %3d x %-3d %s plane: own contrast factor %d, lattice maximum %d\n", w, h, full_range ? "full_range" : "ramp_blown",
           kc, hmax);
    free(u8); free(a); free(sm); free(g); free(o1); free(o2); free(o3); free(d1); free(d2);
    return sum;
}

/* The six point functions on planted keypoints: the four corners and four limit mid-points of every level's accepted domain (the
 * border rule of okz_extrema_map), at the integer position and one level pixel off it on either side, turned to the four
 * diagonals -- where the farthest MLDB sample comes within a pixel of the plane edge (pattern 10) or is clamped (pattern 12).
 * Every plane is allocated with exactly h * p elements: a read outside it is an ASan error.  The int planes hold any int32. */
static long run_points(int w, int h, int patsize)
{
    Prm prm = {2, 4, 0.7f, 0.03f, 1.6f, 1, 1.5f, 0.001f, 1, patsize, 0};
    int owhps[24], osizes[8], offsets[9], sig[8], idx1[488], idx2[488];
    float sizes[8], borders[8], wtab[36];
    int noct = okz_layout(w, h, (w + 127) / 128 * 128, prm.noctaves, prm.max_scale, owhps, osizes, offsets);
    okz_schedule(&prm, noct, sizes, sig, borders);
    okz_orient_weights(wtab);
    okz_compare_indices(idx1, idx2);
    long sum = 0, npts = 0;
    rng_state = 977u + (unsigned)patsize;
    for (int l = 0; l < noct * prm.max_scale; l++) {
        int o = l / prm.max_scale, ow = owhps[3 * o], oh = owhps[3 * o + 1], op = owhps[3 * o + 2];
        size_t n = (size_t)oh * op;
        float *lt = malloc(n * sizeof(float)), *lx = malloc(n * sizeof(float)), *ly = malloc(n * sizeof(float)), *det = malloc(n * sizeof(float));
        int *ilt = malloc(n * sizeof(int)), *ilx = malloc(n * sizeof(int)), *ily = malloc(n * sizeof(int)), *idet = malloc(n * sizeof(int));
        for (size_t i = 0; i < n; i++) {
            lt[i] = (float)(rnd() % 65536u) * (1.f / 65536.f);
            ilt[i] = (int)(rnd() ^ (rnd() << 7));
        }
        okz_derivate(lt, lx, ly, sig[l], ow, oh, op);
        okz_hessian(lx, ly, det, sig[l], ow, oh, op);
        fkz_hessian(ilt, ilx, ily, idet, sig[l], ow, oh, op);
        int lim[2][2];                                                  /* [axis][first, last] accepted coordinate */
        for (int ax = 0; ax < 2; ax++) {
            int ext = ax ? oh : ow, first = -1, last = -1;
            for (int i = (int)borders[o * prm.max_scale]; i < ext; i++)
                if ((int)(i - borders[l] + 0.5f) - 1 >= 0 && (int)(i + borders[l] + 0.5f) + 1 < ext) { if (first < 0) first = i; last = i; }
            if (first < 0) { fprintf(stderr, "run_points: level %d has no accepted domain\n", l); exit(1); }
            lim[ax][0] = first; lim[ax][1] = last;
        }
        int xs[3] = {lim[0][0], (lim[0][0] + lim[0][1]) / 2, lim[0][1]}, ys[3] = {lim[1][0], (lim[1][0] + lim[1][1]) / 2, lim[1][1]};
        for (int yi = 0; yi < 3; yi++)
            for (int xi = 0; xi < 3; xi++) {
                if (xi == 1 && yi == 1) continue;
                for (int k = 0; k < 4; k++) {
                    Pt pt, fpt;
                    memset(&pt, 0, sizeof(pt));
                    pt.x = (float)(xs[xi] << o); pt.y = (float)(ys[yi] << o); pt.octave = l; pt.size = sizes[l];
                    fpt = pt;
                    fpt.x += (float)(k & o); fpt.y += (float)((k >> 1) & o);                  /* both parities at octave 1 */
                    okz_refine_point(&pt, det, o, op);
                    if (k == 1) { pt.x = (float)((xs[xi] - 1) << o); pt.y = (float)((ys[yi] - 1) << o); }      /* the refinement's range */
                    if (k == 2) { pt.x = (float)((xs[xi] + 1) << o); pt.y = (float)((ys[yi] + 1) << o); }
                    okz_orient_point(&pt, lx, ly, o, ow, oh, op, wtab);
                    pt.angle = (float)((2 * k + 1) * 0.78539816339744831);
                    okz_describe_point(&pt, lt, lx, ly, o, ow, oh, op, patsize, idx1, idx2);
                    fkz_refine(&fpt, idet, o, op);
                    fkz_orient(&fpt, ilx, ily, o, ow, oh, op, wtab);
                    fpt.angle = pt.angle;
                    fkz_describe(&fpt, ilt, ilx, ily, o, ow, oh, op, patsize, idx1, idx2);
                    sum += pt.features[k] + fpt.features[60 - k];
                    npts++;
                }
            }
        free(lt); free(lx); free(ly); free(det); free(ilt); free(ilx); free(ily); free(idet);
    }
    printf("  point functions on %ld planted limit / corner keypoints of a %d x %d pyramid, pattern %d\n", 2 * npts, w, h, patsize);
    return sum;
}

int main(void)
{
    if (okz_sizeof_point() != (int)sizeof(Pt) || sizeof(Pt) != 104) { fprintf(stderr, "record layout drifted\n"); return 1; }
    long stage_sum = run_stages(83, 81, 0) + run_stages(83, 81, 1) + run_stages(132, 70, 0) + run_stages(132, 70, 1);
    stage_sum += run_points(265, 245, 10) + run_points(265, 245, 12) + run_points(265, 245, 6);
    (void)stage_sum;
    Prm d = {4, 4, 0.7f, 0.03f, 1.6f, 1, 1.5f, 0.001f, 1, 10, 0};     /* main.cpp:156-166 */
    int total = 0;
    total += run_case(320, 240, &d, 10000, 1);
    total += run_case(211, 173, &d, 10000, 1);                         /* odd sizes, two octaves survive the 80 px rule */
    total += run_case(400, 300, &d, 25, 1);                            /* clamp below the keypoint count */
    total += run_case(324, 200, &d, 10000, 0);                         /* no descriptors */
    Prm u = d; u.upright = 1; u.noctaves = 3; u.max_scale = 3;
    total += run_case(360, 280, &u, 10000, 1);
    Prm c = d; c.diffusivity = 3; c.descriptor_pattern_size = 12; c.soffset = 1.2f;
    total += run_case(300, 220, &c, 10000, 1);
    Prm g = d; g.diffusivity = 0; g.descriptor_pattern_size = 6;
    total += run_case(256, 256, &g, 10000, 1);
    Prm wk = d; wk.diffusivity = 2; wk.reordering = 0;
    total += run_case(288, 200, &wk, 10000, 1);
    /* the integer pipeline far outside its range: two sublevels per octave make FED cycles of ~31 steps at octave 3 (tau up to 50), the
     * 16-bit truncations blow the plane up, sums of squares wrap negative and the conductivity casts see NaN / inf (f2i_sat); found by
     * tests/fuzz_parity.py (seed 5, case 1504) */
    Prm b = d; b.max_scale = 2; b.diffusivity = 3; b.derivative_factor = 1.0f; b.dthreshold = 0.0005f; b.descriptor_pattern_size = 6;
    total += run_case(754, 869, &b, 3000, 1);
    b.diffusivity = 0;
    total += run_case(720, 700, &b, 3000, 1);
    if (total < 200) { fprintf(stderr, "asan_main: the scenes hold too few keypoints (%d) to exercise the tail\n", total); return 1; }
    printf("asan_main: oracle clean\n");
    return 0;
}
