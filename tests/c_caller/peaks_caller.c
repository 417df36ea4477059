/* The peak request of the Capon / Bartlett spectra through the C ABI, from plain C11 (-Wall -Wextra -Werror):
 * nbls_set_capon_peaks beside nbls_set_capon before nbls_plan, nbls_fetch_capon_peaks behind the pass.  Three elements at
 * (0, 0), (1, 0), (0, 1) km, fs = 20, uniform noise, a 3 x 3 lattice of slowness vectors: every refusal of
 * nbls_set_capon_peaks and of the plan behind it, then per window rank 0 must be nbls_fetch_capon's arg-max bit for bit, the
 * ranks must descend, and the count must cover them.  Prints one line
 * "P <window> <which> <count> <index0> <power0 %a> <off00 %a> <off01 %a> <index1> <power1 %a>" per window and spectrum for the
 * test that compares with the Python path, then PEAKS_CALLER_OK. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "nbls.h"

#define NCH 3
#define NPTS 401
#define W 65
#define INC 32
#define VL 16
#define G 9
#define K 2
#define LS 16
#define HS 8

static int fail(nbls_handle* h, const char* what, int rc) {
    fprintf(stderr, "%s: %d %s\n", what, rc, h ? nbls_last_error(h) : "");
    return 1;
}

int main(void) {
    static double trace[NCH * NPTS];
    unsigned int s = 12345u;
    for (int t = 0; t < NCH * NPTS; ++t) {
        s = s * 1664525u + 1013904223u;
        trace[t] = (double)(s >> 8) / 8388608.0 - 1.0;
    }
    const double xij[3 * 2] = {-1.0, 0.0, 0.0, -1.0, 1.0, -1.0};
    const int32_t pair_idx[3 * 2] = {0, 1, 0, 2, 1, 2};
    const double xpinv[2 * 3] = {-2.0 / 3.0, -1.0 / 3.0, 1.0 / 3.0, -1.0 / 3.0, -2.0 / 3.0, -1.0 / 3.0};
    const int32_t winlen[1] = {W}, wininc[1] = {INC};
    double grid[G * 2];
    int32_t cell[G * 2], twice[G * 2], far[G * 2], neg[G * 2];
    for (int g = 0; g < G; ++g) {
        cell[2 * g] = g / 3; cell[2 * g + 1] = g % 3;
        grid[2 * g] = 0.3 * (g / 3 - 1); grid[2 * g + 1] = 0.3 * (g % 3 - 1);
    }
    memcpy(twice, cell, sizeof cell); twice[2 * 8] = 0; twice[2 * 8 + 1] = 0;
    memcpy(far, cell, sizeof cell); far[3] = 32768;
    memcpy(neg, cell, sizeof cell); neg[4] = -1;
    const double freq[1] = {1.0};
    const int32_t ls[1] = {LS}, hs[1] = {HS};
    nbls_handle* h = NULL;
    int rc;
    if (nbls_device_count() < 1) { fprintf(stderr, "no GPU\n"); return 2; }
    if ((rc = nbls_create(0, &h))) return fail(NULL, "nbls_create", rc);
    if ((rc = nbls_set_trace(h, trace, NCH, NPTS, 20.0))) return fail(h, "nbls_set_trace", rc);
    if ((rc = nbls_set_geometry(h, xij, pair_idx, xpinv, 3))) return fail(h, "nbls_set_geometry", rc);
    static int32_t ci[VL], bi[VL], cnt[VL], idx[VL * K];
    static double cp[VL], bp[VL], pw[VL * K], off[VL * K * 2];

    if ((rc = nbls_set_capon_peaks(h, cell, G, NBLS_CAPON_PEAKS_MAX + 1, 0.25)) != NBLS_ERR_ARG) return fail(h, "K too large", rc);
    if ((rc = nbls_set_capon_peaks(h, cell, G, -1, 0.25)) != NBLS_ERR_ARG) return fail(h, "K negative", rc);
    if ((rc = nbls_set_capon_peaks(h, cell, G, K, -0.1)) != NBLS_ERR_ARG) return fail(h, "floor below 0", rc);
    if ((rc = nbls_set_capon_peaks(h, cell, G, K, 1.5)) != NBLS_ERR_ARG) return fail(h, "floor above 1", rc);
    if ((rc = nbls_set_capon_peaks(h, cell, G, K, NAN)) != NBLS_ERR_ARG) return fail(h, "NaN floor", rc);
    if ((rc = nbls_set_capon_peaks(h, far, G, K, 0.25)) != NBLS_ERR_ARG) return fail(h, "a coordinate of 32768", rc);
    if ((rc = nbls_set_capon_peaks(h, neg, G, K, 0.25)) != NBLS_ERR_ARG) return fail(h, "a negative coordinate", rc);
    if ((rc = nbls_set_capon_peaks(h, twice, G, K, 0.25)) != NBLS_ERR_ARG) return fail(h, "two equal cells", rc);
    /* the handle is unchanged: a plan with spectra and without peaks */
    if ((rc = nbls_set_capon(h, grid, G, freq, ls, hs, 1, 0.01, 0))) return fail(h, "nbls_set_capon", rc);
    if ((rc = nbls_plan(h, 1, NULL, 0, 0, NULL, NULL, 0, winlen, wininc, VL, NULL, 0))) return fail(h, "nbls_plan after refusals", rc);
    if ((rc = nbls_fetch_capon_peaks(h, 0, cnt, idx, pw, off)) != NBLS_ERR_STATE) return fail(h, "peaks without nbls_set_capon_peaks", rc);

    if ((rc = nbls_set_capon_peaks(h, cell, G - 1, K, 0.25))) return fail(h, "nbls_set_capon_peaks", rc);
    if ((rc = nbls_plan(h, 1, NULL, 0, 0, NULL, NULL, 0, winlen, wininc, VL, NULL, 0)) != NBLS_ERR_ARG) return fail(h, "another G than the spectra's", rc);
    if ((rc = nbls_set_capon_peaks(h, cell, G, K, 0.0))) return fail(h, "nbls_set_capon_peaks", rc);
    if ((rc = nbls_set_capon(h, NULL, 0, NULL, NULL, NULL, 0, 0.0, 0))) return fail(h, "nbls_set_capon(off)", rc);
    if ((rc = nbls_plan(h, 1, NULL, 0, 0, NULL, NULL, 0, winlen, wininc, VL, NULL, 0)) != NBLS_ERR_ARG) return fail(h, "peaks without spectra", rc);
    if ((rc = nbls_set_capon_peaks(h, NULL, 0, 0, 0.0))) return fail(h, "nbls_set_capon_peaks(off)", rc);
    if ((rc = nbls_plan(h, 1, NULL, 0, 0, NULL, NULL, 0, winlen, wininc, VL, NULL, 0))) return fail(h, "the plain plan", rc);

    if ((rc = nbls_set_capon(h, grid, G, freq, ls, hs, 1, 0.01, 0))) return fail(h, "nbls_set_capon", rc);
    if ((rc = nbls_set_capon_peaks(h, cell, G, K, 0.0))) return fail(h, "nbls_set_capon_peaks", rc);
    if ((rc = nbls_plan(h, 1, NULL, 0, 0, NULL, NULL, 0, winlen, wininc, VL, NULL, 0))) return fail(h, "nbls_plan", rc);
    if ((rc = nbls_set_capon_peaks(h, NULL, 0, 0, 0.0))) return fail(h, "nbls_set_capon_peaks(off)", rc);   /* the plan keeps its request */
    if ((rc = nbls_fetch_capon_peaks(h, 2, cnt, idx, pw, off)) != NBLS_ERR_ARG) return fail(h, "which = 2", rc);
    if ((rc = nbls_fetch_capon_peaks(h, 0, cnt, idx, pw, off))) return fail(h, "nbls_fetch_capon_peaks before a pass", rc);
    for (int w = 0; w < VL; ++w)
        if (cnt[w] != 0 || idx[w * K] != 0 || pw[w * K] != 0.0) { fprintf(stderr, "cell %d is not zero before a pass\n", w); return 1; }
    if ((rc = nbls_execute(h))) return fail(h, "nbls_execute", rc);
    if ((rc = nbls_fetch_capon(h, ci, cp, bi, bp))) return fail(h, "nbls_fetch_capon", rc);
    const int nwin = (NPTS - W + INC - 1) / INC;
    for (int which = 0; which < 2; ++which) {
        if ((rc = nbls_fetch_capon_peaks(h, which, cnt, NULL, NULL, NULL))) return fail(h, "nbls_fetch_capon_peaks", rc);
        if ((rc = nbls_fetch_capon_peaks(h, which, NULL, idx, pw, off))) return fail(h, "nbls_fetch_capon_peaks", rc);
        const int32_t* i0 = which ? bi : ci;
        const double* p0 = which ? bp : cp;
        for (int w = 0; w < VL; ++w) {
            const int32_t* ix = idx + w * K;
            const double* p = pw + w * K;
            const double* o = off + w * K * 2;
            if (w >= nwin) {
                if (cnt[w] != 0 || ix[0] != 0 || ix[1] != 0 || p[0] != 0.0 || o[0] != 0.0) { fprintf(stderr, "cell %d beyond nwin is not zero\n", w); return 1; }
                continue;
            }
            int ok = cnt[w] >= 1 && ix[0] == i0[w] && !memcmp(&p[0], &p0[w], sizeof(double)) && fabs(o[0]) <= 0.5 && fabs(o[1]) <= 0.5;
            if (cnt[w] >= 2) ok = ok && ix[1] >= 0 && ix[1] < G && ix[1] != ix[0] && (p[1] < p[0] || (p[1] == p[0] && ix[1] > ix[0]));
            else ok = ok && ix[1] == -1 && p[1] != p[1] && o[2] != o[2] && o[3] != o[3];
            if (!ok) {
                fprintf(stderr, "window %d spectrum %d: count %d, ranks %d %g, %d %g; arg-max %d %g\n", w, which, (int)cnt[w], (int)ix[0], p[0],
                        (int)ix[1], p[1], (int)i0[w], p0[w]);
                return 1;
            }
            printf("P %d %d %d %d %a %a %a %d %a\n", w, which, (int)cnt[w], (int)ix[0], p[0], o[0], o[1], (int)ix[1], p[1]);
        }
    }
    nbls_destroy(h);
    printf("PEAKS_CALLER_OK %d windows\n", nwin);
    return 0;
}
