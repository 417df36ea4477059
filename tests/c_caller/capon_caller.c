/* The Capon / Bartlett spectra through the C ABI, from plain C11 (-Wall -Wextra -Werror): nbls_set_capon before nbls_plan, the
 * four fetches behind the pass.  Three elements at (0, 0), (1, 0), (0, 1) km, fs = 20, uniform noise: every refusal of
 * nbls_set_capon and of the plan behind it, zeros before a pass, then per window the two maxima, which must be the arg-max of
 * the fetched maps bit for bit, R Hermitian with a real diagonal, and tables whose first entries are the definition's.
 * Prints one line "W <window> <capon_index> <capon_power %a> <bartlett_index> <bartlett_power %a>" per window for the test
 * that compares with the Python path, then CAPON_CALLER_OK. */
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
#define G 4
#define LS 16
#define HS 8

static int fail(nbls_handle* h, const char* what, int rc) {
    fprintf(stderr, "%s: %d %s\n", what, rc, h ? nbls_last_error(h) : "");
    return 1;
}

static int argmax(const double* p, int n) {
    int best = -1;
    for (int g = 0; g < n; ++g)
        if (p[g] == p[g] && (best < 0 || p[g] > p[best])) best = g;
    return best;
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
    const double grid[G * 2] = {0.0, 0.0, -0.3, 0.2, 0.3, -0.2, 1.0, 1.0};
    const double freq[2] = {1.0, 1.0};
    const int32_t ls[2] = {LS, LS}, hs[2] = {HS, HS};
    double bad[2] = {0.0, INFINITY}, badf[1] = {0.0};
    int32_t bad0[1] = {0}, toolong[1] = {W + 1}, k3[1] = {W - 1};
    const int32_t one[1] = {1};
    nbls_handle* h = NULL;
    int rc;
    if (nbls_device_count() < 1) { fprintf(stderr, "no GPU\n"); return 2; }
    if ((rc = nbls_create(0, &h))) return fail(NULL, "nbls_create", rc);
    if ((rc = nbls_set_trace(h, trace, NCH, NPTS, 20.0))) return fail(h, "nbls_set_trace", rc);
    if ((rc = nbls_set_geometry(h, xij, pair_idx, xpinv, 3))) return fail(h, "nbls_set_geometry", rc);
    static int32_t ci[VL], bi[VL];
    static double cp[VL], bp[VL], cmap[VL * G], bmap[VL * G], R[VL * NCH * NCH * 2], coef[LS * 2], steer[G * NCH * 2];

    if ((rc = nbls_plan(h, 1, NULL, 0, 0, NULL, NULL, 0, winlen, wininc, VL, NULL, 0))) return fail(h, "nbls_plan", rc);
    if ((rc = nbls_execute(h))) return fail(h, "nbls_execute", rc);
    if ((rc = nbls_fetch_capon(h, ci, cp, bi, bp)) != NBLS_ERR_STATE) return fail(h, "nbls_fetch_capon without nbls_set_capon", rc);
    if ((rc = nbls_fetch_capon_maps(h, cmap, bmap)) != NBLS_ERR_STATE) return fail(h, "nbls_fetch_capon_maps without nbls_set_capon", rc);
    if ((rc = nbls_fetch_capon_csdm(h, R)) != NBLS_ERR_STATE) return fail(h, "nbls_fetch_capon_csdm without nbls_set_capon", rc);
    if ((rc = nbls_fetch_capon_tables(h, 0, coef, steer)) != NBLS_ERR_STATE) return fail(h, "nbls_fetch_capon_tables without nbls_set_capon", rc);

    if ((rc = nbls_set_capon(h, grid, NBLS_CAPON_GRID_MAX + 1, freq, ls, hs, 1, 0.01, 0)) != NBLS_ERR_ARG) return fail(h, "G too large", rc);
    if ((rc = nbls_set_capon(h, grid, -1, freq, ls, hs, 1, 0.01, 0)) != NBLS_ERR_ARG) return fail(h, "G negative", rc);
    if ((rc = nbls_set_capon(h, bad, 1, freq, ls, hs, 1, 0.01, 0)) != NBLS_ERR_ARG) return fail(h, "an infinite grid entry", rc);
    if ((rc = nbls_set_capon(h, grid, G, badf, ls, hs, 1, 0.01, 0)) != NBLS_ERR_ARG) return fail(h, "frequency 0", rc);
    if ((rc = nbls_set_capon(h, grid, G, freq, bad0, hs, 1, 0.01, 0)) != NBLS_ERR_ARG) return fail(h, "snapshot length 0", rc);
    if ((rc = nbls_set_capon(h, grid, G, freq, ls, bad0, 1, 0.01, 0)) != NBLS_ERR_ARG) return fail(h, "snapshot hop 0", rc);
    if ((rc = nbls_set_capon(h, grid, G, freq, ls, hs, 1, -1.0, 0)) != NBLS_ERR_ARG) return fail(h, "negative loading", rc);
    if ((rc = nbls_set_capon(h, grid, G, freq, ls, hs, 1, NAN, 0)) != NBLS_ERR_ARG) return fail(h, "NaN loading", rc);
    if ((rc = nbls_set_capon(h, grid, G, freq, ls, hs, 0, 0.01, 0)) != NBLS_ERR_ARG) return fail(h, "no band", rc);
    if ((rc = nbls_plan(h, 1, NULL, 0, 0, NULL, NULL, 0, winlen, wininc, VL, NULL, 0))) return fail(h, "nbls_plan after refusals", rc);
    if ((rc = nbls_fetch_capon(h, ci, cp, bi, bp)) != NBLS_ERR_STATE) return fail(h, "the handle changed under a refusal", rc);

    if ((rc = nbls_set_capon(h, grid, G, freq, ls, hs, 2, 0.01, 0))) return fail(h, "nbls_set_capon", rc);
    if ((rc = nbls_plan(h, 1, NULL, 0, 0, NULL, NULL, 0, winlen, wininc, VL, NULL, 0)) != NBLS_ERR_ARG) return fail(h, "two bands of tables for one", rc);
    if ((rc = nbls_set_capon(h, grid, G, freq, toolong, hs, 1, 0.01, 0))) return fail(h, "nbls_set_capon", rc);
    if ((rc = nbls_plan(h, 1, NULL, 0, 0, NULL, NULL, 0, winlen, wininc, VL, NULL, 0)) != NBLS_ERR_ARG) return fail(h, "a snapshot longer than the window", rc);
    if ((rc = nbls_set_capon(h, grid, G, freq, k3, one, 1, 0.0, 0))) return fail(h, "nbls_set_capon", rc);      /* K = 2 < 3 */
    if ((rc = nbls_plan(h, 1, NULL, 0, 0, NULL, NULL, 0, winlen, wininc, VL, NULL, 0)) != NBLS_ERR_ARG) return fail(h, "singular by construction", rc);

    if ((rc = nbls_set_capon(h, grid, G, freq, ls, hs, 1, 0.01, 0))) return fail(h, "nbls_set_capon", rc);
    if ((rc = nbls_plan(h, 1, NULL, 0, 0, NULL, NULL, 0, winlen, wininc, VL, NULL, 0))) return fail(h, "nbls_plan", rc);
    if ((rc = nbls_fetch_capon_maps(h, cmap, bmap)) != NBLS_ERR_STATE) return fail(h, "maps without NBLS_CAPON_MAPS", rc);
    if ((rc = nbls_fetch_capon_csdm(h, R)) != NBLS_ERR_STATE) return fail(h, "R without NBLS_CAPON_CSDM", rc);
    if ((rc = nbls_set_capon(h, grid, G, freq, ls, hs, 1, 0.01, NBLS_CAPON_MAPS | NBLS_CAPON_CSDM))) return fail(h, "nbls_set_capon", rc);
    if ((rc = nbls_plan(h, 1, NULL, 0, 0, NULL, NULL, 0, winlen, wininc, VL, NULL, 0))) return fail(h, "nbls_plan", rc);
    if ((rc = nbls_set_capon(h, NULL, 0, NULL, NULL, NULL, 0, 0.0, 0))) return fail(h, "nbls_set_capon(off)", rc);   /* the plan keeps its tables */
    if ((rc = nbls_fetch_capon_tables(h, 1, coef, steer)) != NBLS_ERR_ARG) return fail(h, "tables of a band the plan does not have", rc);
    if ((rc = nbls_fetch_capon_tables(h, 0, coef, steer))) return fail(h, "nbls_fetch_capon_tables", rc);
    /* c[0] = (0.5 - 0.5 cos(pi / 16)) (1, 0); a[g][0] = 1; a[0][i] = 1 (s = 0) */
    if (fabs(coef[0] - (0.5 - 0.5 * cos(3.14159265358979323846 / LS))) > 1e-15 || coef[1] != 0.0 || steer[0] != 1.0 || steer[1] != 0.0 ||
        steer[2] != 1.0 || steer[3] != 0.0 || fabs(hypot(steer[(1 * NCH + 1) * 2], steer[(1 * NCH + 1) * 2 + 1]) - 1.0) > 1e-15) {
        fprintf(stderr, "tables\n");
        return 1;
    }
    if ((rc = nbls_fetch_capon(h, ci, cp, bi, bp))) return fail(h, "nbls_fetch_capon before a pass", rc);
    for (int w = 0; w < VL; ++w)
        if (ci[w] != 0 || bi[w] != 0 || cp[w] != 0.0 || bp[w] != 0.0) { fprintf(stderr, "cell %d is not zero before a pass\n", w); return 1; }
    if ((rc = nbls_execute(h))) return fail(h, "nbls_execute", rc);
    if ((rc = nbls_fetch_capon(h, ci, NULL, bi, NULL))) return fail(h, "nbls_fetch_capon", rc);
    if ((rc = nbls_fetch_capon(h, NULL, cp, NULL, bp))) return fail(h, "nbls_fetch_capon", rc);
    if ((rc = nbls_fetch_capon_maps(h, cmap, NULL)) || (rc = nbls_fetch_capon_maps(h, NULL, bmap))) return fail(h, "nbls_fetch_capon_maps", rc);
    if ((rc = nbls_fetch_capon_csdm(h, R))) return fail(h, "nbls_fetch_capon_csdm", rc);
    const int nwin = (NPTS - W + INC - 1) / INC;
    for (int w = 0; w < VL; ++w) {
        if (w >= nwin) {
            if (ci[w] != 0 || bi[w] != 0 || cp[w] != 0.0 || bp[w] != 0.0 || cmap[w * G] != 0.0 || bmap[w * G] != 0.0 || R[w * NCH * NCH * 2] != 0.0) {
                fprintf(stderr, "cell %d beyond nwin is not zero\n", w);
                return 1;
            }
            continue;
        }
        const double* r = R + w * NCH * NCH * 2;
        int herm = 1;
        for (int i = 0; i < NCH; ++i)
            for (int j = 0; j < NCH; ++j)
                if (r[(i * NCH + j) * 2] != r[(j * NCH + i) * 2] || r[(i * NCH + j) * 2 + 1] != -r[(j * NCH + i) * 2 + 1]) herm = 0;
        if (!herm || !(r[0] > 0.0) || ci[w] != argmax(cmap + w * G, G) || bi[w] != argmax(bmap + w * G, G) || ci[w] < 0 ||
            memcmp(&cp[w], &cmap[w * G + ci[w]], sizeof(double)) || memcmp(&bp[w], &bmap[w * G + bi[w]], sizeof(double)) || !(cp[w] > 0.0) ||
            !(bp[w] > 0.0)) {
            fprintf(stderr, "window %d: capon %d %g, bartlett %d %g, hermitian %d\n", w, (int)ci[w], cp[w], (int)bi[w], bp[w], herm);
            return 1;
        }
        printf("W %d %d %a %d %a\n", w, (int)ci[w], cp[w], (int)bi[w], bp[w]);
    }
    nbls_destroy(h);
    printf("CAPON_CALLER_OK %d windows\n", nwin);
    return 0;
}
