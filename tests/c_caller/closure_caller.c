/* The closure results through the C ABI, from plain C11 (-Wall -Wextra -Werror): nbls_set_closure before nbls_plan,
 * nbls_fetch_closure / nbls_est_fetch_closure behind the pass.  Four channels of one noise series, channel i delayed by
 * D[i] whole samples: every lag is D[j] - D[i], the table closes and all three outputs are exactly 0.0 in every window.
 * A plan without nbls_set_closure must refuse both fetches with NBLS_ERR_STATE.  Prints CLOSURE_CALLER_OK. */
#include <stdio.h>
#include <stdlib.h>
#include "nbls.h"

#define NCH 4
#define NPTS 401
#define W 65
#define INC 32
#define VL 16

static int fail(nbls_handle* h, const char* what, int rc) {
    fprintf(stderr, "%s: %d %s\n", what, rc, h ? nbls_last_error(h) : "");
    return 1;
}

int main(void) {
    static double trace[NCH * NPTS];
    static double series[NPTS + 8];
    const int D[NCH] = {0, 3, 1, 5};
    unsigned int s = 12345u;
    for (int t = 0; t < NPTS + 8; ++t) {
        s = s * 1664525u + 1013904223u;
        series[t] = (double)(s >> 8) / 8388608.0 - 1.0;
    }
    for (int c = 0; c < NCH; ++c)
        for (int t = 0; t < NPTS; ++t) trace[c * NPTS + t] = series[t + 8 - D[c]];
    /* elements (0, 0), (1, 0), (0, 1), (1, 1) km; xij = r_i - r_j in list order; xpinv = (X^T X)^-1 X^T, X^T X = 4 I */
    const double xij[6 * 2] = {-1.0, 0.0, 0.0, -1.0, -1.0, -1.0, 1.0, -1.0, 0.0, -1.0, -1.0, 0.0};
    const int32_t pair_idx[6 * 2] = {0, 1, 0, 2, 0, 3, 1, 2, 1, 3, 2, 3};
    double xpinv[2 * 6];
    for (int k = 0; k < 6; ++k) { xpinv[k] = xij[2 * k] / 4.0; xpinv[6 + k] = xij[2 * k + 1] / 4.0; }
    const int32_t winlen[1] = {W}, wininc[1] = {INC};
    nbls_handle* h = NULL;
    int rc;
    if (nbls_device_count() < 1) { fprintf(stderr, "no GPU\n"); return 2; }
    if ((rc = nbls_create(0, &h))) return fail(NULL, "nbls_create", rc);
    if ((rc = nbls_set_trace(h, trace, NCH, NPTS, 20.0))) return fail(h, "nbls_set_trace", rc);
    if ((rc = nbls_set_geometry(h, xij, pair_idx, xpinv, 6))) return fail(h, "nbls_set_geometry", rc);
    static double cons[VL], cmax[VL], el[VL * NCH];

    if ((rc = nbls_plan(h, 1, NULL, 0, 0, NULL, NULL, 0, winlen, wininc, VL, NULL, 0))) return fail(h, "nbls_plan", rc);
    if ((rc = nbls_execute(h))) return fail(h, "nbls_execute", rc);
    if ((rc = nbls_fetch_closure(h, cons, cmax, el)) != NBLS_ERR_STATE) return fail(h, "nbls_fetch_closure without nbls_set_closure", rc);
    if ((rc = nbls_est_fetch_closure(h, 0, cons, NULL, NULL)) != NBLS_ERR_STATE)
        return fail(h, "nbls_est_fetch_closure without nbls_set_closure", rc);

    if ((rc = nbls_set_closure(h, 1))) return fail(h, "nbls_set_closure", rc);
    if ((rc = nbls_plan(h, 1, NULL, 0, 0, NULL, NULL, 0, winlen, wininc, VL, NULL, 0))) return fail(h, "nbls_plan", rc);
    for (int w = 0; w < VL; ++w) { cons[w] = cmax[w] = -1.0; for (int m = 0; m < NCH; ++m) el[w * NCH + m] = -1.0; }
    if ((rc = nbls_execute(h))) return fail(h, "nbls_execute", rc);
    if ((rc = nbls_fetch_closure(h, cons, NULL, NULL))) return fail(h, "nbls_fetch_closure", rc);
    if ((rc = nbls_fetch_closure(h, NULL, cmax, el))) return fail(h, "nbls_fetch_closure", rc);
    static int32_t lag[VL * 6];
    if ((rc = nbls_fetch(h, NULL, NULL, NULL, NULL, NULL, lag, NULL, NULL, NULL))) return fail(h, "nbls_fetch", rc);
    const int nwin = (NPTS - W + INC - 1) / INC;
    for (int w = 0; w < VL; ++w) {
        int bad = cons[w] != 0.0 || cmax[w] != 0.0;
        for (int m = 0; m < NCH; ++m) bad |= el[w * NCH + m] != 0.0;
        if (w < nwin)
            for (int k = 0; k < 6; ++k) bad |= lag[w * 6 + k] != D[pair_idx[2 * k + 1]] - D[pair_idx[2 * k]];
        if (bad) { fprintf(stderr, "window %d: consistency %g closure_max %g\n", w, cons[w], cmax[w]); return 1; }
    }
    if ((rc = nbls_est_fetch_closure(h, 1, cons, cmax, el)) != NBLS_ERR_ARG) return fail(h, "nbls_est_fetch_closure of estimator 1", rc);
    nbls_destroy(h);
    printf("CLOSURE_CALLER_OK %d windows\n", nwin);
    return 0;
}
