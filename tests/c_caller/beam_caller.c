/* The beam results through the C ABI, from plain C11 (-Wall -Wextra -Werror): nbls_set_beam before nbls_plan,
 * nbls_fetch_beam behind the pass.  Three identical channels: every lag is 0, the solved slowness is 0, every delay is
 * 0, the beam is 3 x[t] — beam_power is the window's mean square and the channels line up exactly, so fstat is +inf or
 * (S_b and 3 S_t rounded apart) huge.  A plan without nbls_set_beam must refuse the fetch with NBLS_ERR_STATE.
 * Prints BEAM_CALLER_OK. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include "nbls.h"

#define NCH 3
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
    unsigned int s = 12345u;
    for (int t = 0; t < NPTS; ++t) {
        s = s * 1664525u + 1013904223u;
        const double v = (double)(s >> 8) / 8388608.0 - 1.0;
        for (int c = 0; c < NCH; ++c) trace[c * NPTS + t] = v;
    }
    /* elements (0, 0), (1, 0), (0, 1) km; xij = r_i - r_j, xpinv = (X^T X)^-1 X^T */
    const double xij[3 * 2] = {-1.0, 0.0, 0.0, -1.0, 1.0, -1.0};
    const int32_t pair_idx[3 * 2] = {0, 1, 0, 2, 1, 2};
    const double xpinv[2 * 3] = {-2.0 / 3.0, -1.0 / 3.0, 1.0 / 3.0, -1.0 / 3.0, -2.0 / 3.0, -1.0 / 3.0};
    const int32_t winlen[1] = {W}, wininc[1] = {INC};
    nbls_handle* h = NULL;
    int rc;
    if (nbls_device_count() < 1) { fprintf(stderr, "no GPU\n"); return 2; }
    if ((rc = nbls_create(0, &h))) return fail(NULL, "nbls_create", rc);
    if ((rc = nbls_set_trace(h, trace, NCH, NPTS, 20.0))) return fail(h, "nbls_set_trace", rc);
    if ((rc = nbls_set_geometry(h, xij, pair_idx, xpinv, 3))) return fail(h, "nbls_set_geometry", rc);
    static double power[VL], fstat[VL];

    if ((rc = nbls_plan(h, 1, NULL, 0, 0, NULL, NULL, 0, winlen, wininc, VL, NULL, 0))) return fail(h, "nbls_plan", rc);
    if ((rc = nbls_execute(h))) return fail(h, "nbls_execute", rc);
    if ((rc = nbls_fetch_beam(h, power, fstat)) != NBLS_ERR_STATE) return fail(h, "nbls_fetch_beam without nbls_set_beam", rc);

    if ((rc = nbls_set_beam(h, 1))) return fail(h, "nbls_set_beam", rc);
    if ((rc = nbls_plan(h, 1, NULL, 0, 0, NULL, NULL, 0, winlen, wininc, VL, NULL, 0))) return fail(h, "nbls_plan", rc);
    if ((rc = nbls_execute(h))) return fail(h, "nbls_execute", rc);
    if ((rc = nbls_fetch_beam(h, power, NULL))) return fail(h, "nbls_fetch_beam", rc);
    if ((rc = nbls_fetch_beam(h, NULL, fstat))) return fail(h, "nbls_fetch_beam", rc);
    const int nwin = (NPTS - W + INC - 1) / INC;
    for (int w = 0; w < VL; ++w) {
        if (w >= nwin) {
            if (power[w] != 0.0 || fstat[w] != 0.0) { fprintf(stderr, "cell %d beyond nwin is not zero\n", w); return 1; }
            continue;
        }
        double ms = 0.0;
        for (int t = 0; t < W; ++t) ms += trace[w * INC + t] * trace[w * INC + t];
        ms /= W;
        if (fabs(power[w] - ms) > 1e-12 * ms || !(fstat[w] > 1e6)) {
            fprintf(stderr, "window %d: beam_power %.17g (mean square %.17g), fstat %g\n", w, power[w], ms, fstat[w]);
            return 1;
        }
    }
    nbls_destroy(h);
    printf("BEAM_CALLER_OK %d windows\n", nwin);
    return 0;
}
