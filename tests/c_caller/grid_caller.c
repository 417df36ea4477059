/* The slowness-grid search through the C ABI, from plain C11 (-Wall -Wextra -Werror): nbls_set_beam_grid before nbls_plan,
 * the three fetches behind the pass.  Three elements at (0, 0), (1, 0), (0, 1) km, fs = 20: channel i is channel 0 read
 * d_i = 0, -6, 4 samples away, the delays of the slowness (0.3, -0.2) s/km — grid point 2 of 4, and grid point 3 repeats it.
 * The maximum must sit on point 2 (the lower index of the two), with the beam power of a lined-up beam and an F-statistic
 * that is +inf or huge; the map's entry there is that F bit for bit.  Bad grids and a plan without a grid are refused.
 * Prints GRID_CALLER_OK. */
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

static int fail(nbls_handle* h, const char* what, int rc) {
    fprintf(stderr, "%s: %d %s\n", what, rc, h ? nbls_last_error(h) : "");
    return 1;
}

int main(void) {
    static double base[NPTS + 32], trace[NCH * NPTS];
    const int32_t delay[NCH] = {0, -6, 4};
    unsigned int s = 12345u;
    for (int t = 0; t < NPTS + 32; ++t) {
        s = s * 1664525u + 1013904223u;
        base[t] = (double)(s >> 8) / 8388608.0 - 1.0;
    }
    /* x_i[n] = base[16 + n - d_i]: reading element i at +d_i gives base[16 + n] on every channel */
    for (int c = 0; c < NCH; ++c)
        for (int t = 0; t < NPTS; ++t) trace[c * NPTS + t] = base[16 + t - delay[c]];
    /* xij = r_i - r_j, xpinv = (X^T X)^-1 X^T */
    const double xij[3 * 2] = {-1.0, 0.0, 0.0, -1.0, 1.0, -1.0};
    const int32_t pair_idx[3 * 2] = {0, 1, 0, 2, 1, 2};
    const double xpinv[2 * 3] = {-2.0 / 3.0, -1.0 / 3.0, 1.0 / 3.0, -1.0 / 3.0, -2.0 / 3.0, -1.0 / 3.0};
    const int32_t winlen[1] = {W}, wininc[1] = {INC};
    /* fs xij . s = 20 * (-0.3) = -6 and 20 * 0.2 = 4 at s = (0.3, -0.2) */
    const double grid[G * 2] = {0.0, 0.0, -0.3, 0.2, 0.3, -0.2, 0.3, -0.2};
    double bad[2] = {0.0, 0.0};
    nbls_handle* h = NULL;
    int rc;
    if (nbls_beam_grid_lds_bytes(NCH, W, 6) != NCH * (W + 12) * 8 || nbls_beam_grid_lds_bytes(NCH, W, 100000) != 0 ||
        nbls_beam_grid_lds_bytes(0, W, 0) != NBLS_ERR_ARG) { fprintf(stderr, "nbls_beam_grid_lds_bytes\n"); return 1; }
    if (nbls_device_count() < 1) { fprintf(stderr, "no GPU\n"); return 2; }
    if ((rc = nbls_create(0, &h))) return fail(NULL, "nbls_create", rc);
    if ((rc = nbls_set_trace(h, trace, NCH, NPTS, 20.0))) return fail(h, "nbls_set_trace", rc);
    if ((rc = nbls_set_geometry(h, xij, pair_idx, xpinv, 3))) return fail(h, "nbls_set_geometry", rc);
    static int32_t index[VL], dtab[G * NCH];
    static double fstat[VL], power[VL], map[VL * G];

    if ((rc = nbls_plan(h, 1, NULL, 0, 0, NULL, NULL, 0, winlen, wininc, VL, NULL, 0))) return fail(h, "nbls_plan", rc);
    if ((rc = nbls_execute(h))) return fail(h, "nbls_execute", rc);
    if ((rc = nbls_fetch_beam_grid(h, index, fstat, power)) != NBLS_ERR_STATE) return fail(h, "nbls_fetch_beam_grid without a grid", rc);
    if ((rc = nbls_fetch_beam_grid_map(h, map)) != NBLS_ERR_STATE) return fail(h, "nbls_fetch_beam_grid_map without a grid", rc);
    if ((rc = nbls_fetch_beam_grid_delays(h, dtab)) != NBLS_ERR_STATE) return fail(h, "nbls_fetch_beam_grid_delays without a grid", rc);

    if ((rc = nbls_set_beam_grid(h, grid, 0, 0)) != NBLS_ERR_ARG) return fail(h, "nbls_set_beam_grid with G = 0", rc);
    if ((rc = nbls_set_beam_grid(h, grid, NBLS_BEAM_GRID_MAX + 1, 0)) != NBLS_ERR_ARG) return fail(h, "nbls_set_beam_grid with G too large", rc);
    bad[1] = INFINITY;
    if ((rc = nbls_set_beam_grid(h, bad, 1, 0)) != NBLS_ERR_ARG) return fail(h, "nbls_set_beam_grid with an infinite entry", rc);
    bad[1] = 1e9;                            /* a delay of 2e10 samples */
    if ((rc = nbls_set_beam_grid(h, bad, 1, 0))) return fail(h, "nbls_set_beam_grid", rc);
    if ((rc = nbls_plan(h, 1, NULL, 0, 0, NULL, NULL, 0, winlen, wininc, VL, NULL, 0)) != NBLS_ERR_ARG) return fail(h, "nbls_plan with a delay of 2^30", rc);

    if ((rc = nbls_set_beam_grid(h, grid, G, 0))) return fail(h, "nbls_set_beam_grid", rc);
    if ((rc = nbls_plan(h, 1, NULL, 0, 0, NULL, NULL, 0, winlen, wininc, VL, NULL, 0))) return fail(h, "nbls_plan", rc);
    if ((rc = nbls_fetch_beam_grid_map(h, map)) != NBLS_ERR_STATE) return fail(h, "nbls_fetch_beam_grid_map without want_map", rc);
    if ((rc = nbls_set_beam_grid(h, grid, G, 1))) return fail(h, "nbls_set_beam_grid", rc);
    if ((rc = nbls_plan(h, 1, NULL, 0, 0, NULL, NULL, 0, winlen, wininc, VL, NULL, 0))) return fail(h, "nbls_plan", rc);
    if ((rc = nbls_set_beam_grid(h, NULL, 0, 0))) return fail(h, "nbls_set_beam_grid(NULL)", rc);     /* the plan keeps its grid */
    if ((rc = nbls_fetch_beam_grid_delays(h, dtab))) return fail(h, "nbls_fetch_beam_grid_delays", rc);
    const int32_t want[G * NCH] = {0, 0, 0, 0, 6, -4, 0, -6, 4, 0, -6, 4};
    if (memcmp(dtab, want, sizeof want)) { fprintf(stderr, "delay table\n"); return 1; }
    if ((rc = nbls_fetch_beam_grid(h, index, fstat, power))) return fail(h, "nbls_fetch_beam_grid before a pass", rc);
    for (int w = 0; w < VL; ++w)
        if (index[w] != 0 || fstat[w] != 0.0 || power[w] != 0.0) { fprintf(stderr, "cell %d is not zero before a pass\n", w); return 1; }
    if ((rc = nbls_execute(h))) return fail(h, "nbls_execute", rc);
    if ((rc = nbls_fetch_beam_grid(h, index, NULL, NULL))) return fail(h, "nbls_fetch_beam_grid", rc);
    if ((rc = nbls_fetch_beam_grid(h, NULL, fstat, power))) return fail(h, "nbls_fetch_beam_grid", rc);
    if ((rc = nbls_fetch_beam_grid_map(h, map))) return fail(h, "nbls_fetch_beam_grid_map", rc);
    const int nwin = (NPTS - W + INC - 1) / INC;
    for (int w = 0; w < VL; ++w) {
        if (w >= nwin) {
            if (index[w] != 0 || power[w] != 0.0 || fstat[w] != 0.0 || map[w * G] != 0.0) { fprintf(stderr, "cell %d beyond nwin is not zero\n", w); return 1; }
            continue;
        }
        if (w == 0 || w * INC + W + 6 > NPTS) continue;       /* windows that read outside the trace: zeros there, no exact line-up */
        double ms = 0.0;
        for (int t = 0; t < W; ++t) ms += base[16 + w * INC + t] * base[16 + w * INC + t];
        ms /= W;
        if (index[w] != 2 || fabs(power[w] - ms) > 1e-12 * ms || !(fstat[w] > 1e6) ||
            memcmp(&fstat[w], &map[w * G + 2], sizeof(double)) || memcmp(&map[w * G + 2], &map[w * G + 3], sizeof(double)) ||
            !(map[w * G] < 100.0) || !(map[w * G + 1] < 100.0)) {
            fprintf(stderr, "window %d: index %d, power %.17g (mean square %.17g), fstat %g, map %g %g %g %g\n", w, (int)index[w],
                    power[w], ms, fstat[w], map[w * G], map[w * G + 1], map[w * G + 2], map[w * G + 3]);
            return 1;
        }
    }
    nbls_destroy(h);
    printf("GRID_CALLER_OK %d windows\n", nwin);
    return 0;
}
