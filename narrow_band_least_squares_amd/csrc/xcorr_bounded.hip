// Bounded-lag correlator (nbls_set_lag_limits): the lag pick of every (unit, pair) searched only within the
// pair's physical range |lag| <= L_k, L_k = min(max_lag[k], W-1).
//
// For one unit and pair k = (i, j), a, b the unit's windows of elements i and j (R and the picks: lag_pick.h):
//     lag  = L - np.argmax(cij[W-1-L : W+L]),   cij = np.correlate(a, b, 'full') / sqrt(sum a^2 * sum b^2)
//     cmax = R(lag) / sqrt(sum a^2 * sum b^2)
// Quotients are compared by nbls_pick::better_first, the first maximum in np.correlate index order wins (among equal maxima
// the LARGEST lag).  An all-zero range gives lag = +L, cmax = 0; a dead channel lag = +L, cmax = NaN; windows whose sum of
// squares is not finite cmax = NaN and lag = min(the plain pass's lag, L) (nbls_wave::nonfinite_argmax_clamped).
//
// Two forms (nbls_lag_limit_form names the one a window group takes), both the shared bodies of lag_pick.h under the
// policy Bounded:
//   1  xcorr_bounded_mfma_kernel: mfma_tile_body with the tile loop cut at the largest limit among the wave's pairs and the
//      epilogue masked per pair.  3..16 elements whose zero-padded windows fit a CU's LDS (the fit rule of NBLS_ROUTE_MFMA).
//   2  xcorr_bounded_simple_kernel: range_pick_item over [-L, L].  Everything else (17..32 elements, windows beyond the
//      fit); the slow fallback and the checker of form 1.
// The order of every sum depends on (elements, W, limit table, lag) alone: no atomics, nothing depends on the launch's unit
// range.
#include "nbls_internal.h"
#include "wave_ops.h"
#include "lag_pick.h"

namespace {
using namespace nbls_pick;

struct Bounded {
    // the limit of the pair of two elements, and the largest among the pairs of element wv (wave uniform)
    __device__ static int pair_limit(const nbls_range_args& a, int ci, int cj, int W) { return min(a.limsq[ci * a.nchans + cj], W - 1); }
    __device__ static int wave_limit(const nbls_range_args& a, int wv, int W) {
        int Lw = 0;
        for (int q = 0; q < a.nchans; ++q) {
            const int lq = pair_limit(a, wv, q, W);
            if (q != wv && lq > Lw) Lw = lq;
        }
        return Lw;
    }
    __device__ static void range(const nbls_range_args& a, int, int64_t, int ci, int cj, int W, int& lo, int& hi) {
        hi = pair_limit(a, ci, cj, W);
        lo = -hi;
    }
    __device__ static bool better(double v1, int k1, double v2, int k2, double ss) { return better_first(v1, k1, v2, k2, ss); }
    static constexpr bool WAVE_PER_PAIR = true;
    // NaN / Inf samples: NumPy's semantics on the slice
    __device__ static int nonfinite(const double* xa, const double* xb, int W, int L, int lane) { return nbls_wave::nonfinite_argmax_clamped(xa, xb, W, L, lane); }
};

__global__ __launch_bounds__(1024) void xcorr_bounded_mfma_kernel(nbls_range_args a) {
    extern __shared__ double sm[];
    const int u = a.u0 + blockIdx.x;
    const int band = a.unit_band[u];
    mfma_tile_body<Bounded>(a, band, a.unit_win[u], a.Wb[band], sm);
}

__global__ __launch_bounds__(256) void xcorr_bounded_simple_kernel(nbls_range_args a) { range_pick_item<Bounded>(a); }

}  // namespace

// 0: the plan's ordinary route (the smallest limit of the table reaches W-1: the full search IS the bounded search),
// 1: the matrix-core form, 2: the general form.  The fit rule of form 1 is NBLS_ROUTE_MFMA's (nbls_route_compute).
int nbls_lag_limit_form_of(int nelem, int W, int min_limit) {
    if (min_limit >= W - 1) return 0;
    nbls_route r;
    nbls_route_compute(nbls_route_query{nelem, W, nelem * (nelem - 1) / 2, 1, 2, 2, 0, 0, true}, &r);
    return r.correlator == NBLS_ROUTE_MFMA ? 1 : 2;
}

// The bounded-lag pick of the units [ub, ue) of one window group (windows of gW samples), in the form `form` (1 / 2).
hipError_t nbls_launch_xcorr_bounded(nbls_handle* h, int64_t ub, int64_t ue, int gW, int form) {
    const int64_t nu = ue - ub;
    if (nu <= 0) return hipSuccess;
    nbls_range_args a = nbls_range_args_of(h, ub, nu);
    a.limsq = h->d_limsq;
    if (form == 1) {
        nbls_route r;
        nbls_route_compute(nbls_route_query_of(h, gW, h->nbands, 2, true), &r);
        if (r.correlator != NBLS_ROUTE_MFMA) return hipErrorInvalidValue;
        const size_t shm = (size_t)r.lds_dyn[NBLS_ROUTE_GENERAL];
        a.S = r.S;
        a.PF = r.PFB;
        a.CS = r.CSB;
        const hipError_t e = hipFuncSetAttribute((const void*)xcorr_bounded_mfma_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(xcorr_bounded_mfma_kernel, dim3((unsigned)nu), dim3(64 * h->nelem), shm, h->stream, a);
    } else {
        hipLaunchKernelGGL(xcorr_bounded_simple_kernel, dim3((unsigned)((a.nitems + 3) / 4)), dim3(256), 0, h->stream, a);
    }
    return nbls_finish_lag_pick(h, ub, nu, gW);
}
