// Seeded-lag correlator (nbls_set_lag_seed): the lag pick of every (unit, pair) searched only near the delay
// that the unit's slowness-grid maximum (nbls_set_beam_grid, beam_grid.hip) predicts for the pair.
//
// For the unit of result row r, window w, with g = grid_index[r][w], K = halfwidth[band of r] >= 0, and pair k = (i, j),
// a, b the unit's windows of elements i and j (R and the picks: lag_pick.h):
//     c    = d[g][j] - d[g][i]  (the plan's delay table; 0 if g == -1),   c' = min(max(c, -(W-1)), W-1)
//     lo   = max(c' - K, -(W-1)),  hi = min(c' + K, W-1)                                       (never empty)
//     lag  = hi - np.argmax(cij[W-1-hi : W-lo]),   cij = np.correlate(a, b, 'full') / sqrt(sum a^2 * sum b^2)
//     cmax = R(lag) / sqrt(sum a^2 * sum b^2)
// Quotients are compared by nbls_pick::better_first, the first maximum in np.correlate index order wins (among equal maxima
// the LARGEST lag).  An all-zero range gives lag = hi, cmax = 0; a dead channel lag = hi, cmax = NaN; windows whose sum of
// squares is not finite lag = hi, cmax = NaN.
//
// Two forms (nbls_lag_seed_form names the one a window group takes):
//   1  xcorr_seeded_staged_kernel: one workgroup per unit, one wave per element while staging — the unit's N windows go
//      to LDS once, their sums of squares are taken on the way — then each lane one full dot product over the LDS
//      windows: lanes at consecutive lags read consecutive doubles of the sliding window (conflict-free ds_read_b64) and
//      one broadcast double of the other.  Ranges of up to 63 lags are packed, pair after pair, into chunks of 64 lanes;
//      longer ones go a wave per pair (range_pick).  3..16 elements whose windows fit SEED_LDS_MAX bytes.
//   2  xcorr_seeded_simple_kernel: range_pick_item under the policy Seeded.  Everything else (17..32 elements, windows
//      beyond the fit) and the checker of form 1.
// Both forms take their dot product, order and sums of squares from lag_pick.h, so the two forms give the same bits.
// The order of every sum depends on (elements, W, range, lag) alone: no atomics, nothing depends on the launch's unit
// range.
#include "nbls_internal.h"
#include "wave_ops.h"
#include "lag_pick.h"

namespace {
using namespace nbls_pick;

constexpr size_t SEED_LDS_MAX = 156 * 1024;  // form 1: dynamic LDS up to which a unit's windows are staged (a CU has 160 KiB)

// The range [lo, hi] of pair (ci, cj) of a unit whose grid maximum is g.  K is at most 2 (W-1) here (the full search), so
// nothing overflows: |d| < 2^30.
__device__ inline void seeded_range(const int32_t* delay, int N, int g, int ci, int cj, int W, int K, int& lo, int& hi) {
    int c = g < 0 ? 0 : delay[(int64_t)g * N + cj] - delay[(int64_t)g * N + ci];
    c = min(max(c, -(W - 1)), W - 1);
    lo = max(c - K, -(W - 1));
    hi = min(c + K, W - 1);
}

struct Seeded {
    __device__ static void range(const nbls_range_args& a, int band, int64_t cell, int ci, int cj, int W, int& lo, int& hi) {
        seeded_range(a.delay, a.nchans, a.gindex[cell], ci, cj, W, min(a.halfw[band], 2 * (W - 1)), lo, hi);
    }
    // NaN / Inf samples: the range's first lag
    __device__ static int nonfinite(const double*, const double*, int W, int hi, int) { return W - 1 - hi; }
};

// ------------------------------------------------------------------------------------
// Form 1.  LDS: [N][W] the unit's windows | [N] their sums of squares.  64 N threads: wave wv stages element wv.  Then
//   * S = 2K + 1 <= 64 lags a pair (the half-widths the feature is made for: 37 at K = 18): the P S (pair, lag) items of
//     the unit lie in one row, pair-major, and wave wv takes the chunks wv, wv + N, ... of 64 consecutive items — every
//     lane at work, not S of 64 —, one dot product a lane.  A chunk holds the ends of up to 64 pairs: a segmented shuffle
//     reduce under the total order leaves each pair's best of the chunk in the first lane of its segment, which puts it
//     in the pair's slot of a small static table (a pair lies in at most two chunks); after a barrier thread k combines
//     the slots of pair k and stores.  An item whose lag falls below lo (a range cut by the clamp) takes no part.
//   * longer ranges: wave wv takes the pairs wv, wv + N, ... whole (range_pick), lanes over the lags in trips of 64.
// The dot product of a (pair, lag) and the total order are the same either way: the same bits.
// ------------------------------------------------------------------------------------
constexpr int SEED_MAX_PAIRS = 120;            // 16 elements

__global__ __launch_bounds__(1024) void xcorr_seeded_staged_kernel(nbls_range_args a) {
    extern __shared__ double sm[];
    __shared__ double part_v[2 * SEED_MAX_PAIRS];      // [P][2] a pair's best in its first / second chunk
    __shared__ int part_k[2 * SEED_MAX_PAIRS];         // ... and its np.correlate index (NO_PICK: the pair has no such chunk)
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;
    const int N = a.nchans;
    const int u = a.u0 + blockIdx.x;
    const int band = a.unit_band[u];
    const int w = a.unit_win[u];
    const int W = a.Wb[band];
    const int64_t t0 = (int64_t)w * a.incb[band];
    double* nrm = sm + (size_t)N * W;
    {
        double* ch = sm + (size_t)wv * W;
        const double* src = a.filt + ((int64_t)band * N + wv) * a.npts_pad + t0;
        double q = 0.0;
        for (int n = lane; n < W; n += 64) {
            const double v = src[n];
            ch[n] = v;
            q += v * v;
        }
        for (int off = 32; off > 0; off >>= 1) q += __shfl_xor(q, off, 64);
        if (lane == 0) nrm[wv] = q;
    }
    for (int i = tid; i < 2 * a.npairs; i += 64 * N) { part_v[i] = 0.0; part_k[i] = NO_PICK; }
    __syncthreads();
    const int64_t cell = (int64_t)band * a.vector_len + w;
    const int g = a.gindex[cell];
    const int K = min(a.halfw[band], 2 * (W - 1));
    if (K <= 31) {                                                // (the same for every thread of the workgroup)
        const int S = 2 * K + 1, total = a.npairs * S;
        for (int f0 = wv * 64; f0 < total; f0 += 64 * N) {        // (f0 is the same for every lane of the wave)
            const int f = f0 + lane;
            const int k = f < total ? f / S : -1;
            double cc = 0.0, nrm_ab = 0.0;
            int kk = NO_PICK;
            if (k >= 0) {
                const int ci = a.pair[2 * k], cj = a.pair[2 * k + 1];
                int lo, hi;
                seeded_range(a.delay, N, g, ci, cj, W, K, lo, hi);
                const int lag = hi - (f - k * S);
                nrm_ab = nrm[ci] * nrm[cj];
                if (lag >= lo) {
                    kk = (W - 1) - lag;
                    cc = lag_dot<true>(sm + (size_t)ci * W, sm + (size_t)cj * W, W, kk);
                }
            }
            for (int off = 1; off < 64; off <<= 1) {              // lane l: the best of its pair's lanes l .. l + 2 off - 1
                const double ov = __shfl_down(cc, off, 64);
                const int ok = __shfl_down(kk, off, 64);
                const int okey = __shfl_down(k, off, 64);
                if (lane + off < 64 && okey == k && better_first(ov, ok, cc, kk, nrm_ab)) { cc = ov; kk = ok; }
            }
            const int kprev = __shfl_up(k, 1, 64);
            if (k >= 0 && (lane == 0 || kprev != k)) {            // the first lane of a pair's segment
                const int slot = 2 * k + (f0 / 64 - (k * S) / 64);
                part_v[slot] = cc;
                part_k[slot] = kk;
            }
        }
        __syncthreads();
        if (tid < a.npairs) {
            const int k = tid;
            const int ci = a.pair[2 * k], cj = a.pair[2 * k + 1];
            const double nrm_ab = nrm[ci] * nrm[cj];
            double best = part_v[2 * k];
            int bestk = part_k[2 * k];
            if (better_first(part_v[2 * k + 1], part_k[2 * k + 1], best, bestk, nrm_ab)) { best = part_v[2 * k + 1]; bestk = part_k[2 * k + 1]; }
            if (!nbls_wave::finite_f64(nrm[ci]) || !nbls_wave::finite_f64(nrm[cj])) {      // as range_pick
                int lo, hi;
                seeded_range(a.delay, N, g, ci, cj, W, K, lo, hi);
                bestk = Seeded::nonfinite(nullptr, nullptr, W, hi, lane);
                best = __builtin_nan("");
            }
            store_pick(a.lag, a.cmax, cell * a.npairs + k, W, best, bestk, nrm[ci], nrm[cj]);
        }
        return;
    }
    for (int k = wv; k < a.npairs; k += N) {                      // (k is the same for every lane of the wave)
        const int ci = a.pair[2 * k], cj = a.pair[2 * k + 1];
        int lo, hi;
        seeded_range(a.delay, N, g, ci, cj, W, K, lo, hi);
        double best;
        int bestk;
        range_pick<true, Seeded>(sm + (size_t)ci * W, sm + (size_t)cj * W, W, lo, hi, nrm[ci], nrm[cj], lane, best, bestk);
        if (lane == 0) store_pick(a.lag, a.cmax, cell * a.npairs + k, W, best, bestk, nrm[ci], nrm[cj]);
    }
}

__global__ __launch_bounds__(256) void xcorr_seeded_simple_kernel(nbls_range_args a) { range_pick_item<Seeded>(a); }

}  // namespace

// 1: the staged form (3..16 elements whose windows and sums of squares fit SEED_LDS_MAX), 2: the general form.  The staged
// block has no padding: the half-width and the halo do not enter the fit.
int nbls_lag_seed_form_of(int nelem, int W) {
    if (nelem < 3 || nelem > 16) return 2;
    return (size_t)nelem * ((size_t)W + 1) * sizeof(double) <= SEED_LDS_MAX ? 1 : 2;
}

// The seeded pick of the units [ub, ue) of one window group (windows of gW samples), in the form `form` (1 / 2), behind the
// grid search of the same units (the caller has queued it on the handle's stream).
hipError_t nbls_launch_xcorr_seeded(nbls_handle* h, int64_t ub, int64_t ue, int gW, int form) {
    const int64_t nu = ue - ub;
    if (nu <= 0) return hipSuccess;
    nbls_range_args a = nbls_range_args_of(h, ub, nu);
    a.halfw = h->d_seed;
    a.delay = h->d_grid_delay;
    a.gindex = h->d_grid_index;
    if (form == 1) {
        if (nbls_lag_seed_form_of(h->nelem, gW) != 1) return hipErrorInvalidValue;
        const size_t shm = (size_t)h->nelem * ((size_t)gW + 1) * sizeof(double);
        if (!h->seed_attr_set) {           // once per handle
            const hipError_t e = hipFuncSetAttribute((const void*)xcorr_seeded_staged_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SEED_LDS_MAX);
            if (e != hipSuccess) return e;
            h->seed_attr_set = true;
        }
        hipLaunchKernelGGL(xcorr_seeded_staged_kernel, dim3((unsigned)nu), dim3(64 * h->nelem), shm, h->stream, a);
    } else {
        hipLaunchKernelGGL(xcorr_seeded_simple_kernel, dim3((unsigned)((a.nitems + 3) / 4)), dim3(256), 0, h->stream, a);
    }
    return nbls_finish_lag_pick(h, ub, nu, gW);
}
