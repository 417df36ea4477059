// Seeded-lag correlator (nbls_set_lag_seed): the lag pick of every (unit, pair) searched only near the delay
// that the unit's slowness-grid maximum (nbls_set_beam_grid, beam_grid.hip) predicts for the pair.
//
// For the unit of result row r, window w, with g = grid_index[r][w], K = halfwidth[band of r] >= 0, and pair k = (i, j),
// a, b the unit's windows of elements i and j, R(m) = sum_n a[n-m] b[n] (indices inside [0, W)) =
// np.correlate(a, b, 'full')[W-1-m]:
//     c    = d[g][j] - d[g][i]  (the plan's delay table; 0 if g == -1),   c' = min(max(c, -(W-1)), W-1)
//     lo   = max(c' - K, -(W-1)),  hi = min(c' + K, W-1)                                       (never empty)
//     lag  = hi - np.argmax(cij[W-1-hi : W-lo]),   cij = np.correlate(a, b, 'full') / sqrt(sum a^2 * sum b^2)
//     cmax = R(lag) / sqrt(sum a^2 * sum b^2)
// Quotients are compared by nbls_wave::better_q with "no lag seen yet" as the least element, the first maximum in
// np.correlate index order wins (among equal maxima the LARGEST lag).  An all-zero range gives lag = hi, cmax = 0; a dead
// channel lag = hi, cmax = NaN; windows whose sum of squares is not finite lag = hi, cmax = NaN.
//
// Two forms (nbls_lag_seed_form names the one a window group takes):
//   1  xcorr_seeded_staged_kernel: one workgroup per unit, one wave per element while staging — the unit's N windows go
//      to LDS once, their sums of squares are taken on the way — then each lane one full dot product over the LDS
//      windows: lanes at consecutive lags read consecutive doubles of the sliding window (conflict-free ds_read_b64) and
//      one broadcast double of the other.  Ranges of up to 63 lags are packed, pair after pair, into chunks of 64 lanes;
//      longer ones go a wave per pair, lanes over the lags hi .. lo in trips of 64.  3..16 elements whose windows fit
//      SEED_LDS_MAX bytes.
//   2  xcorr_seeded_simple_kernel: a wave per (unit, pair), four per workgroup, the same lanes-over-lags loop reading the
//      windows from global memory (L2).  Everything else (17..32 elements, windows beyond the fit) and the checker of form 1.
// Both forms run ONE pick routine (seeded_pick): a lane's dot product is the four-accumulator ascending-n sum of
// xcorr_simple_kernel, the sums of squares are a 64-lane strided sum and one xor tree, so the two forms give the same bits.
// The order of every sum depends on (elements, W, range, lag) alone: no atomics, nothing depends on the launch's unit
// range.  Picks are written with plain vector stores.
#include "nbls_internal.h"
#include "wave_ops.h"

namespace {

struct SdArgs {
    const double* filt;       // [B][N][npts_pad]
    int64_t npts_pad;
    int nchans;               // array elements N
    int npairs;
    const int32_t* pair;      // [P][2]
    const int32_t* halfw;     // [B] half-width K of every result row
    const int32_t* delay;     // [G][N] the plan's delay table (beam_grid.hip)
    const int32_t* gindex;    // [B][VL] the grid maximum of every unit, -1: none
    const int32_t* Wb;        // [B]
    const int32_t* incb;      // [B]
    const int32_t* unit_band; // [U]
    const int32_t* unit_win;  // [U]
    int vector_len;
    int32_t* lag;             // [B][VL][P]
    double* cmax;             // [B][VL][P]
    int u0;                   // first unit of this launch
    int64_t nitems;           // form 2: (unit, pair) items of this launch
};

constexpr size_t SEED_LDS_MAX = 156 * 1024;  // form 1: dynamic LDS up to which a unit's windows are staged (a CU has 160 KiB)
constexpr int NO_PICK = 0x7fffffff;          // index of a running maximum that has seen no lag yet
// nbls_wave::better_q with "no lag yet" as the least element whatever the values are (xcorr_bounded.hip: on a dead channel
// the first lag of the range has to win against the initial -inf).
__device__ inline bool better_s(double v1, int k1, double v2, int k2, double ss) {
    if (k1 == NO_PICK) return false;
    if (k2 == NO_PICK) return true;
    return nbls_wave::better_q(v1, k1, v2, k2, ss);
}

// The range [lo, hi] of pair (ci, cj) of a unit whose grid maximum is g.  K is at most 2 (W-1) here (the full search), so
// nothing overflows: |d| < 2^30.
__device__ inline void seeded_range(const int32_t* delay, int N, int g, int ci, int cj, int W, int K, int& lo, int& hi) {
    int c = g < 0 ? 0 : delay[(int64_t)g * N + cj] - delay[(int64_t)g * N + ci];
    c = min(max(c, -(W - 1)), W - 1);
    lo = max(c - K, -(W - 1));
    hi = min(c + K, W - 1);
}

// A read of a window: LDS form — volatile, so that every read stays one ds_read_b64 (256 B/clk/CU; merged in pairs into
// ds_read2_b64 they run at half that rate, as beam_grid.hip found for its own loop) — or global memory.
typedef const volatile __attribute__((address_space(3))) double* lds_f64;
template <bool LDS>
__device__ inline double win_at(const double* p, int i) {
    if (LDS) return *((lds_f64)p + i);
    return p[i];
}

// R at np.correlate index kk (lag W-1-kk) by one lane: the four-accumulator ascending-n sum of xcorr_simple_kernel.
template <bool LDS>
__device__ inline double seeded_dot(const double* sa, const double* sb, int W, int kk) {
    const int d = kk - (W - 1);
    const int nlo = d < 0 ? -d : 0;
    const int nhi = d < 0 ? W : W - d;
    double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;
    int n = nlo;
    for (; n + 3 < nhi; n += 4) {
        c0 = __builtin_fma(win_at<LDS>(sa, n + d), win_at<LDS>(sb, n), c0);
        c1 = __builtin_fma(win_at<LDS>(sa, n + d + 1), win_at<LDS>(sb, n + 1), c1);
        c2 = __builtin_fma(win_at<LDS>(sa, n + d + 2), win_at<LDS>(sb, n + 2), c2);
        c3 = __builtin_fma(win_at<LDS>(sa, n + d + 3), win_at<LDS>(sb, n + 3), c3);
    }
    for (; n < nhi; ++n) c0 = __builtin_fma(win_at<LDS>(sa, n + d), win_at<LDS>(sb, n), c0);
    return (c0 + c1) + (c2 + c3);
}

// The pick of one pair by one wave: sa, sb the two windows (LDS or global memory), ssa, ssb their sums of squares.  Lane l
// takes the np.correlate indices W-1-hi + l, + 64, ... up to W-1-lo.  Every lane returns the same (value, index).
template <bool LDS>
__device__ inline void seeded_pick(const double* sa, const double* sb, int W, int lo, int hi, double ssa, double ssb, int lane,
                                   double& best, int& bestk) {
    const double nrm_ab = ssa * ssb;
    best = -__builtin_inf();
    bestk = NO_PICK;
    for (int kk = (W - 1 - hi) + lane; kk <= (W - 1) - lo; kk += 64) {
        const double cc = seeded_dot<LDS>(sa, sb, W, kk);
        if (better_s(cc, kk, best, bestk, nrm_ab)) { best = cc; bestk = kk; }
    }
    for (int off = 32; off > 0; off >>= 1) {                      // (a total order: every lane ends with the same pick)
        const double ov = __shfl_xor(best, off, 64);
        const int ok = __shfl_xor(bestk, off, 64);
        if (better_s(ov, ok, best, bestk, nrm_ab)) { best = ov; bestk = ok; }
    }
    if (!nbls_wave::finite_f64(ssa) || !nbls_wave::finite_f64(ssb)) {      // NaN / Inf samples: the range's first lag, NaN
        bestk = W - 1 - hi;
        best = __builtin_nan("");
    }
}

// ------------------------------------------------------------------------------------
// Form 1.  LDS: [N][W] the unit's windows | [N] their sums of squares.  64 N threads: wave wv stages element wv.  Then
//   * S = 2K + 1 <= 64 lags a pair (the half-widths the feature is made for: 37 at K = 18): the P S (pair, lag) items of
//     the unit lie in one row, pair-major, and wave wv takes the chunks wv, wv + N, ... of 64 consecutive items — every
//     lane at work, not S of 64 —, one dot product a lane.  A chunk holds the ends of up to 64 pairs: a segmented shuffle
//     reduce under the total order leaves each pair's best of the chunk in the first lane of its segment, which puts it
//     in the pair's slot of a small static table (a pair lies in at most two chunks); after a barrier thread k combines
//     the slots of pair k and stores.  An item whose lag falls below lo (a range cut by the clamp) takes no part.
//   * longer ranges: wave wv takes the pairs wv, wv + N, ... whole (seeded_pick), lanes over the lags in trips of 64.
// The dot product of a (pair, lag) and the total order are the same either way: the same bits.
// ------------------------------------------------------------------------------------
constexpr int SEED_MAX_PAIRS = 120;            // 16 elements

__global__ __launch_bounds__(1024) void xcorr_seeded_staged_kernel(SdArgs a) {
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
                    cc = seeded_dot<true>(sm + (size_t)ci * W, sm + (size_t)cj * W, W, kk);
                }
            }
            for (int off = 1; off < 64; off <<= 1) {              // lane l: the best of its pair's lanes l .. l + 2 off - 1
                const double ov = __shfl_down(cc, off, 64);
                const int ok = __shfl_down(kk, off, 64);
                const int okey = __shfl_down(k, off, 64);
                if (lane + off < 64 && okey == k && better_s(ov, ok, cc, kk, nrm_ab)) { cc = ov; kk = ok; }
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
            if (better_s(part_v[2 * k + 1], part_k[2 * k + 1], best, bestk, nrm_ab)) { best = part_v[2 * k + 1]; bestk = part_k[2 * k + 1]; }
            if (!nbls_wave::finite_f64(nrm[ci]) || !nbls_wave::finite_f64(nrm[cj])) {      // as seeded_pick
                int lo, hi;
                seeded_range(a.delay, N, g, ci, cj, W, K, lo, hi);
                bestk = W - 1 - hi;
                best = __builtin_nan("");
            }
            const int64_t o = cell * a.npairs + k;
            a.lag[o] = (W - 1) - bestk;
            a.cmax[o] = best / sqrt(nrm_ab);
        }
        return;
    }
    for (int k = wv; k < a.npairs; k += N) {                      // (k is the same for every lane of the wave)
        const int ci = a.pair[2 * k], cj = a.pair[2 * k + 1];
        int lo, hi;
        seeded_range(a.delay, N, g, ci, cj, W, K, lo, hi);
        double best;
        int bestk;
        seeded_pick<true>(sm + (size_t)ci * W, sm + (size_t)cj * W, W, lo, hi, nrm[ci], nrm[cj], lane, best, bestk);
        if (lane == 0) {
            const int64_t o = cell * a.npairs + k;
            a.lag[o] = (W - 1) - bestk;
            a.cmax[o] = best / sqrt(nrm[ci] * nrm[cj]);
        }
    }
}

// ------------------------------------------------------------------------------------
// Form 2.  Four waves per workgroup, a wave per (unit, pair) item.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void xcorr_seeded_simple_kernel(SdArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= a.nitems) return;                                 // (the same for every lane of the wave; no barrier below)
    const int u = a.u0 + (int)(item / a.npairs);
    const int k = (int)(item % a.npairs);
    const int band = a.unit_band[u];
    const int w = a.unit_win[u];
    const int W = a.Wb[band];
    const int64_t t0 = (int64_t)w * a.incb[band];
    const int ci = a.pair[2 * k], cj = a.pair[2 * k + 1];
    const double* sa = a.filt + ((int64_t)band * a.nchans + ci) * a.npts_pad + t0;
    const double* sb = a.filt + ((int64_t)band * a.nchans + cj) * a.npts_pad + t0;
    const int64_t cell = (int64_t)band * a.vector_len + w;
    const int K = min(a.halfw[band], 2 * (W - 1));
    int lo, hi;
    seeded_range(a.delay, a.nchans, a.gindex[cell], ci, cj, W, K, lo, hi);

    double ssa = 0.0, ssb = 0.0;
    for (int n = lane; n < W; n += 64) {
        const double va = sa[n], vb = sb[n];
        ssa += va * va;
        ssb += vb * vb;
    }
    for (int off = 32; off > 0; off >>= 1) {
        ssa += __shfl_xor(ssa, off, 64);
        ssb += __shfl_xor(ssb, off, 64);
    }
    double best;
    int bestk;
    seeded_pick<false>(sa, sb, W, lo, hi, ssa, ssb, lane, best, bestk);
    if (lane == 0) {
        const int64_t o = cell * a.npairs + k;
        a.lag[o] = (W - 1) - bestk;
        a.cmax[o] = best / sqrt(ssa * ssb);
    }
}

}  // namespace

// 1: the staged form (3..16 elements whose windows and sums of squares fit SEED_LDS_MAX), 2: the general form.  The staged
// block has no padding: the half-width and the halo do not enter the fit.
int nbls_lag_seed_form_of(int nelem, int W, int max_halfwidth, int halo) {
    (void)max_halfwidth; (void)halo;
    if (nelem < 3 || nelem > 16) return 2;
    return (size_t)nelem * ((size_t)W + 1) * sizeof(double) <= SEED_LDS_MAX ? 1 : 2;
}

// The seeded pick of the units [ub, ue) of one window group (windows of gW samples), in the form `form` (1 / 2), behind the
// grid search of the same units (the caller has queued it on the handle's stream).
hipError_t nbls_launch_xcorr_seeded(nbls_handle* h, int64_t ub, int64_t ue, int gW, int form) {
    const int64_t nu = ue - ub;
    if (nu <= 0) return hipSuccess;
    SdArgs a{};
    a.filt = h->d_filt;
    a.npts_pad = h->npts_pad;
    a.nchans = h->nelem;
    a.npairs = h->npairs;
    a.pair = h->d_pair;
    a.halfw = h->d_seed;
    a.delay = h->d_grid_delay;
    a.gindex = h->d_grid_index;
    a.Wb = h->d_W;
    a.incb = h->d_inc;
    a.unit_band = h->d_unit_band;
    a.unit_win = h->d_unit_win;
    a.vector_len = h->vector_len;
    a.lag = h->d_lag;
    a.cmax = h->d_cmax;
    a.u0 = (int)ub;
    a.nitems = nu * h->npairs;
    hipError_t e;
    if (form == 1) {
        if (nbls_lag_seed_form_of(h->nelem, gW, 0, 0) != 1) return hipErrorInvalidValue;
        const size_t shm = (size_t)h->nelem * ((size_t)gW + 1) * sizeof(double);
        if (!h->seed_attr_set) {           // once per handle
            if ((e = hipFuncSetAttribute((const void*)xcorr_seeded_staged_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SEED_LDS_MAX)) != hipSuccess) return e;
            h->seed_attr_set = true;
        }
        hipLaunchKernelGGL(xcorr_seeded_staged_kernel, dim3((unsigned)nu), dim3(64 * h->nelem), shm, h->stream, a);
    } else {
        hipLaunchKernelGGL(xcorr_seeded_simple_kernel, dim3((unsigned)((a.nitems + 3) / 4)), dim3(256), 0, h->stream, a);
    }
    if ((e = hipGetLastError()) != hipSuccess || !h->refine) return e;
    return nbls_launch_refine(h, ub, nu, gW, h->stream);        // the lags' sub-sample fractions (refine.hip), behind the lag pick
}
