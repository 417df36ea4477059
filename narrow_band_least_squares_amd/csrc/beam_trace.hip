// The beam trace of every result row: the delay-and-sum beam steered, window by window, at the slowness the window solved,
// and the overlapping windows stitched with a synthesis window (nbls_set_beam_trace; the definition is in
// include/nbls.h).
//
// Per result row r (N elements, window length W, hop inc, nwin[r] windows, synthesis window g[0..W)) and sample n:
//   window w (s0 = w * inc) is usable iff w < nwin[r], z0 and z1 of its cell are finite, every |fs * (xij[m-1] . z)| < 2^30,
//   and, with the gate on, mdccm[cell] >= mdccm_min
//   d_0 = 0,  d_m = rint(fs * (xij[m-1][0] * z0 + xij[m-1][1] * z1))   always against element 0's position
//   s_w[t] = ((0.0 + x_a) + x_b) + ...   over the window's elements in ascending m,  x_m = filt[r][m][s0 + t + d_m], 0.0
//                                        outside [0, npts)
//   acc = sum_w g[n - s0] * s_w[n - s0],  den = sum_w g[n - s0] * M_w   over the usable windows with 0 <= n - s0 < W, in
//                                        ascending w, both from 0.0;  trace[r][n] = den > 0 ? acc / den : 0.0
//
// Mapping: a gather, one output sample owned by one thread.  A workgroup of BT_THREADS threads takes a tile of BT_TILE
// consecutive samples of one row: wave v the samples [v * 64 * BT_SPT, (v + 1) * 64 * BT_SPT) of the tile, lane l the BT_SPT
// samples l, l + 64, ... of those — a wave reads 64 consecutive doubles of a channel row per element and sample group, and
// the BT_SPT loads of an element are independent.  The window loop is uniform in the workgroup (the windows that can touch
// the tile, ascending); a wave passes over a window that does not touch its own samples, and over an unusable one, before
// it reads a sample.  Every wave works out the window's delays for itself: lane m holds d_m and the element loop reads it
// back with readlane (beam.hip).  No LDS, no barrier, no atomics; the order of every sum depends on (N, the kept set, W,
// inc) alone and nothing on the launch, so single, streamed, batched and HBM-round passes give the same bits.
//
// The KEPT instance (NBLS_BEAM_TRACE_KEPT) sums a window over the elements its dropped mask leaves (kept.hip; the whole
// array where fewer than 3 would remain) and counts M_w of them; the delays stay those against element 0.
#include "nbls_internal.h"
#include "wave_ops.h"

namespace {

constexpr int BT_THREADS = 256;          // threads of a workgroup
constexpr int BT_SPT = 4;                // samples per thread, 64 apart
constexpr int BT_TILE = BT_THREADS * BT_SPT;      // samples of a workgroup's tile
constexpr double BT_MAX_DELAY = 1073741824.0;     // 2^30 samples: beyond, the window is unusable
// lane m of a wave holds d_m: at most 64 elements (the plan's pair limit keeps every array below that)
static_assert((64 + 1) * 64 / 2 > NBLS_MAX_PAIRS, "beam_trace_kernel keeps one element's delay per lane");

struct TArgs {
    const double* filt;       // [R][N][npts_pad]
    int64_t npts, npts_pad;
    int N;
    const double* xij;        // [P][2] estimator 0's co-array: row m - 1 is pair (0, m)
    const double* z;          // [R][VL][2]
    const double* mdccm;      // [R][VL]
    double fs;
    int gate;                 // 1: windows with !(mdccm >= mdccm_min) are not used
    double mdccm_min;
    const int32_t* Wb;        // [R]
    const int32_t* incb;      // [R]
    const int32_t* nwin;      // [R]
    const double* win;        // the synthesis windows, band after band
    const int32_t* win_off;   // [R] where the row's window starts in `win`
    int vector_len;
    int64_t ntiles;           // tiles of a row
    double* trace;            // [R][npts_pad]
    const uint32_t* dropped;  // [R][VL] the KEPT instance: bit m set, element m is dropped (kept.hip)
};

template <bool KEPT>
__global__ __launch_bounds__(BT_THREADS) void beam_trace_kernel(TArgs a) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t row = (int64_t)blockIdx.x / a.ntiles, tile = (int64_t)blockIdx.x - row * a.ntiles;
    const int W = a.Wb[row], inc = a.incb[row], nwin = a.nwin[row];
    const int64_t n0 = tile * BT_TILE;                                       // the tile [n0, n1]
    const int64_t n1 = (n0 + BT_TILE < a.npts ? n0 + BT_TILE : a.npts) - 1;
    const int64_t v0 = n0 + (int64_t)wave * 64 * BT_SPT, v1 = v0 + 64 * BT_SPT - 1;      // the wave's own samples
    const int64_t wlo = n0 - W + 1 > 0 ? (n0 - W + inc) / inc : 0;            // ceil((n0 - W + 1) / inc)
    const int64_t whi = n1 / inc < nwin - 1 ? n1 / inc : nwin - 1;
    const double* rowbase = a.filt + row * a.N * a.npts_pad;
    const double* g = a.win + a.win_off[row];
    double acc[BT_SPT], den[BT_SPT];
#pragma unroll
    for (int k = 0; k < BT_SPT; ++k) { acc[k] = 0.0; den[k] = 0.0; }
    for (int64_t w = wlo; w <= whi; ++w) {
        const int64_t s0 = w * inc;
        if (s0 + W <= v0 || s0 > v1) continue;                               // not one of this wave's samples
        const int64_t cell = row * a.vector_len + w;
        if (a.gate && !(a.mdccm[cell] >= a.mdccm_min)) continue;             // (a NaN MdCCM fails the gate)
        const double z0 = a.z[2 * cell], z1 = a.z[2 * cell + 1];
        bool bad_l = !nbls_wave::finite_f64(z0) || !nbls_wave::finite_f64(z1);
        int d_mine = 0;
        if (lane > 0 && lane < a.N) {
            const double tau = a.fs * (a.xij[2 * (lane - 1)] * z0 + a.xij[2 * (lane - 1) + 1] * z1);
            if (fabs(tau) < BT_MAX_DELAY) d_mine = (int)rint(tau);
            else bad_l = true;                                               // (NaN too)
        }
        if (__any(bad_l)) continue;
        int M = a.N;
        uint32_t bits = 0;
        if (KEPT) bits = nbls_kept_bits_of(a.dropped[cell], a.N, M);         // (N <= 32; the same in every lane)
        int64_t t[BT_SPT];
        bool in[BT_SPT];
        double s[BT_SPT];
#pragma unroll
        for (int k = 0; k < BT_SPT; ++k) {
            const int64_t n = v0 + k * 64 + lane;
            t[k] = n - s0;
            in[k] = t[k] >= 0 && t[k] < W && n < a.npts;
            s[k] = 0.0;
        }
        for (int m = 0; m < a.N; ++m) {
            if (KEPT && !((bits >> m) & 1u)) continue;
            const int d = __builtin_amdgcn_readlane(d_mine, m);
            const double* x = rowbase + (int64_t)m * a.npts_pad;
#pragma unroll
            for (int k = 0; k < BT_SPT; ++k) {
                const int64_t i = s0 + t[k] + d;
                double v = 0.0;
                if (in[k] && i >= 0 && i < a.npts) v = x[i];
                s[k] = s[k] + v;
            }
        }
        const double Md = (double)M;
#pragma unroll
        for (int k = 0; k < BT_SPT; ++k)
            if (in[k]) {
                const double gk = g[t[k]];
                acc[k] = acc[k] + gk * s[k];
                den[k] = den[k] + gk * Md;
            }
    }
    double* out = a.trace + row * a.npts_pad;
#pragma unroll
    for (int k = 0; k < BT_SPT; ++k) {
        const int64_t n = v0 + k * 64 + lane;
        if (n < a.npts) out[n] = den[k] > 0.0 ? acc[k] / den[k] : 0.0;
    }
}

}  // namespace

hipError_t nbls_launch_beam_trace(nbls_handle* h, hipStream_t st) {
    if (!h->req.bt || h->nbands < 1 || h->npts < 1) return hipSuccess;
    const nbls_estimator& s = h->est[0];
    TArgs a{};
    a.filt = h->d_filt;
    a.npts = h->npts; a.npts_pad = h->npts_pad;
    a.N = h->nelem;
    a.xij = s.d_xij;
    a.z = s.d_z;
    a.mdccm = nbls_view_of(h, s).mdccm;
    a.fs = h->fs;
    a.gate = h->req.bt_min == h->req.bt_min ? 1 : 0;                     // (off iff mdccm_min is NaN)
    a.mdccm_min = h->req.bt_min;
    a.Wb = h->d_W; a.incb = h->d_inc; a.nwin = h->d_nwin;
    a.win = h->d_bt_win; a.win_off = h->d_bt_off;
    a.vector_len = h->vector_len;
    a.ntiles = (h->npts + BT_TILE - 1) / BT_TILE;
    a.trace = h->d_bt;
    // (nbls_plan has refused such a plan)
    if (a.N < 1 || a.N > 64 || !a.filt || !a.xij || !a.z || !a.mdccm || !a.win || !a.win_off || !a.trace) return hipErrorInvalidValue;
    const int64_t blocks = a.ntiles * h->nbands;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(BT_THREADS);
    if (h->req.bt_kept()) {
        if (a.N > 32 || !h->d_kept_mask) return hipErrorInvalidValue;
        a.dropped = h->d_kept_mask;
        hipLaunchKernelGGL(beam_trace_kernel<true>, grid, block, 0, st, a);
    } else {
        hipLaunchKernelGGL(beam_trace_kernel<false>, grid, block, 0, st, a);
    }
    return hipGetLastError();
}
