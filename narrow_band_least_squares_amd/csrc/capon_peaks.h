// The K strongest peaks of one spectrum of a unit (nbls_set_capon_peaks): the one body that capon_kernel
// (capon.hip) runs on its two spectra and capon_music_kernel (capon_music.hip) on its pseudo-spectrum.  Device code.
#pragma once
#include "nbls_internal.h"
#include "capon_point.h"
#include "refine_fraction.h"

namespace nbls_capon {

constexpr int PKM = NBLS_CAPON_PEAKS_MAX;

// the request and where one spectrum's results go
struct PeakOut {
    const int32_t* nbr;       // [8][G] neighbour table, -1: absent
    int G, K;
    double pfloor;
    int32_t* count;           // [cells]
    int32_t* index;           // [cells][K]
    double* power;            // [cells][K]
    double* offset;           // [cells][K][2]
};

// A unit without a spectrum: count 0, every rank empty.
__device__ inline void capon_peaks_none(const PeakOut& a, int64_t c, int tid) {
    const double nan_ = __builtin_nan("");
    if (tid == 0) a.count[c] = 0;
    if (tid < a.K) {
        const int64_t o = c * a.K + tid;
        a.index[o] = -1; a.power[o] = nan_;
        a.offset[2 * o] = nan_; a.offset[2 * o + 1] = nan_;
    }
}

// P [G]: the unit's spectrum, complete and visible to the workgroup (LDS or the unit's slab: the caller's pointer decides,
// the code is one).  (bp, bg): the spectrum's arg-max as thread 0 holds it behind capon_best.
//   1. every thread tests the points tid, tid + CT, ... against their neighbours and keeps its own K best kept peaks in
//      registers: an unrolled compare-and-swap chain, every index a constant
//   2. K rounds of capon_best over the threads' heads; the owner of a round's winner pops its head
//   3. threads k < K write rank k with its two offsets
__device__ inline void capon_peaks_of(const PeakOut& a, const double* P, int64_t c, double bp, int bg, double* sp, int* sg, int tid) {
    __shared__ double win_p[PKM + 1];         // [k]: the winner of round k; [PKM]: the arg-max, for every thread
    __shared__ int win_g[PKM + 1];
    __shared__ int cnt_w[CW];
    const int G = a.G, K = a.K;
    const double nan_ = __builtin_nan("");
    if (tid == 0) { win_p[PKM] = bp; win_g[PKM] = bg; }
    __syncthreads();
    const double pmax = win_p[PKM];
    const int gmax = win_g[PKM];
    const double thr = a.pfloor * pmax;
    double tp[PKM];
    int tg[PKM];
#pragma unroll
    for (int k = 0; k < PKM; ++k) { tp[k] = 0.0; tg[k] = -1; }
    int cnt = 0;
    for (int g = tid; g < G; g += CT) {
        const double p = P[g];
        bool peak = p == p;
#pragma unroll
        for (int d = 0; d < 8; ++d) {
            const int n = a.nbr[(int64_t)d * G + g];
            if (n < 0) continue;
            const double q = P[n];
            if (q == q && !(p > q || (p == q && g < n))) peak = false;       // capon_better(p, g; q, n) of two candidates
        }
        if (!peak) continue;
        if (!(g == gmax || a.pfloor == 0.0 || p >= thr)) continue;
        ++cnt;
        double cp = p;
        int cg = g;
#pragma unroll
        for (int k = 0; k < PKM; ++k)
            if (k < K && capon_better(cp, cg, tp[k], tg[k])) {
                const double op = tp[k]; const int og = tg[k];
                tp[k] = cp; tg[k] = cg;
                cp = op; cg = og;
            }
    }
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if ((tid & 63) == 0) cnt_w[tid >> 6] = cnt;
    for (int k = 0; k < K; ++k) {                                    // (K is the same for every thread)
        double p = tp[0];
        int g = tg[0];
        capon_best(p, g, sp, sg, tid);
        if (tid == 0) { win_p[k] = p; win_g[k] = g; }
        __syncthreads();
        const int wg = win_g[k];
        if (wg >= 0 && tg[0] == wg) {                                // the owner pops its head
#pragma unroll
            for (int j = 0; j + 1 < PKM; ++j) { tp[j] = tp[j + 1]; tg[j] = tg[j + 1]; }
            tg[PKM - 1] = -1;
        }
    }
    if (tid == 0) {
        int total = 0;
        for (int j = 0; j < CW; ++j) total += cnt_w[j];
        a.count[c] = total;
    }
    if (tid < K) {
        const int64_t o = c * K + tid;
        const int g = win_g[tid];
        if (g < 0) {
            a.index[o] = -1; a.power[o] = nan_;
            a.offset[2 * o] = nan_; a.offset[2 * o + 1] = nan_;
        } else {
            const double p0 = win_p[tid];
            a.index[o] = g; a.power[o] = p0;
            for (int ax = 0; ax < 2; ++ax) {
                const int m = a.nbr[(int64_t)(2 * ax) * G + g], q = a.nbr[(int64_t)(2 * ax + 1) * G + g];
                a.offset[2 * o + ax] = (m < 0 || q < 0) ? 0.0 : refine_fraction(P[m], p0, P[q]);
            }
        }
    }
    __syncthreads();                                                 // (win_*, cnt_w and sp / sg are free again)
}

}  // namespace nbls_capon
