// The parts the FP64 correlators (xcorr.hip, xcorr_bounded.hip, xcorr_seeded.hip) are built from, each stated once: the
// lane dot product, the comparison with "no lag seen yet" as the least element, the lanes-over-lags pick of one pair by one
// wave and the wave-per-item kernel body around it, and the f64-MFMA Toeplitz tile body.  Device code only.
//
// For a pair (a, b) of W-sample windows, R(m) = sum_n a[n-m] b[n] (indices inside [0, W)) = np.correlate(a, b, 'full')[W-1-m];
// a pick is (value, np.correlate index kk), lag = W-1-kk.  The order of every sum depends on (W, kk) alone, so kernels that
// take their dot from lag_dot and their order from one comparison give the same bits.
#pragma once
#include "nbls_internal.h"
#include "wave_ops.h"

namespace nbls_pick {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int NO_PICK = 0x7fffffff;         // index of a running maximum that has seen no lag yet
// nbls_wave::better_q with "no lag yet" as the least element whatever the values are.  Against the initial -inf better_q
// takes its quotient branch (|v - -inf| <= 1e-15 * inf holds) and divides by the norm: on a dead channel that is 0 / 0 = NaN
// against -inf / 0 = -inf, NaN > -inf is false, and no lag would ever be picked — in a range-restricted search the first
// lag of the range has to win there.
__device__ inline bool better_first(double v1, int k1, double v2, int k2, double ss) {
    if (k1 == NO_PICK) return false;
    if (k2 == NO_PICK) return true;
    return nbls_wave::better_q(v1, k1, v2, k2, ss);
}

// A read of a window: LDS form — volatile, so that every read stays one ds_read_b64 (256 B/clk/CU; merged in pairs into
// ds_read2_b64 they run at half that rate, as beam_grid.hip found for its own loop) — or a plain pointer read.
typedef const volatile __attribute__((address_space(3))) double* lds_f64;
template <bool LDS>
__device__ inline double win_at(const double* p, int i) {
    if (LDS) return *((lds_f64)p + i);
    return p[i];
}

// R at np.correlate index kk (lag W-1-kk) by one lane: four accumulators over ascending n, reduced as (c0+c1)+(c2+c3).
// Every bit-for-bit equality between the correlators' forms rests on this order.
template <bool LDS>
__device__ inline double lag_dot(const double* sa, const double* sb, int W, int kk) {
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

// The sums of squares of a pair's windows by one wave: a 64-lane strided sum and one xor tree (every lane the result).
__device__ inline void pair_sumsq(const double* sa, const double* sb, int W, int lane, double& ssa, double& ssb) {
    ssa = 0.0;
    ssb = 0.0;
    for (int n = lane; n < W; n += 64) {
        const double va = sa[n], vb = sb[n];
        ssa += va * va;
        ssb += vb * vb;
    }
    for (int off = 32; off > 0; off >>= 1) {
        ssa += __shfl_xor(ssa, off, 64);
        ssb += __shfl_xor(ssb, off, 64);
    }
}

// The result of a pair at offset o of the pass's lag / cmax rows (plain vector stores).
__device__ inline void store_pick(int32_t* lag, double* cmax, int64_t o, int W, double best, int bestk, double ssa, double ssb) {
    lag[o] = (W - 1) - bestk;
    cmax[o] = best / sqrt(ssa * ssb);
}

// The pick of one pair over the lags lo .. hi by one wave: sa, sb the two windows (LDS or global memory), ssa, ssb their
// sums of squares.  Lane l takes the np.correlate indices W-1-hi + l, + 64, ... up to W-1-lo.  Every lane returns the same
// (value, index).  Windows that are not finite: the value is NaN and the index Policy::nonfinite(sa, sb, W, hi, lane).
template <bool LDS, class Policy>
__device__ inline void range_pick(const double* sa, const double* sb, int W, int lo, int hi, double ssa, double ssb, int lane,
                                  double& best, int& bestk) {
    const double nrm_ab = ssa * ssb;
    best = -__builtin_inf();
    bestk = NO_PICK;
    for (int kk = (W - 1 - hi) + lane; kk <= (W - 1) - lo; kk += 64) {
        const double cc = lag_dot<LDS>(sa, sb, W, kk);
        if (better_first(cc, kk, best, bestk, nrm_ab)) { best = cc; bestk = kk; }
    }
    for (int off = 32; off > 0; off >>= 1) {                      // (a total order: every lane ends with the same pick)
        const double ov = __shfl_xor(best, off, 64);
        const int ok = __shfl_xor(bestk, off, 64);
        if (better_first(ov, ok, best, bestk, nrm_ab)) { best = ov; bestk = ok; }
    }
    if (!nbls_wave::finite_f64(ssa) || !nbls_wave::finite_f64(ssb)) {
        bestk = Policy::nonfinite(sa, sb, W, hi, lane);
        best = __builtin_nan("");
    }
}

// The general form of a range-restricted correlator: four waves per workgroup (256 threads), a wave per (unit, pair) item,
// the windows read from global memory (L2).  Policy::range(a, band, cell, ci, cj, W, lo, hi) names the pair's lags.
template <class Policy>
__device__ inline void range_pick_item(const nbls_range_args& a) {
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
    int lo, hi;
    Policy::range(a, band, cell, ci, cj, W, lo, hi);
    double ssa, ssb, best;
    int bestk;
    pair_sumsq(sa, sb, W, lane, ssa, ssb);
    range_pick<false, Policy>(sa, sb, W, lo, hi, ssa, ssb, lane, best, bestk);
    if (lane == 0) store_pick(a.lag, a.cmax, cell * a.npairs + k, W, best, bestk, ssa, ssb);
}

// ------------------------------------------------------------------------------------
// The FP64 matrix-core correlator (v_mfma_f64_16x16x4_f64) of one unit: window w of band `band`.  One workgroup per unit,
// one wave per "sliding" channel i.  The whole N-channel window sits in LDS once (zero padded, one buffer per channel).
// For wave i the positive-lag correlations against ALL other channels are a Toeplitz product that maps onto 16x16 MFMA
// tiles with no wasted lanes:
//
//     C[r][c] = sum_n'  A[r][n'] * B[n'][c],   A[r][n'] = x_i[n' + r + D0]
//                                              B[n'][c] = x_j(c)[n' - 16 s(c)]
//     => C[r][c] = sum_n x_i[n + d] x_j[n],    d = D0 + 16 s(c) + r
//
// rows r = 16 consecutive lags, columns c = (partner j, lag block s): (N-1)*S of the 16 columns are live (14/16 for N = 8).
// A tile step covers 16*S lags of every partner; its K loop runs only over the n' that can overlap (W - D0), so the
// triangular lag/overlap structure costs ~16*S/2 wasted samples per lag instead of W/2.  Ordered pair (wv, j) is lag -d of
// pair (wv, j) when wv < j (np.correlate index W-1+d) and lag +d of pair (j, wv) otherwise (index W-1-d): every ordered
// (i, j) is one column family and a full search totals P * W^2 multiply-adds, as in the direct form.
//
// LDS: [N][CS] zero-padded windows | [N] sums of squares | [N][16] best value per (wave, column) | [N][16] its np.correlate
// index.  Reads per MFMA: two ds_read_b64 (one A, one B value per lane).  A lanes read <= 17 consecutive doubles (broadcast
// + conflict free); B lanes read one double per (column, k): with the channel stride CS == 2 (mod 32) doubles and the
// 16-sample block shift, the 32 addresses of a half-wave fall on 32 distinct bank pairs.
//
// Per-lane running (max, first index) over its 4 accumulator rows and all tile steps, then a shuffle reduce over the 4
// lanes of a column, then one LDS hand-off to combine the two orderings of each pair.  Ties resolve to the smaller
// np.correlate index, like np.argmax.
//
// Policy (Args: the kernel's argument struct, with filt, npts_pad, nchans, npairs, pair, vector_len, lag, cmax, S, CS, PF):
//     wave_limit(a, wv, W)             the largest lag d wave wv has to cover (wave uniform): the tile loop's bound
//     pair_limit(a, ci, cj, W)         the largest |lag| of the pair of two elements (<= W-1): the column's mask
//     better(v1, k1, v2, k2, ss)       the order of the picks, from the start (-inf, NO_PICK)
//     WAVE_PER_PAIR                    the final combination of a pair's two orderings: by a wave, or by one thread
//     nonfinite(xa, xb, W, L, lane)    the np.correlate index of a pair whose windows are not finite, by that wave or thread
// ------------------------------------------------------------------------------------
template <class Policy, class Args>
__device__ inline void mfma_tile_body(const Args& a, int band, int w, int W, double* sm) {
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;                    // sliding channel of this wave
    const int N = a.nchans;
    const int64_t t0 = (int64_t)w * a.incb[band];
    const int S = a.S, CS = a.CS, PF = a.PF;
    double* nrm = sm + (size_t)N * CS;          // [N] sum of squares, once per element
    double* cbv = nrm + N;                      // [N][16] best value per (wave, column)
    int* cbk = (int*)(cbv + N * 16);            // [N][16] its np.correlate index

    {   // stage: wave wv loads channel wv (zero padded) and its sum of squares
        double* ch = sm + (size_t)wv * CS;
        const double* src = a.filt + ((int64_t)band * N + wv) * a.npts_pad + t0;
        double q = 0.0;
        for (int n = lane; n < CS; n += 64) {
            const int idx = n - PF;
            const double v = (idx >= 0 && idx < W) ? src[idx] : 0.0;
            ch[n] = v;
            q += v * v;
        }
        for (int off = 32; off > 0; off >>= 1) q += __shfl_down(q, off, 64);
        if (lane == 0) nrm[wv] = q;
    }
    __syncthreads();

    const int c = lane & 15, kq = lane >> 4;
    const int ncol = (N - 1) * S;
    const bool colvalid = c < ncol;
    const int jj = colvalid ? c % (N - 1) : 0;
    const int s = colvalid ? c / (N - 1) : 0;
    const int j = jj + (jj >= wv ? 1 : 0);      // partner channel of this column
    const int Lw = Policy::wave_limit(a, wv, W);
    const int Lc = colvalid ? Policy::pair_limit(a, wv, j, W) : -1;     // (-1: a dead column, nothing to pick)
    const double* pa = sm + (size_t)wv * CS + PF + kq + c;        // + D0 + n'   (row r = lane & 15)
    const double* pb = sm + (size_t)j * CS + PF + kq - 16 * s;    // + n'
    double bestv = -__builtin_inf();
    int bestk = NO_PICK;
    const double nrm_wj = wv < j ? nrm[wv] * nrm[j] : nrm[j] * nrm[wv];    // (square of the norm; product in pair order ci < cj, as in the final division)
    const int step = 16 * S;
    for (int D0 = 0; D0 <= Lw; D0 += step) {
        d4 acc = {0.0, 0.0, 0.0, 0.0};
        const int klen = W - D0;
        const double* qa = pa + D0;
        const double* qb = pb;
        int n0 = 0;
        for (; n0 + 28 < klen; n0 += 32) {
#pragma unroll
            for (int uu = 0; uu < 8; ++uu)
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(qa[n0 + 4 * uu], qb[n0 + 4 * uu], acc, 0, 0, 0);
        }
        for (; n0 < klen; n0 += 4)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(qa[n0], qb[n0], acc, 0, 0, 0);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int d = D0 + 16 * s + kq + 4 * reg;
            if (d <= Lc) {
                const int kk = (wv < j) ? (W - 1 + d) : (W - 1 - d);
                if (Policy::better(acc[reg], kk, bestv, bestk, nrm_wj)) { bestv = acc[reg]; bestk = kk; }
            }
        }
    }
    for (int off = 16; off <= 32; off <<= 1) {
        const double ov = __shfl_xor(bestv, off, 64);
        const int ok = __shfl_xor(bestk, off, 64);
        if (Policy::better(ov, ok, bestv, bestk, nrm_wj)) { bestv = ov; bestk = ok; }
    }
    if (lane < 16) { cbv[wv * 16 + lane] = bestv; cbk[wv * 16 + lane] = bestk; }
    __syncthreads();
    // the two orderings of every pair combined: a wave per pair (every lane the same few LDS words; lane 0 stores) or a
    // thread per pair — the same integers and cmax either way, the policy names the one its kernel is timed with
    auto finish_pair = [&](int k, bool store) {
        const int ci = a.pair[2 * k], cj = a.pair[2 * k + 1];     // ci < cj
        double bv = -__builtin_inf();
        int bk = NO_PICK;
        const double nrm_p2 = nrm[ci] * nrm[cj];
        for (int ss = 0; ss < S; ++ss) {
            const int c1 = (cj - 1) + (N - 1) * ss;     // wave ci, partner cj
            if (Policy::better(cbv[ci * 16 + c1], cbk[ci * 16 + c1], bv, bk, nrm_p2)) { bv = cbv[ci * 16 + c1]; bk = cbk[ci * 16 + c1]; }
            const int c2 = ci + (N - 1) * ss;           // wave cj, partner ci
            if (Policy::better(cbv[cj * 16 + c2], cbk[cj * 16 + c2], bv, bk, nrm_p2)) { bv = cbv[cj * 16 + c2]; bk = cbk[cj * 16 + c2]; }
        }
        if (!nbls_wave::finite_f64(nrm[ci]) || !nbls_wave::finite_f64(nrm[cj])) {      // NaN / Inf samples: NumPy's semantics
            bk = Policy::nonfinite(sm + (size_t)ci * CS + PF, sm + (size_t)cj * CS + PF, W, Policy::pair_limit(a, ci, cj, W), lane);
            bv = __builtin_nan("");
        }
        if (store) store_pick(a.lag, a.cmax, ((int64_t)band * a.vector_len + w) * a.npairs + k, W, bv, bk, nrm[ci], nrm[cj]);
    };
    if (Policy::WAVE_PER_PAIR) {
        for (int k = wv; k < a.npairs; k += N) finish_pair(k, lane == 0);
    } else if (tid < a.npairs) {
        finish_pair(tid, true);
    }
}

}  // namespace nbls_pick
