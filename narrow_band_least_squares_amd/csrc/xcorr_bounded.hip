// Bounded-lag correlator (nbls_set_lag_limits): the lag pick of every (unit, pair) searched only within the
// pair's physical range |lag| <= L_k, L_k = min(max_lag[k], W-1).
//
// For one unit and pair k = (i, j), a, b the unit's windows of elements i and j, R(m) = sum_n a[n-m] b[n] (indices inside
// [0, W)) = np.correlate(a, b, 'full')[W-1-m]:
//     lag  = L - np.argmax(cij[W-1-L : W+L]),   cij = np.correlate(a, b, 'full') / sqrt(sum a^2 * sum b^2)
//     cmax = R(lag) / sqrt(sum a^2 * sum b^2)
// Quotients are compared by nbls_wave::better_q, the first maximum in np.correlate index order wins (among equal maxima the
// LARGEST lag).  An all-zero range gives lag = +L, cmax = 0; a dead channel lag = +L, cmax = NaN; windows whose sum of
// squares is not finite cmax = NaN and lag = min(the plain pass's lag, L) (nbls_wave::nonfinite_argmax_clamped).
//
// Two forms (nbls_lag_limit_form names the one a window group takes):
//   1  xcorr_bounded_mfma_kernel: the Toeplitz mapping of xcorr_mfma_kernel (xcorr.hip) on v_mfma_f64_16x16x4_f64 — one
//      workgroup per unit, one wave per sliding element, rows = 16 consecutive lags, columns = (partner, lag block), channel
//      stride == 2 (mod 32) doubles — with the tile loop cut at the largest limit among the wave's pairs and the epilogue
//      masked per pair.  3..16 elements whose zero-padded windows fit a CU's LDS (the fit rule of NBLS_ROUTE_MFMA).
//   2  xcorr_bounded_simple_kernel: a wave per (unit, pair), lanes over the lags of the range in trips of 64, each lane one
//      full dot product in the four-accumulator ascending-n order of xcorr_simple_kernel, windows read from global memory
//      (L2).  Everything else (17..32 elements, windows beyond the fit); the slow fallback and the checker of form 1.
// The order of every sum depends on (elements, W, limit table, lag) alone: no atomics, nothing depends on the launch's unit
// range.  Picks are written with plain vector stores.
#include "nbls_internal.h"
#include "wave_ops.h"

namespace {

struct BArgs {
    const double* filt;       // [B][N][npts_pad]
    int64_t npts_pad;
    int nchans;               // array elements N
    int npairs;
    const int32_t* pair;      // [P][2]
    const int32_t* limsq;     // [N][N] max_lag of the pair of two elements, symmetric, 0 on the diagonal (not yet clamped to W-1)
    const int32_t* Wb;        // [B]
    const int32_t* incb;      // [B]
    const int32_t* unit_band; // [U]
    const int32_t* unit_win;  // [U]
    int vector_len;
    int32_t* lag;             // [B][VL][P]
    double* cmax;             // [B][VL][P]
    int S, CS, PF;            // form 1: lag blocks per tile, channel stride (doubles), zero prefix — as xcorr_mfma_kernel
    int u0;                   // first unit of this launch
    int64_t nitems;           // form 2: (unit, pair) items of this launch
};

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int NO_PICK = 0x7fffffff;         // index of a running maximum that has seen no lag yet
// nbls_wave::better_q with "no lag yet" as the least element whatever the values are.  Against the initial -inf better_q
// takes its quotient branch (|v - -inf| <= 1e-15 * inf holds) and divides by the norm: on a dead channel that is 0 / 0 = NaN
// against -inf / 0 = -inf, NaN > -inf is false, and no lag would ever be picked — the first lag of the range (lag = +L)
// has to win there.
__device__ inline bool better_b(double v1, int k1, double v2, int k2, double ss) {
    if (k1 == NO_PICK) return false;
    if (k2 == NO_PICK) return true;
    return nbls_wave::better_q(v1, k1, v2, k2, ss);
}

// ------------------------------------------------------------------------------------
// Form 1.  LDS: [N][CS] zero-padded windows | [N] sums of squares | [N][16] best value per (wave, column) | [N][16] its
// np.correlate index — the layout and size of xcorr_mfma_kernel.  Wave wv covers the lags d = 0..L of its element against
// every partner: ordered pair (wv, j) is lag -d of pair (wv, j) when wv < j (np.correlate index W-1+d) and lag +d of pair
// (j, wv) otherwise (index W-1-d).
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void xcorr_bounded_mfma_kernel(BArgs a) {
    extern __shared__ double sm[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;                    // sliding channel of this wave
    const int N = a.nchans;
    const int u = a.u0 + blockIdx.x;
    const int band = a.unit_band[u];
    const int w = a.unit_win[u];
    const int W = a.Wb[band];
    const int64_t t0 = (int64_t)w * a.incb[band];
    const int S = a.S, CS = a.CS, PF = a.PF;
    double* nrm = sm + (size_t)N * CS;          // [N] sum of squares, once per element
    double* cbv = nrm + N;                      // [N][16]
    int* cbk = (int*)(cbv + N * 16);            // [N][16]

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
    // the limits: Lc of this column's pair (-1: nothing to pick), Lw the largest among the wave's pairs (wave uniform)
    const int32_t* lrow = a.limsq + wv * N;
    int Lw = 0;
    for (int q = 0; q < N; ++q) {
        const int lq = min(lrow[q], W - 1);
        if (q != wv && lq > Lw) Lw = lq;
    }
    const int Lc = colvalid ? min(lrow[j], W - 1) : -1;
    const double* pa = sm + (size_t)wv * CS + PF + kq + c;        // + D0 + n'   (row r = lane & 15)
    const double* pb = sm + (size_t)j * CS + PF + kq - 16 * s;    // + n'
    double bestv = -__builtin_inf();
    int bestk = NO_PICK;
    const double nrm_wj = wv < j ? nrm[wv] * nrm[j] : nrm[j] * nrm[wv];    // product in pair order ci < cj, as in the final division
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
            if (d <= Lc) {                                       // (Lc <= W-1; -1 for a dead column)
                const int kk = (wv < j) ? (W - 1 + d) : (W - 1 - d);
                if (better_b(acc[reg], kk, bestv, bestk, nrm_wj)) { bestv = acc[reg]; bestk = kk; }
            }
        }
    }
    for (int off = 16; off <= 32; off <<= 1) {
        const double ov = __shfl_xor(bestv, off, 64);
        const int ok = __shfl_xor(bestk, off, 64);
        if (better_b(ov, ok, bestv, bestk, nrm_wj)) { bestv = ov; bestk = ok; }
    }
    if (lane < 16) { cbv[wv * 16 + lane] = bestv; cbk[wv * 16 + lane] = bestk; }
    __syncthreads();
    // the two orderings of every pair combined, a wave per pair (every lane the same few LDS words; lane 0 stores)
    for (int k = wv; k < a.npairs; k += N) {
        const int ci = a.pair[2 * k], cj = a.pair[2 * k + 1];     // ci < cj
        double bv = -__builtin_inf();
        int bk = NO_PICK;
        const double nrm_p2 = nrm[ci] * nrm[cj];
        for (int ss = 0; ss < S; ++ss) {
            const int c1 = (cj - 1) + (N - 1) * ss;     // wave ci, partner cj
            if (better_b(cbv[ci * 16 + c1], cbk[ci * 16 + c1], bv, bk, nrm_p2)) { bv = cbv[ci * 16 + c1]; bk = cbk[ci * 16 + c1]; }
            const int c2 = ci + (N - 1) * ss;           // wave cj, partner ci
            if (better_b(cbv[cj * 16 + c2], cbk[cj * 16 + c2], bv, bk, nrm_p2)) { bv = cbv[cj * 16 + c2]; bk = cbk[cj * 16 + c2]; }
        }
        if (!nbls_wave::finite_f64(nrm[ci]) || !nbls_wave::finite_f64(nrm[cj])) {      // NaN / Inf samples: NumPy's semantics on the slice
            const int L = min(a.limsq[ci * N + cj], W - 1);
            bk = nbls_wave::nonfinite_argmax_clamped(sm + (size_t)ci * CS + PF, sm + (size_t)cj * CS + PF, W, L, lane);
            bv = __builtin_nan("");
        }
        if (lane == 0) {
            const int64_t o = ((int64_t)band * a.vector_len + w) * a.npairs + k;
            a.lag[o] = (W - 1) - bk;
            a.cmax[o] = bv / sqrt(nrm_p2);
        }
    }
}

// ------------------------------------------------------------------------------------
// Form 2.  Four waves per workgroup, a wave per (unit, pair) item.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void xcorr_bounded_simple_kernel(BArgs a) {
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
    const int L = min(a.limsq[ci * a.nchans + cj], W - 1);

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
    const double nrm_ab = ssa * ssb;

    double best = -__builtin_inf();
    int bestk = NO_PICK;
    for (int kk = (W - 1 - L) + lane; kk <= (W - 1) + L; kk += 64) {
        const int d = kk - (W - 1);
        const int nlo = d < 0 ? -d : 0;
        const int nhi = d < 0 ? W : W - d;
        double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;
        int n = nlo;
        for (; n + 3 < nhi; n += 4) {
            c0 = __builtin_fma(sa[n + d], sb[n], c0);
            c1 = __builtin_fma(sa[n + d + 1], sb[n + 1], c1);
            c2 = __builtin_fma(sa[n + d + 2], sb[n + 2], c2);
            c3 = __builtin_fma(sa[n + d + 3], sb[n + 3], c3);
        }
        for (; n < nhi; ++n) c0 = __builtin_fma(sa[n + d], sb[n], c0);
        const double cc = (c0 + c1) + (c2 + c3);
        if (better_b(cc, kk, best, bestk, nrm_ab)) { best = cc; bestk = kk; }
    }
    for (int off = 32; off > 0; off >>= 1) {                      // (a total order: every lane ends with the same pick)
        const double ov = __shfl_xor(best, off, 64);
        const int ok = __shfl_xor(bestk, off, 64);
        if (better_b(ov, ok, best, bestk, nrm_ab)) { best = ov; bestk = ok; }
    }
    if (!nbls_wave::finite_f64(ssa) || !nbls_wave::finite_f64(ssb)) {
        bestk = nbls_wave::nonfinite_argmax_clamped(sa, sb, W, L, lane);
        best = __builtin_nan("");
    }
    if (lane == 0) {
        const int64_t o = ((int64_t)band * a.vector_len + w) * a.npairs + k;
        a.lag[o] = (W - 1) - bestk;
        a.cmax[o] = best / sqrt(nrm_ab);
    }
}

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
    BArgs a{};
    a.filt = h->d_filt;
    a.npts_pad = h->npts_pad;
    a.nchans = h->nelem;
    a.npairs = h->npairs;
    a.pair = h->d_pair;
    a.limsq = h->d_limsq;
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
        nbls_route r;
        nbls_route_compute(nbls_route_query_of(h, gW, h->nbands, 2, true), &r);
        if (r.correlator != NBLS_ROUTE_MFMA) return hipErrorInvalidValue;
        const size_t shm = (size_t)r.lds_dyn[NBLS_ROUTE_GENERAL];
        a.S = r.S;
        a.PF = r.PFB;
        a.CS = r.CSB;
        if ((e = hipFuncSetAttribute((const void*)xcorr_bounded_mfma_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm)) != hipSuccess) return e;
        hipLaunchKernelGGL(xcorr_bounded_mfma_kernel, dim3((unsigned)nu), dim3(64 * h->nelem), shm, h->stream, a);
    } else {
        hipLaunchKernelGGL(xcorr_bounded_simple_kernel, dim3((unsigned)((a.nitems + 3) / 4)), dim3(256), 0, h->stream, a);
    }
    if ((e = hipGetLastError()) != hipSuccess || !h->refine) return e;
    return nbls_launch_refine(h, ub, nu, gW, h->stream);        // the lags' sub-sample fractions (refine.hip), behind the lag pick
}
