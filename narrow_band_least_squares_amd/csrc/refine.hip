// Sub-sample refinement of the picked lags (nbls_set_lag_refinement).
//
// Per unit (result row r, window w, start s0 = w * inc[r], length W) and pair (i, j) with picked lag l = W-1-argmax (what
// the correlators wrote to d_lag; it stays what it is), a, b the unit's windows of elements i and j:
//   R(m) = sum_n a[n - m] b[n]   over the n with both indices in [0, W)   (= np.correlate(a, b, 'full')[W-1-m], raw)
//   Nn = R(l-1) - R(l+1),  D = R(l-1) - 2 R(l) + R(l+1),  frac = Nn / (2 D) clamped to [-1/2, 1/2]
//   frac = 0 if |l| >= W-1, if D >= 0 (no strict maximum), or if one of the three values or the quotient is not finite
// The solve kernels then read tau = ((double)lag + frac) / fs (solve.hip: tau_of).
//
// Mapping: a workgroup takes one unit, wave j of its NW waves the pairs j, j + NW, ...: one wave per (unit, pair).  The
// lanes stride over n; every lane keeps three accumulators, one per m, each added in ascending n, and the wave adds them
// with the fixed DPP tree of wave_ops.h.  All three R come from this one loop — R(l) is not cmax * norm — so their
// roundings are alike.  The order of every sum depends on (W, l) alone: no atomics, and nothing depends on the launch's
// unit range, so single, streamed, batched, window-sliced and multi-estimator passes give the same bits.
//
// Two forms of one loop.  The pairs of a unit ask for 2 P W 8 bytes of its N W 8 bytes of samples (537 KB of 77 KB at 8
// elements x 1200 samples): read from global memory that is the vector cache's and L2's load, and the kernel took 5.6 ms
// in the cfg-3 pass against the verifier's 2.2 (profiles/r10_refine_time.txt; 4.9 ms with the LDS form).  So where the unit's N windows fit REFINE_LDS_MAX bytes (two workgroups
// per CU) a workgroup of eight waves stages them in LDS once, as verify_lds_kernel does, and the pair loops read LDS;
// larger units keep the global-memory form with four waves.  A wave runs the same loop on the same values either way:
// the two forms give the same bits.
#include "nbls_internal.h"
#include "wave_ops.h"
#include "refine_fraction.h"

namespace {

constexpr int REFINE_WAVES = 4;             // global-memory form
constexpr int REFINE_LDS_WAVES = 8;         // LDS form
constexpr size_t REFINE_LDS_MAX = 80 * 1024;  // bytes of a unit's windows (nelem * W * 8) up to which they are staged in LDS

struct RArgs {
    const double* filt;       // [B][nelem][npts_pad]
    int64_t npts_pad;
    int nelem;                // rows per result row
    int npairs;
    const int32_t* pair;      // [P][2]
    const int32_t* Wb;        // [B]
    const int32_t* incb;      // [B]
    const int32_t* unit_band; // [U]
    const int32_t* unit_win;  // [U]
    int vector_len, u0, nunits;
    int maxW;                 // LDS form: the window length the dynamic LDS was sized for
    const int32_t* lag;       // [B][VL][P]
    double* frac;             // [B][VL][P]
};

template <bool LDS, int NW>
__global__ __launch_bounds__(NW * 64) void refine_lag_kernel(RArgs a) {
    extern __shared__ double refine_win[];                           // LDS form: [nelem][W] the unit's windows
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if ((int)blockIdx.x >= a.nunits) return;                         // (the same for every thread of the workgroup)
    const int u = a.u0 + blockIdx.x;
    const int row = a.unit_band[u], w = a.unit_win[u];
    const int W = a.Wb[row], P = a.npairs;
    const int64_t cell = (int64_t)row * a.vector_len + w;
    const double* base = a.filt + (int64_t)row * a.nelem * a.npts_pad + (int64_t)w * a.incb[row];
    const bool staged = LDS && W <= a.maxW;                          // (never false for the units of one window group)
    if (staged) {
        for (int e = 0; e < a.nelem; ++e)
            for (int n = threadIdx.x; n < W; n += NW * 64) refine_win[e * W + n] = base[(int64_t)e * a.npts_pad + n];
        __syncthreads();
    }
    const int64_t stride = staged ? W : a.npts_pad;
    const double* src = staged ? refine_win : base;
    for (int k = wave; k < P; k += NW) {                             // (k, l, W are the same for every lane of the wave)
        const int l = a.lag[cell * P + k];
        double f = 0.0;
        if (l > -(W - 1) && l < W - 1) {
            const double* xa = src + a.pair[2 * k] * stride;
            const double* xb = src + a.pair[2 * k + 1] * stride;
            double rm = 0.0, r0 = 0.0, rp = 0.0;                     // R(l-1), R(l), R(l+1)
            for (int n = lane; n < W; n += 64) {
                const double vb = xb[n];
                const int i0 = n - l;                                // a's index for m = l; l-1 reads i0 + 1, l+1 reads i0 - 1
                // a term whose index is outside the window is left out (not added as a zero: 0 * NaN would be NaN)
                if (i0 + 1 >= 0 && i0 + 1 < W) rm = rm + xa[i0 + 1] * vb;
                if (i0 >= 0 && i0 < W) r0 = r0 + xa[i0] * vb;
                if (i0 - 1 >= 0 && i0 - 1 < W) rp = rp + xa[i0 - 1] * vb;
            }
            rm = nbls_wave::sum_f64(rm);
            r0 = nbls_wave::sum_f64(r0);
            rp = nbls_wave::sum_f64(rp);
            f = refine_fraction(rm, r0, rp);
        }
        if (lane == 0) a.frac[cell * P + k] = f;
    }
}

}  // namespace

size_t nbls_refine_lds_bytes_of(int nelem, int W) {
    const size_t lds = (size_t)nelem * (size_t)W * sizeof(double);
    return lds <= REFINE_LDS_MAX ? lds : 0;
}

hipError_t nbls_launch_refine(nbls_handle* h, int64_t u0, int64_t nu, int gW, hipStream_t st) {
    if (nu <= 0) return hipSuccess;
    RArgs a{};
    a.filt = h->d_filt;
    a.npts_pad = h->npts_pad;
    a.nelem = h->nelem;
    a.npairs = h->npairs;
    a.pair = h->d_pair;
    a.Wb = h->d_W; a.incb = h->d_inc;
    a.unit_band = h->d_unit_band; a.unit_win = h->d_unit_win;
    a.vector_len = h->vector_len; a.u0 = (int)u0; a.nunits = (int)nu;
    a.maxW = gW;
    a.lag = h->d_lag;
    a.frac = h->d_lagfrac;
    // the units of a launch are windows of up to gW samples (one window group): their N windows in LDS where they fit
    const size_t lds = nbls_refine_lds_bytes_of(h->nelem, gW);
    if (lds) {
        if (!h->refine_attr_set) {         // once per handle (a streamed pass launches per unit batch)
            const hipError_t e = hipFuncSetAttribute((const void*)refine_lag_kernel<true, REFINE_LDS_WAVES>,
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)REFINE_LDS_MAX);
            if (e != hipSuccess) return e;
            h->refine_attr_set = true;
        }
        hipLaunchKernelGGL((refine_lag_kernel<true, REFINE_LDS_WAVES>), dim3((unsigned)nu), dim3(REFINE_LDS_WAVES * 64), lds, st, a);
    } else {
        hipLaunchKernelGGL((refine_lag_kernel<false, REFINE_WAVES>), dim3((unsigned)nu), dim3(REFINE_WAVES * 64), 0, st, a);
    }
    return hipGetLastError();
}
