// Windowed pairwise full-lag cross-correlation, lag pick and correlation maximum for every
// (band, window, pair) of the plan in one batched launch.
//
// Replaces LsBeam.correlate of lts_array (called through ltsva at
// narrow_band_least_squares.py:91,183; source absent, algorithm per SURVEY.md §3.3/§8 a8):
//     cij[:,k] = np.correlate(x_i, x_j, 'full') / sqrt(sum x_i^2 * sum x_j^2)   (2W-1 lags)
//     cmax_k   = max_l cij[l,k]
//     tau_k    = (W - (argmax_l cij[l,k] + 1)) / fs          first maximum wins
// The kernel returns the integer lag W-1-argmax (tau = lag/fs, exact) and cmax_k; the
// median over pairs (MdCCM) is taken by the solve kernel.
//
// Cost: W^2 FP64 multiply-adds per (unit, pair) — this is the dominant kernel of the path
// and it is FP64-throughput bound (2*P*W^2 flop per unit against ~8*N*inc bytes), not
// HBM bound.
#include "nbls_internal.h"
#include "wave_ops.h"
#include "lag_pick.h"

namespace {
using namespace nbls_pick;

struct XArgs {
    const double* filt;       // [B][N][npts_pad]
    int64_t npts_pad;
    int nchans;
    int npairs;
    const int32_t* pair;      // [P][2]
    const int32_t* Wb;        // [B]
    const int32_t* incb;      // [B]
    const int32_t* unit_off;  // [B+1]
    const int32_t* win_off;   // [B] first window of each band's range (window sharding)
    const int32_t* unit_band; // [U]
    int vector_len;
    int32_t* lag;             // [B][VL][P]
    double* cmax;             // [B][VL][P]
    // f64-MFMA kernel only
    int S;                    // lag blocks (of 16) per tile = floor(16 / (N-1))
    int CS;                   // LDS elements per channel buffer, == 2 (mod 32)
    int PF;                   // zero padding in front of each channel window
    int u0;                   // first unit of this launch (window groups of a plan: nbls_launch_xcorr)
    int from_global;          // xcorr_simple_kernel: the two windows do not fit a CU's LDS beside the kernel's static LDS
                              // (> 10 235 samples: nbls_route_compute) and are read from global memory (L2) instead
};

// ------------------------------------------------------------------------------------
// v1: plain VALU kernel.  One workgroup per (unit, pair); both channel windows staged in
// LDS; thread t owns lags t, t+256, ...; consecutive lanes read consecutive LDS words
// (conflict-free), the partner sample is an LDS broadcast.  Two LDS reads per FMA make it
// LDS-issue bound — it is the always-correct general-purpose path and the checker for the
// MFMA kernel.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void xcorr_simple_kernel(XArgs a) {
    extern __shared__ double sm[];
    const int tid = threadIdx.x;
    const int64_t bid = blockIdx.x;
    const int u = a.u0 + (int)(bid / a.npairs);
    const int k = (int)(bid % a.npairs);
    const int band = a.unit_band[u];
    const int w = u - a.unit_off[band] + a.win_off[band];   // window index inside the band (global)
    const int W = a.Wb[band];
    const int64_t t0 = (int64_t)w * a.incb[band];
    const int ci = a.pair[2 * k], cj = a.pair[2 * k + 1];
    const double* xa = a.filt + ((int64_t)band * a.nchans + ci) * a.npts_pad + t0;
    const double* xb = a.filt + ((int64_t)band * a.nchans + cj) * a.npts_pad + t0;
    const double* sa = a.from_global ? xa : sm;
    const double* sb = a.from_global ? xb : sm + W;
    __shared__ double red_v[8];
    __shared__ int red_k[4];
    static_assert(sizeof(red_v) + sizeof(red_k) == NBLS_SLDS_XCORR_SIMPLE, "static LDS of xcorr_simple_kernel: nbls_internal.h");

    double qa = 0.0, qb = 0.0;
    for (int n = tid; n < W; n += 256) {
        const double va = xa[n], vb = xb[n];
        if (!a.from_global) { sm[n] = va; sm[W + n] = vb; }
        qa += va * va;
        qb += vb * vb;
    }
    for (int off = 32; off > 0; off >>= 1) {
        qa += __shfl_down(qa, off, 64);
        qb += __shfl_down(qb, off, 64);
    }
    if ((tid & 63) == 0) { red_v[(tid >> 6) * 2] = qa; red_v[(tid >> 6) * 2 + 1] = qb; }
    __syncthreads();
    const double ssa = (red_v[0] + red_v[2]) + (red_v[4] + red_v[6]);
    const double ssb = (red_v[1] + red_v[3]) + (red_v[5] + red_v[7]);
    __syncthreads();

    double best = -__builtin_inf();
    int bestk = 0x7fffffff;
    const double nrm_ab = ssa * ssb;                     // (square of the norm) maxima are compared by quotient, like np.argmax(cij / norm): better_q
    const int nl = 2 * W - 1;
    for (int kk = tid; kk < nl; kk += 256) {
        const double c = lag_dot<false>(sa, sb, W, kk);
        if (nbls_wave::better_q(c, kk, best, bestk, nrm_ab)) { best = c; bestk = kk; }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_down(best, off, 64);
        const int ok = __shfl_down(bestk, off, 64);
        if (nbls_wave::better_q(ov, ok, best, bestk, nrm_ab)) { best = ov; bestk = ok; }
    }
    if ((tid & 63) == 0) { red_v[tid >> 6] = best; red_k[tid >> 6] = bestk; }
    __syncthreads();
    if (tid < 64) {
        for (int i = 1; i < 4; ++i)
            if (nbls_wave::better_q(red_v[i], red_k[i], best, bestk, nrm_ab)) { best = red_v[i]; bestk = red_k[i]; }
        if (!nbls_wave::finite_f64(ssa) || !nbls_wave::finite_f64(ssb)) {      // NaN / Inf samples: NumPy's semantics
            bestk = nbls_wave::nonfinite_argmax(sa, sb, W, tid);
            best = __builtin_nan("");
        }
        if (tid == 0) {
            store_pick(a.lag, a.cmax, ((int64_t)band * a.vector_len + w) * a.npairs + k, W, best, bestk, ssa, ssb);
        }
    }
}


// ------------------------------------------------------------------------------------
// v2: FP64 matrix-core kernel: nbls_pick::mfma_tile_body (lag_pick.h) over every lag of every pair.
// The full search orders its picks by nbls_wave::better_q alone, from (-inf, NO_PICK).  That is NOT the order of the
// range-restricted correlators (better_first): better_q(0.0, k, -inf, NO_PICK, 0) is false, so on a dead channel (sum of
// squares exactly zero) this kernel never picks a lag and stores lag = W-1 - NO_PICK, where the bounded kernel picks the
// first lag of its range.  The two are kept apart on purpose.
// ------------------------------------------------------------------------------------
struct FullSearch {
    __device__ static int wave_limit(const XArgs&, int, int W) { return W - 1; }
    __device__ static int pair_limit(const XArgs&, int, int, int W) { return W - 1; }
    __device__ static bool better(double v1, int k1, double v2, int k2, double ss) { return nbls_wave::better_q(v1, k1, v2, k2, ss); }
    static constexpr bool WAVE_PER_PAIR = false;        // (a wave per pair: four trips at 8 elements, +0.6 % of the cfg-3 pass)
    // NaN / Inf samples: NumPy's semantics (see wave_ops.h nonfinite_argmax), scanned by the pair's one thread
    __device__ static int nonfinite(const double* xa, const double* xb, int W, int, int) {
        bool has_nan = false;
        int first_a = 0x7fffffff, last_b = -1;
        for (int n = 0; n < W; ++n) {
            const double va = xa[n], vb = xb[n];
            has_nan = has_nan || (va != va) || (vb != vb);
            if (fabs(va) == __builtin_inf() && n < first_a) first_a = n;
            if (fabs(vb) == __builtin_inf()) last_b = n;
        }
        int kk = 0x7fffffff;
        if (first_a != 0x7fffffff) kk = first_a;
        if (last_b >= 0 && W - 1 - last_b < kk) kk = W - 1 - last_b;
        return (has_nan || kk == 0x7fffffff) ? 0 : kk;
    }
};

__global__ __launch_bounds__(1024) void xcorr_mfma_kernel(XArgs a) {
    extern __shared__ double sm[];
    const int u = a.u0 + blockIdx.x;
    const int band = a.unit_band[u];
    const int w = u - a.unit_off[band] + a.win_off[band];   // window index inside the band (global)
    mfma_tile_body<FullSearch>(a, band, w, a.Wb[band], sm);
}

__global__ void probe_mfma_f64_kernel(const double* a, const double* b, double* out) {
    const int lane = threadIdx.x;
    d4 acc = {0.0, 0.0, 0.0, 0.0};
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[lane], b[lane], acc, 0, 0, 0);
    out[lane * 4 + 0] = acc[0];
    out[lane * 4 + 1] = acc[1];
    out[lane * 4 + 2] = acc[2];
    out[lane * 4 + 3] = acc[3];
}

}  // namespace

// The general correlators for the units [ub, ue) (windows of up to gW samples).  impl: 1 plain VALU, 2 f64 MFMA,
// 0 the faster one that applies.
static hipError_t launch_general_range(nbls_handle* h, int64_t ub, int64_t ue, int gW, int impl, int* used) {
    XArgs a{};
    a.filt = h->d_filt;
    a.npts_pad = h->npts_pad;
    a.nchans = h->nelem;                   // array elements (several recordings: d_filt rows of result row r = band r)
    a.npairs = h->npairs;
    a.pair = h->d_pair;
    a.Wb = h->d_W;
    a.incb = h->d_inc;
    a.unit_off = h->d_unit_off;
    a.win_off = h->d_win_off;
    a.unit_band = h->d_unit_band;
    a.vector_len = h->vector_len;
    a.lag = h->d_lag;
    a.cmax = h->d_cmax;
    a.u0 = (int)ub;
    const int64_t nu = ue - ub;
    if (nu <= 0) return hipSuccess;
    // the correlator and its LDS: nbls_route_compute (xcorr_route.hip), the general correlators only
    nbls_route r;
    nbls_route_compute(nbls_route_query_of(h, gW, h->nbands, impl, true), &r);
    if (r.correlator == NBLS_ROUTE_REJECTED) return hipErrorInvalidValue;
    const size_t shm = (size_t)r.lds_dyn[NBLS_ROUTE_GENERAL];
    if (r.correlator == NBLS_ROUTE_MFMA) {
        a.S = r.S;
        a.PF = r.PFB;
        a.CS = r.CSB;
        hipError_t e = hipFuncSetAttribute((const void*)xcorr_mfma_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
        if (e != hipSuccess) return e;
        *used = 2;
        hipLaunchKernelGGL(xcorr_mfma_kernel, dim3((unsigned)nu), dim3(64 * h->nelem), shm, h->stream, a);
        return nbls_finish_lag_pick(h, ub, nu, gW);
    }
    const int64_t nblocks = nu * h->npairs;
    a.from_global = r.correlator == NBLS_ROUTE_VALU_GLOBAL ? 1 : 0;
    if (shm > 48 * 1024) {      // long windows: opt in to more than the default dynamic LDS
        hipError_t e = hipFuncSetAttribute((const void*)xcorr_simple_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
        if (e != hipSuccess) return e;
    }
    *used = 1;
    hipLaunchKernelGGL(xcorr_simple_kernel, dim3((unsigned)nblocks), dim3(256), shm, h->stream, a);
    return nbls_finish_lag_pick(h, ub, nu, gW);
}

// The correlation stage of a pass.  The plan's bands come in window groups (h->wgroups: consecutive bands of one
// window length): each group takes the int8 screening path when its channel images fit a CU's LDS (possibly with
// partner groups) and a general correlator otherwise — a long-window band of an adaptive-window plan no longer sends
// every band of the plan to the 50x slower kernel.
hipError_t nbls_launch_xcorr(nbls_handle* h) {
    if (h->nunits == 0) return hipSuccess;
    h->tim.xcorr_launches = 0;
    h->tim.xcorr_fallback_bands = 0;
    h->bev_used = 0;
    int64_t launches = 0;
    int used = 0, fallback_bands = 0;
    bool any_screen = false, any_bounded = false, any_seeded = false;
    for (const nbls_wgroup& g : h->wgroups) {
        if (g.u1 <= g.u0) continue;
        hipError_t e;
        if (h->xcorr_impl == 3 && g.screen) {
            any_screen = true;
            e = nbls_launch_xcorr_screen_range(h, g.u0, g.u1, g.W, &launches);
        } else {
            if (g.sform) {       // a plan with a lag seed: the group's grid search, then the seeded correlator in the general correlators' slot
                any_seeded = true;
                e = nbls_launch_beam_grid(h, g.u0, g.u1 - g.u0, h->stream);
                if (e == hipSuccess) e = nbls_launch_xcorr_seeded(h, g.u0, g.u1, g.W, g.sform);
            } else if (g.bform) {       // a plan with lag limits: the bounded-lag correlator in the general correlators' slot
                any_bounded = true;
                e = nbls_launch_xcorr_bounded(h, g.u0, g.u1, g.W, g.bform);
            } else {
                int u_ = 0;
                e = launch_general_range(h, g.u0, g.u1, g.W, h->xcorr_impl == 3 ? 0 : h->xcorr_impl, &u_);
                used = u_ > used ? u_ : used;
                fallback_bands += g.b1 - g.b0;
            }
            if (h->xcorr_impl != 3) ++launches;
            // per-batch solves (nbls_execute_stages: fuse_solve): a window group that does not take the screening path
            // is one batch of its own — without this its units were never solved (nbls_xcorr_screen_finish marks the
            // solve stage done for the whole pass)
            if (e == hipSuccess && h->fuse_solve) {
                e = nbls_launch_solve_range(h, g.u0, g.u1 - g.u0, h->stream);
                if (e == hipSuccess) e = nbls_queue_result_batch(h, g.u0, g.u1, h->stream);
            }
        }
        if (e != hipSuccess) return e;
    }
    if (h->xcorr_impl == 3 && (any_screen || h->fuse_solve)) {
        h->xcorr_impl_used = any_seeded ? 5 : any_bounded ? 4 : 3;
        h->tim.xcorr_fallback_bands = fallback_bands;          // bands of this pass that ran on a general correlator
        return nbls_xcorr_screen_finish(h, launches);
    }
    h->xcorr_impl_used = any_seeded ? 5 : any_bounded ? 4 : used;
    h->tim.xcorr_launches = launches;
    return hipGetLastError();
}

hipError_t nbls_launch_probe_mfma(nbls_handle* h, const double* da, const double* db, double* dout) {
    hipLaunchKernelGGL(probe_mfma_f64_kernel, dim3(1), dim3(64), 0, h->stream, da, db, dout);
    return hipGetLastError();
}
