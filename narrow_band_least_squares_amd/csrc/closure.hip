// Closure (consistency) of the picked lags, per window and per element (nbls_set_closure).
//
// Per unit (result row r, window w) and estimator of N elements with its lexicographic pair list, k(i,j) the index of
// pair (i, j), i < j:
//   t_ij     plan without lag refinement:  t_ij = lag[k(i,j)]                     (int32, exactly the lag of nbls_fetch / nbls_est_fetch)
//            plan with lag refinement:     t_ij = (double)lag[k(i,j)] + frac[k(i,j)]   (the sum every other site forms, un-fused double)
//   closure  c_ijk = (t_ij + t_jk) − t_ik           for i < j < k;  T = N (N−1)(N−2) / 6 triplets
//   sums     Q = Σ_{i<j<k} c_ijk²,   E_m = Σ_{triplets that contain element m} c_ijk²,   T_m = (N−1)(N−2) / 2
//   outputs  consistency            = sqrt(Q / T) / fs                          seconds, [rows][VL]
//            closure_max            = max_{i<j<k} |c_ijk| / fs                  seconds, [rows][VL]
//            element_consistency[m] = sqrt(E_m / T_m) / fs                      seconds, [rows][VL][N]
// Without refinement c, Q and E_m are exact integers (int64: |c| <= 3 (W - 1)), converted to double once; with it
// everything is un-fused IEEE double (this file is built with -ffp-contract=off).  An estimator of fewer than three
// elements has no triplet: its outputs are zeros.
//
// Mapping: a workgroup of four waves takes four consecutive units, wave j unit j.  The wave stages its unit's row in LDS as
// the antisymmetric N x N table t[i][j], t[j][i] = -t[i][j]: a closure is three LDS reads.  The pair list's (i, j) of
// every pair index is worked out once per workgroup.  For Q and the maximum the lanes stride over the pairs (i, k) and
// loop over the j between them; for E_m, one element after the other, the lanes stride over the pairs (a, b) that do not
// hold m and close the sorted triplet of (m, a, b).  Every lane keeps its own sum in that order, the wave adds them with
// the fixed DPP tree of wave_ops.h (the integer form with a butterfly).  The order of every sum depends on N alone: no
// atomics, and nothing depends on the launch's unit range, so single, batched, streamed and sliced passes give the same bits.
#include "nbls_internal.h"
#include "wave_ops.h"

namespace {

constexpr int CLOSURE_WAVES = 4;
constexpr int CLOSURE_MAX_ELEMENTS = 32;     // 33 elements are 528 pairs: beyond the plan's pair limit
static_assert((CLOSURE_MAX_ELEMENTS + 1) * CLOSURE_MAX_ELEMENTS / 2 > NBLS_MAX_PAIRS,
              "closure_kernel keeps one element per lane of a half wave and a 16-bit pair table: revisit both before lifting the pair limit");

struct CArgs {
    const int32_t* lag;       // [B][VL][P']
    const double* frac;       // [B][VL][P'] (the refined form)
    int N, P;                 // elements and pairs of this estimator
    double fs;
    const int32_t* unit_band; // [U]
    const int32_t* unit_win;  // [U]
    int vector_len, u0, nunits;
    double* cons;             // [B][VL]
    double* cmax;             // [B][VL]
    double* el;               // [B][VL][N]
};

template <bool REFINED> struct CT;
template <> struct CT<false> { using val = int32_t; using acc = int64_t; };
template <> struct CT<true> { using val = double; using acc = double; };

__device__ inline int64_t wave_sum(int64_t v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor((long long)v, off, 64);
    return v;
}
__device__ inline double wave_sum(double v) { return nbls_wave::sum_f64(v); }
__device__ inline int32_t wave_max(int32_t v) { return (int32_t)nbls_wave::max_u32((unsigned int)v); }     // (v >= 0)
__device__ inline double wave_max(double v) { return -nbls_wave::min_f64(-v); }                             // (v >= 0, finite)
__device__ inline int32_t abs_of(int32_t v) { return v < 0 ? -v : v; }
__device__ inline double abs_of(double v) { return fabs(v); }

template <bool REFINED>
__global__ __launch_bounds__(CLOSURE_WAVES * 64) void closure_kernel(CArgs a) {
    using val = typename CT<REFINED>::val;
    using acc = typename CT<REFINED>::acc;
    __shared__ uint16_t pij[NBLS_MAX_PAIRS];                     // pair k of the list: i | j << 8
    extern __shared__ double closure_dyn[];                      // [CLOSURE_WAVES][N][N] val
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int N = a.N, P = a.P;
    for (int k = tid; k < P; k += CLOSURE_WAVES * 64) {
        int i = 0, off = 0;                                      // row i of the list starts at off and has N - 1 - i pairs
        while (k >= off + (N - 1 - i)) { off += N - 1 - i; ++i; }
        pij[k] = (uint16_t)(i | ((i + 1 + (k - off)) << 8));
    }
    val* const t = (val*)closure_dyn + (size_t)wave * N * N;
    const int ul = blockIdx.x * CLOSURE_WAVES + wave;
    const bool live = ul < a.nunits;
    int64_t cell = 0;
    __syncthreads();
    if (live) {
        const int u = a.u0 + ul;
        cell = (int64_t)a.unit_band[u] * a.vector_len + a.unit_win[u];
        for (int k = lane; k < P; k += 64) {
            val v = (val)a.lag[cell * P + k];
            if constexpr (REFINED) v = v + a.frac[cell * P + k];
            const int i = pij[k] & 0xff, j = pij[k] >> 8;
            t[i * N + j] = v;
            t[j * N + i] = -v;
        }
    }
    __syncthreads();
    if (!live) return;
    // Q and the maximum: pairs (i, k), the j between them
    acc q = 0;
    val mx = 0;
    for (int p = lane; p < P; p += 64) {
        const int i = pij[p] & 0xff, k = pij[p] >> 8;
        const val tik = t[i * N + k];
        for (int j = i + 1; j < k; ++j) {
            const val c = (t[i * N + j] + t[j * N + k]) - tik;
            q += (acc)c * (acc)c;
            const val ac = abs_of(c);
            if (ac > mx) mx = ac;
        }
    }
    q = wave_sum(q);
    mx = wave_max(mx);
    // E_m: the pairs (a, b) without m, closed over the sorted triplet
    acc e_mine = 0;
    for (int m = 0; m < N; ++m) {
        acc e = 0;
        for (int p = lane; p < P; p += 64) {
            const int pa = pij[p] & 0xff, pb = pij[p] >> 8;
            if (pa == m || pb == m) continue;
            const int i = m < pa ? m : pa;
            const int k = m > pb ? m : pb;
            const int j = m < pa ? pa : (m > pb ? pb : m);
            const val c = (t[i * N + j] + t[j * N + k]) - t[i * N + k];
            e += (acc)c * (acc)c;
        }
        e = wave_sum(e);
        if (lane == m) e_mine = e;
    }
    const double nT = (double)((int64_t)N * (N - 1) * (N - 2) / 6), nTm = (double)((int64_t)(N - 1) * (N - 2) / 2);
    if (lane == 0) {
        a.cons[cell] = N < 3 ? 0.0 : sqrt((double)q / nT) / a.fs;
        a.cmax[cell] = (double)mx / a.fs;
    }
    if (lane < N) a.el[cell * N + lane] = N < 3 ? 0.0 : sqrt((double)e_mine / nTm) / a.fs;
}

}  // namespace

hipError_t nbls_launch_closure(nbls_handle* h, const nbls_estimator& s, int64_t u0, int64_t nu, hipStream_t st) {
    if (nu <= 0) return hipSuccess;
    const nbls_est_view v = nbls_view_of(h, s);
    const size_t cells = (size_t)h->nbands * h->vector_len;
    CArgs a{};
    a.lag = v.lag;
    a.frac = v.frac;
    a.N = s.kept.empty() ? h->nelem : (int)s.kept.size();
    a.P = s.npairs;
    if (a.N > CLOSURE_MAX_ELEMENTS || a.P > NBLS_MAX_PAIRS || (int64_t)a.N * (a.N - 1) / 2 != a.P) return hipErrorInvalidValue;
    a.fs = h->fs;
    a.unit_band = h->d_unit_band; a.unit_win = h->d_unit_win;
    a.vector_len = h->vector_len; a.u0 = (int)u0; a.nunits = (int)nu;
    a.cons = s.d_closure; a.cmax = s.d_closure + cells;
    a.el = s.d_closure_el;
    const dim3 grid((unsigned)((nu + CLOSURE_WAVES - 1) / CLOSURE_WAVES)), block(CLOSURE_WAVES * 64);
    const size_t cell_sz = h->req.refine ? sizeof(double) : sizeof(int32_t);
    const size_t shm = (size_t)CLOSURE_WAVES * a.N * a.N * cell_sz;      // at most 32 KB
    if (h->req.refine) hipLaunchKernelGGL(closure_kernel<true>, grid, block, shm, st, a);
    else hipLaunchKernelGGL(closure_kernel<false>, grid, block, shm, st, a);
    return hipGetLastError();
}
