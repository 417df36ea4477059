// Each element's delay against the beam of the others, per window (nbls_set_element_delays; the definition
// is in include/nbls.h).
//
// Per unit (result row r, window w, s0 = w * inc[r], length W, K = max_shift of the row's band) of estimator 0, N elements:
//   tau_0 = 0, tau_m = fs * (xij[m-1][0] * z0 + xij[m-1][1] * z1), d_m = rint(tau_m)      always against element 0's position
//   y_m(k)[t] = filt[r][m][s0 + t + d_m + k], 0.0 outside [0, npts),  k in [-K, K]
//   b[t] = ((0.0 + y_a(0)[t]) + y_b(0)[t]) + ...  over the set S in ascending element order (all N; the KEPT instance: the
//          kept set of the unit's dropped mask, kept.hip),  b_m[t] = b[t] - y_m(0)[t] for m in S, b[t] otherwise
//   E_b,m = sum_t b_m[t]^2,  E_m(k) = sum_t y_m(k)[t]^2,  C_m(k) = sum_t y_m(k)[t] b_m[t],  c_m(k) = C_m(k) / sqrt(E_m(k) * E_b,m)
//   k* = the k of the largest c_m(k) under "c descending, |k| ascending, k ascending" (NaN is no candidate),
//   frac = refine_fraction(c_m(k*-1), c_m(k*), c_m(k*+1)), 0 where |k*| == K
//   shift = k*, cc = c_m(k*), delay = ((((double)(d_m + k*)) + frac) - tau_m) / fs
//
// Mapping: one workgroup of ED_WAVES waves per unit.  ONE wave sums one item: first the N items "E_b of element m", then
// the items (m, chunk of KC consecutive shifts), wave j taking the items j, j + ED_WAVES, ... of the list ordered by (m, k).
// Its lanes stride over t, every lane adds the products of each (m, k) in t order, the wave adds the lanes with the fixed DPP
// tree of wave_ops.h: the order of every sum depends on (N, S, W, K) alone, and not on KC (ED_CHUNK = 4 by default, 1 with
// option "element_delay_chunk": b_m[t] stays in registers for the shifts of a chunk, which saves LDS reads).  No atomics, and nothing depends on the launch's unit range: single, streamed,
// batched and window-sliced passes give the same bits.
//
// The pick needs no table of the N (2K + 1) quotients (131 KiB at 32 elements and K = 256: the LDS is the rows').  A wave's
// items ascend in (m, k), so it keeps the best (c, k) of the element it is in in registers and leaves it in LDS when the
// element changes; the (m, k) items are dealt in groups of ED_GROUP elements, so that table is [ED_WAVES][ED_GROUP].  Behind
// a group, wave j < ED_GROUP combines the sixteen candidates of element j (a total order: the deal does not show) and sums
// the two neighbours of k* again for the parabola — the same function, the same bits as the first time.
//
// Two forms of the one loop, chosen by nbls_element_delay_lds_bytes_of for the whole plan.  Staged: the N rows over
// [s0 + d_m - K, s0 + d_m + W + K), zeros outside the trace, and behind them b[W], in dynamic LDS; the loop has no bounds
// test and reads single ds_read_b64 (the volatile pointer, as in beam_grid.hip: merged pairs run at half the rate).
// Global: reads d_filt with the load-and-select of beam.hip's interpolated sums, and forms b[t] from its |S| samples where
// it needs it.  A wave adds the same values in the same order either way: the two forms give the same bits.
#include "nbls_internal.h"
#include "refine_fraction.h"
#include "wave_ops.h"

namespace {

constexpr int ED_WAVES = 16;
constexpr int ED_THREADS = ED_WAVES * 64;
constexpr int ED_GROUP = 8;                      // elements whose (m, k) items are dealt together
constexpr int ED_TU = 4;                         // samples of a lane in flight together
constexpr int ED_CHUNK = 4;                      // shifts of an element a wave takes together (option "element_delay_chunk")
constexpr int ED_MAX_ELEMENTS = 32;              // one bit per element of the dropped mask; lane m of a wave holds d_m
constexpr double ED_MAX_DELAY = 1073741824.0;    // 2^30 samples: beyond, the unit's results are NaN
// Dynamic LDS up to which a unit's rows are staged: a CU's 160 KiB less the kernel's static LDS and room to spare
constexpr size_t ED_LDS_MAX = 156 * 1024;
constexpr int ED_NONE = -0x7fffffff;             // "no candidate" in the table of the waves' bests
typedef const volatile __attribute__((address_space(3))) double* lds_f64;
static_assert(NBLS_ELEMENT_DELAY_MAX_SHIFT == 256, "the header's limit and the comment above");

struct EArgs {
    const double* filt;       // [B][N][npts_pad]
    int64_t npts, npts_pad;
    int N;
    const double* xij;        // [P][2] estimator 0's co-array: row m - 1 is pair (0, m)
    const double* z;          // [B][VL][2]
    double fs;
    const int32_t* Wb;        // [B]
    const int32_t* incb;      // [B]
    const int32_t* Kb;        // [B] max_shift of the row's band
    const int32_t* unit_band; // [U]
    const int32_t* unit_win;  // [U]
    int vector_len, u0, nunits;
    const uint32_t* dropped;  // [B][VL] the KEPT instance: bit m set, element m is dropped (kept.hip)
    double* delay;            // [B][VL][N]
    double* cc;               // [B][VL][N]
    int32_t* shift;           // [B][VL][N]
};

// What a wave needs to read the samples of one unit.  Staged form: win = the block [N][L] whose column 0 of row m is sample
// s0 + d_m - K, bsum = b[W] behind it.  Global form: rowbase = the row's [N][npts_pad], d_mine: lane m holds d_m.
struct EUnit {
    const double* win;
    const double* bsum;
    const double* rowbase;
    int64_t s0, npts, npts_pad;
    int N, W, K, L, d_mine;
    uint32_t bits;            // the set S
};

// y_m(k)[t] for t < W
template <bool LDS>
__device__ inline double ed_sample(const EUnit& c, int m, int dm, int k, int t) {
    if (LDS) return *((lds_f64)c.win + (m * c.L + c.K + k + t));
    const int64_t at = c.s0 + t + dm + k;
    const bool in = at >= 0 && at < c.npts;
    const double v = c.rowbase[(int64_t)m * c.npts_pad + (in ? at : 0)];
    return in ? v : 0.0;
}

// b[t] for t < W
template <bool LDS>
__device__ inline double ed_beam(const EUnit& c, int t) {
    if (LDS) return *((lds_f64)c.bsum + t);
    double s = 0.0;
    for (int e = 0; e < c.N; ++e)
        if ((c.bits >> e) & 1u) s = s + ed_sample<false>(c, e, __builtin_amdgcn_readlane(c.d_mine, e), 0, t);
    return s;
}

// The item "E_b of element m" of a wave -> sum_t b_m[t]^2.  m is the same in every lane.
template <bool LDS>
__device__ inline double ed_beam_energy(const EUnit& c, int m, int lane) {
    const bool in_s = (c.bits >> m) & 1u;
    const int dm = __builtin_amdgcn_readlane(c.d_mine, m);
    double sb = 0.0;
    for (int t = lane; t < c.W; t += ED_TU * 64) {
        double bm[ED_TU];
#pragma unroll
        for (int j = 0; j < ED_TU; ++j) {
            const int tj = t + j * 64;
            bm[j] = 0.0;
            if (tj < c.W) {
                bm[j] = ed_beam<LDS>(c, tj);
                if (in_s) bm[j] = bm[j] - ed_sample<LDS>(c, m, dm, 0, tj);
            }
        }
#pragma unroll
        for (int j = 0; j < ED_TU; ++j) sb = sb + bm[j] * bm[j];     // (samples beyond the window contribute zeros, in t order)
    }
    return nbls_wave::sum_f64(sb);
}

// The quotients c_m(k0), ..., c_m(k0 + KC - 1) by one wave: b_m[t] is formed once per sample and stays in registers for
// the KC shifts, so a product pair costs (2 + KC) / KC LDS reads where a single item costs 3.  Every (m, k) still adds its
// own products in t order and through the same tree: the quotients have the same bits whatever KC is.  A shift
// beyond K (the last chunk of an element) reads shift K again; the caller does not look at it.
template <bool LDS, int KC>
__device__ inline void ed_quotients(const EUnit& c, int m, int k0, int lane, double eb, double* q) {
    const bool in_s = (c.bits >> m) & 1u;
    const int dm = __builtin_amdgcn_readlane(c.d_mine, m);
    double sc[KC], se[KC];
#pragma unroll
    for (int i = 0; i < KC; ++i) { sc[i] = 0.0; se[i] = 0.0; }
    for (int t = lane; t < c.W; t += ED_TU * 64) {
        double y[KC][ED_TU], bm[ED_TU];
#pragma unroll
        for (int j = 0; j < ED_TU; ++j) {
            const int tj = t + j * 64;
            bm[j] = 0.0;
#pragma unroll
            for (int i = 0; i < KC; ++i) y[i][j] = 0.0;
            if (tj < c.W) {
                bm[j] = ed_beam<LDS>(c, tj);
                if (in_s) bm[j] = bm[j] - ed_sample<LDS>(c, m, dm, 0, tj);
#pragma unroll
                for (int i = 0; i < KC; ++i) y[i][j] = ed_sample<LDS>(c, m, dm, k0 + i < c.K ? k0 + i : c.K, tj);
            }
        }
#pragma unroll
        for (int i = 0; i < KC; ++i)
#pragma unroll
            for (int j = 0; j < ED_TU; ++j) {      // (samples beyond the window contribute zeros, in t order)
                sc[i] = sc[i] + y[i][j] * bm[j];
                se[i] = se[i] + y[i][j] * y[i][j];
            }
    }
#pragma unroll
    for (int i = 0; i < KC; ++i) q[i] = nbls_wave::sum_f64(sc[i]) / sqrt(nbls_wave::sum_f64(se[i]) * eb);
}

template <bool LDS>
__device__ inline double ed_quotient(const EUnit& c, int m, int k, int lane, double eb) {
    double q[1];
    ed_quotients<LDS, 1>(c, m, k, lane, eb, q);
    return q[0];
}

// "c descending, |k| ascending, k ascending"; a NaN is no candidate, bk == ED_NONE is "none yet"
__device__ inline bool ed_better(double v, int k, double bv, int bk) {
    if (v != v) return false;
    if (bk == ED_NONE) return true;
    if (v != bv) return v > bv;
    const int ak = k < 0 ? -k : k, abk = bk < 0 ? -bk : bk;
    return ak < abk || (ak == abk && k < bk);
}

template <bool LDS, bool KEPT, int KC>
__global__ __launch_bounds__(ED_THREADS) void element_delay_kernel(EArgs a) {
    extern __shared__ double ed_win[];                               // staged form: [N][W + 2K] the rows, then b[W]
    __shared__ double eb_s[ED_MAX_ELEMENTS];
    __shared__ double best_c[ED_WAVES][ED_GROUP];
    __shared__ int best_k[ED_WAVES][ED_GROUP];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if ((int)blockIdx.x >= a.nunits) return;                         // (the same for every thread of the workgroup)
    const int u = a.u0 + blockIdx.x;
    const int row = a.unit_band[u], w = a.unit_win[u];
    const int N = a.N;
    const int64_t cell = (int64_t)row * a.vector_len + w;
    // the delays: every wave works them out for itself, lane m holds d_m and tau_m
    const double z0 = a.z[2 * cell], z1 = a.z[2 * cell + 1];
    bool bad_l = !nbls_wave::finite_f64(z0) || !nbls_wave::finite_f64(z1);
    int d_mine = 0;
    double tau_mine = 0.0;
    if (lane > 0 && lane < N) {
        const double tau = a.fs * (a.xij[2 * (lane - 1)] * z0 + a.xij[2 * (lane - 1) + 1] * z1);
        if (fabs(tau) < ED_MAX_DELAY) { d_mine = (int)rint(tau); tau_mine = tau; }
        else bad_l = true;                                           // (NaN too)
    }
    double* const o_delay = a.delay + cell * N;
    double* const o_cc = a.cc + cell * N;
    int32_t* const o_shift = a.shift + cell * N;
    if (__any(bad_l)) {                                              // (the same in every wave: no barrier is skipped by some)
        if (tid < N) { o_delay[tid] = __builtin_nan(""); o_cc[tid] = __builtin_nan(""); o_shift[tid] = 0; }
        return;
    }
    EUnit c;
    c.N = N; c.W = a.Wb[row]; c.K = a.Kb[row]; c.L = c.W + 2 * c.K;
    c.s0 = (int64_t)w * a.incb[row]; c.npts = a.npts; c.npts_pad = a.npts_pad;
    c.rowbase = a.filt + (int64_t)row * N * a.npts_pad;
    c.win = ed_win; c.bsum = ed_win + N * c.L;
    c.d_mine = d_mine;
    int M = N;
    c.bits = N >= 32 ? 0xffffffffu : ((1u << N) - 1u);
    if (KEPT) c.bits = nbls_kept_bits_of(a.dropped[cell], N, M);
    const int W = c.W, K = c.K, L = c.L;
    if (LDS) {                                                       // one coalesced pass per row, zeros outside the trace
        for (int e = 0; e < N; ++e) {
            const int64_t first = c.s0 + __builtin_amdgcn_readlane(d_mine, e) - K;
            for (int n = tid; n < L; n += ED_THREADS) {
                const int64_t j = first + n;
                ed_win[e * L + n] = (j >= 0 && j < a.npts) ? c.rowbase[(int64_t)e * a.npts_pad + j] : 0.0;
            }
        }
        __syncthreads();
        for (int t = tid; t < W; t += ED_THREADS) {
            double s = 0.0;
            for (int e = 0; e < N; ++e)
                if ((c.bits >> e) & 1u) s = s + *((lds_f64)ed_win + (e * L + K + t));
            ed_win[N * L + t] = s;
        }
        __syncthreads();
    }
    for (int m = wave; m < N; m += ED_WAVES) {                       // E_b of every element
        const double eb = ed_beam_energy<LDS>(c, m, lane);
        if (lane == 0) eb_s[m] = eb;
    }
    __syncthreads();
    const int nk = 2 * K + 1, nck = (nk + KC - 1) / KC;                // shifts and chunks of KC shifts of an element
    for (int m0 = 0; m0 < N; m0 += ED_GROUP) {
        const int ne = N - m0 < ED_GROUP ? N - m0 : ED_GROUP;
        if (lane < ED_GROUP) best_k[wave][lane] = ED_NONE;
        int cur = -1, bk = ED_NONE;                                  // the element of the group the wave is in, and its best
        double bc = 0.0;
        for (int i = wave; i < ne * nck; i += ED_WAVES) {            // (i is the same for every lane of the wave)
            const int ml = i / nck, k0 = (i - ml * nck) * KC - K;
            if (ml != cur) {
                if (cur >= 0 && lane == 0) { best_c[wave][cur] = bc; best_k[wave][cur] = bk; }
                cur = ml; bk = ED_NONE; bc = 0.0;
            }
            double q[KC];
            ed_quotients<LDS, KC>(c, m0 + ml, k0, lane, eb_s[m0 + ml], q);
#pragma unroll
            for (int j = 0; j < KC; ++j)
                if (k0 + j <= K && ed_better(q[j], k0 + j, bc, bk)) { bc = q[j]; bk = k0 + j; }
        }
        if (cur >= 0 && lane == 0) { best_c[wave][cur] = bc; best_k[wave][cur] = bk; }
        __syncthreads();
        if (wave < ne) {                                             // the pick and the fraction of element m0 + wave
            const int m = m0 + wave;
            bc = 0.0; bk = ED_NONE;
            for (int j = 0; j < ED_WAVES; ++j) {
                const int kj = best_k[j][wave];
                if (kj != ED_NONE && ed_better(best_c[j][wave], kj, bc, bk)) { bc = best_c[j][wave]; bk = kj; }
            }
            double frac = 0.0;
            if (bk != ED_NONE && bk > -K && bk < K) {
                const double eb = eb_s[m];
                const double qm = ed_quotient<LDS>(c, m, bk - 1, lane, eb), qp = ed_quotient<LDS>(c, m, bk + 1, lane, eb);
                frac = refine_fraction(qm, bc, qp);
            }
            if (lane == 0) {
                if (bk == ED_NONE) { o_delay[m] = __builtin_nan(""); o_cc[m] = __builtin_nan(""); o_shift[m] = 0; }
                else {
                    const int dm = __builtin_amdgcn_readlane(d_mine, m);
                    const double tau = nbls_wave::readlane_f64(tau_mine, m);
                    o_delay[m] = ((((double)(dm + bk)) + frac) - tau) / a.fs;
                    o_cc[m] = bc;
                    o_shift[m] = bk;
                }
            }
        }
        __syncthreads();
    }
}

template <bool LDS>
const void* ed_kernel_of(bool kept, int chunk) {
    if (chunk == 1) return kept ? (const void*)element_delay_kernel<LDS, true, 1> : (const void*)element_delay_kernel<LDS, false, 1>;
    return kept ? (const void*)element_delay_kernel<LDS, true, ED_CHUNK> : (const void*)element_delay_kernel<LDS, false, ED_CHUNK>;
}

}  // namespace

size_t nbls_element_delay_lds_bytes_of(int nelem, int W, int max_shift) {
    const size_t lds = ((size_t)nelem * ((size_t)W + 2 * (size_t)max_shift) + (size_t)W) * sizeof(double);
    return lds <= ED_LDS_MAX ? lds : 0;
}

hipError_t nbls_launch_element_delays(nbls_handle* h, int64_t u0, int64_t nu, hipStream_t st) {
    if (nu <= 0) return hipSuccess;
    const nbls_estimator& s = h->est[0];
    EArgs a{};
    a.filt = h->d_filt;
    a.npts = h->npts; a.npts_pad = h->npts_pad;
    a.N = h->nelem;
    a.xij = s.d_xij;
    a.z = s.d_z;
    a.fs = h->fs;
    a.Wb = h->d_W; a.incb = h->d_inc; a.Kb = h->d_ed_K;
    a.unit_band = h->d_unit_band; a.unit_win = h->d_unit_win;
    a.vector_len = h->vector_len; a.u0 = (int)u0; a.nunits = (int)nu;
    a.delay = h->d_ed_fp; a.cc = h->d_ed_fp + (size_t)h->nbands * h->vector_len * h->nelem;
    a.shift = h->d_ed_shift;
    // (nbls_plan has refused such a plan)
    if (a.N < 1 || a.N > ED_MAX_ELEMENTS || !a.filt || !a.xij || !a.z || !a.Kb || !a.delay || !a.shift) return hipErrorInvalidValue;
    if (h->req.ed_kept()) {
        if (!h->d_kept_mask) return hipErrorInvalidValue;
        a.dropped = h->d_kept_mask;
    }
    const size_t lds = h->derived.ed_lds;                // the plan's form: every row's block fits (the largest one's bytes), or 0
    const int chunk = h->opt.element_delay_chunk == 1 ? 1 : ED_CHUNK;
    const int inst = (h->req.ed_kept() ? 1 : 0) + (chunk == 1 ? 2 : 0);
    if (lds && !h->ed_attr_set[inst]) {          // once per handle and instance (a streamed pass launches per unit batch)
        const hipError_t e = hipFuncSetAttribute(ed_kernel_of<true>(h->req.ed_kept(), chunk), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ED_LDS_MAX);
        if (e != hipSuccess) return e;
        h->ed_attr_set[inst] = true;
    }
    void* args[] = {&a};
    return hipLaunchKernel(lds ? ed_kernel_of<true>(h->req.ed_kept(), chunk) : ed_kernel_of<false>(h->req.ed_kept(), chunk), dim3((unsigned)nu),
                           dim3(ED_THREADS), args, lds, st);
}
