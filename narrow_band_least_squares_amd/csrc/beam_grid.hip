// Per-window search of the beam F-statistic over a grid of slowness vectors (nbls_set_beam_grid).
//
// The caller gives G slowness vectors grid[G][2] (s/km, the (z0, z1) convention of the solved z).  Once per plan, for the
// plan's full array of N = nelem elements (the geometry's first N-1 pairs are the pairs (0, i)):
//   d[g][0] = 0,  d[g][i] = rint(fs * (xij[i-1][0] * s_g0 + xij[i-1][1] * s_g1))     un-fused IEEE double, ties to even
//   H = max |d[g][i]|                                                                the plan's halo
// Per unit (result row r, window w, start s0 = w * inc[r], length W) and grid point g, the sums of beam.hip with d_i = d[g][i]:
//   x_i[t] = filt[r][i][s0 + t + d_i], 0.0 outside [0, npts)
//   b[t] = sum_i x_i[t],  S_b = sum_t b[t]^2,  S_t = sum_t sum_i x_i[t]^2,  D = N S_t - S_b
//   F(g) = (N - 1) S_b / D;  +inf if D <= 0 and S_b > 0;  NaN if S_t == 0 or a NaN sample was read
//   P(g) = S_b / (N^2 W)
// and the unit's result is the g with the largest F under the total order "F descending (+inf first), g ascending", NaN
// values not being candidates (-1 / NaN / NaN if there is none), with F and P at that g, and on request every F(g).
//
// Mapping: one workgroup of GRID_WAVES waves per unit; wave j takes the grid points j, j + GRID_WAVES, ...: ONE wave sums
// one (unit, grid point), its lanes striding over t exactly as beam_sums<64> of beam.hip does, and adds the lanes with the
// fixed DPP tree of wave_ops.h.  The order of every sum depends on (N, W) alone; the arg-max is a total order, so neither
// the deal of the grid points nor the order in which the waves' bests are combined shows in the result.  No atomics, and
// nothing depends on the launch's unit range: single, streamed, batched and window-sliced passes give the same bits.
//
// Two forms of the one loop, as refine.hip has.  A unit's G grid points ask for G N W samples of its N (W + 2H) (12 M of
// 12 k at 8 elements x 1200 samples and 1257 points), so where the block fits GRID_LDS_MAX bytes the workgroup first
// stages the N rows over [s0 - H, s0 + W + H) in LDS, zeros where the index is outside [0, npts): the loop then needs no
// bounds test, and lanes reading consecutive t are conflict-free ds_read_b64.  Larger blocks (a far grid point: a large
// halo) keep the form that reads d_filt with beam.hip's bounds test.  A wave adds the same values in the same order
// either way: the two forms give the same bits.
//
// A plan that asked for fractional-sample steering (nbls_set_beam_interpolation) runs the TAPS = 4, 6 or 8
// instances.  Its tables are n[G][N] = floor(tau) (where d stood) and c[G][N][TAPS], the Lagrange coefficients of
// mu = tau - n (steer.h), both made on the host below; x_i[t] = ((0.0 + c_0 y_0) + c_1 y_1) + ..., y_j = the sample at
// s0 + t + n_i - K + 1 + j, and its halo is H = max(|n - K + 1|, |n + K|), so the staged block still holds every tap.  Lane i
// holds n_i as it held d_i; the TAPS coefficients of (g, i) are the same for the whole wave and the table is never written
// by a kernel, so the element loop reads them as scalar loads of the constant address space, straight into SGPRs: the
// sixteen waves of a workgroup have 128 VGPRs each, and the 4 x TAPS samples in flight take 64 of them at 8 taps.
// The taps are single ds_read_b64 as well: their addresses are consecutive doubles, but a lane's first tap is 16-byte
// aligned only for every other n (no ds_read_b128), and ds_read2_b64 runs at half the rate of two ds_read_b64.
#include "nbls_internal.h"
#include "steer.h"
#include "wave_ops.h"
#include <algorithm>
#include <cmath>

namespace {

constexpr int GRID_WAVES = NBLS_BEAM_GRID_WAVES;
constexpr int GRID_TU = 4;                       // samples of a lane that go through the element loop together
constexpr int GRID_BLOCK = 64 * GRID_TU;         // samples a wave takes per step of its t loop
// Dynamic LDS up to which a unit's block is staged: a CU's 160 KiB less the kernel's static LDS (the waves' bests) and
// room to spare.  Up to half of it two workgroups share a CU, above one workgroup of sixteen waves has it alone.
constexpr size_t GRID_LDS_MAX = 156 * 1024;
typedef const volatile __attribute__((address_space(3))) double* lds_f64;   // a read of the staged block (grid_step)
typedef const __attribute__((address_space(4))) double* const_f64;          // a wave-uniform read of the coefficient table
constexpr int GRID_MAX_ELEMENTS = 64;            // lane i of a wave holds d_i (read back with readlane)
constexpr double GRID_MAX_DELAY = 1073741824.0;  // 2^30 samples: a plan whose table reaches it is refused

struct GArgs {
    const double* filt;       // [B][nelem][npts_pad]
    int64_t npts, npts_pad;
    int N;                    // elements = rows per result row
    const int32_t* Wb;        // [B]
    const int32_t* incb;      // [B]
    const int32_t* unit_band; // [U]
    const int32_t* unit_win;  // [U]
    int vector_len, u0, nunits;
    int G, halo;
    int maxW;                 // LDS form: the window length the dynamic LDS was sized for
    const int32_t* delay;     // [G][N]  (an interpolated plan: n = floor(tau))
    int32_t* index;           // [B][VL]
    double* fstat;            // [B][VL]
    double* power;            // [B][VL]
    double* map;              // [B][VL][G] or NULL
    const double* coef;       // [G][N][TAPS] an interpolated plan's Lagrange coefficients (last: the others keep their places)
};

// One step of the t loop of a wave: the samples t, t + 64, t + 128, t + 192 of the lane.  d_mine: lane i < N holds d_i.
// LDS form: src = the staged block [N][stride] whose column 0 is sample s0 - H, so x_i[t] = src[i * stride + H + d_i + t]
// and every index is inside the block; global form: src = the row's [N][npts_pad] whose column 0 is sample 0.  The four
// samples go through the element loop together (four independent loads in flight per element); their squares are added
// in t order, and a sample beyond the window or outside the trace is added as 0.0, so neither the unrolling nor the form
// shows in the result.  WHOLE: the step lies inside the window and no sample of it needs the t < W test (the LDS form
// then has no test at all).
template <bool LDS, bool WHOLE>
__device__ inline void grid_step(const double* src, int64_t stride, int64_t origin, int64_t npts, int N, int W, int d_mine,
                                 int t, double& sb, double& st) {
    double b[GRID_TU], q[GRID_TU];
#pragma unroll
    for (int k = 0; k < GRID_TU; ++k) { b[k] = 0.0; q[k] = 0.0; }
    for (int i = 0; i < N; ++i) {
        const int d = __builtin_amdgcn_readlane(d_mine, i);
        const double* row = src + (int64_t)i * stride;
        const int64_t at = origin + d;                               // scalar: index of the sample t = 0 of element i
#pragma unroll
        for (int k = 0; k < GRID_TU; ++k) {
            const int tk = t + k * 64;
            const int64_t idx = at + tk;
            double v = 0.0;
            // (inside the block: |d| <= H, tk < W.  volatile: four ds_read_b64, 256 B/clk/CU each — merged in pairs into
            //  ds_read2st64_b64 they would run at half that rate)
            if (LDS) { if (WHOLE || tk < W) v = *((lds_f64)row + (int)idx); }
            else if ((WHOLE || tk < W) && idx >= 0 && idx < npts) v = row[idx];
            b[k] += v;
            q[k] += v * v;
        }
    }
#pragma unroll
    for (int k = 0; k < GRID_TU; ++k) {
        sb += b[k] * b[k];
        st += q[k];
    }
}

// grid_step of an interpolated plan: lane i < N holds n_i in d_mine, crow[i * TAPS + j] is c_{j-K+1} of element i (the
// same address in every lane).  The global form keeps the
// bounds test per tap; the LDS form has none (|n - K + 1|, |n + K| <= H).  The TAPS loads of a sample and the four samples
// of a lane are independent; each product is rounded before its addition, the taps ascending.
template <bool LDS, bool WHOLE, int TAPS>
__device__ inline void grid_step_steer(const double* src, int64_t stride, int64_t origin, int64_t npts, int N, int W, int d_mine,
                                       const_f64 crow, int t, double& sb, double& st) {
    double b[GRID_TU], q[GRID_TU];
#pragma unroll
    for (int k = 0; k < GRID_TU; ++k) { b[k] = 0.0; q[k] = 0.0; }
    for (int i = 0; i < N; ++i) {
        const int d = __builtin_amdgcn_readlane(d_mine, i) - (TAPS / 2 - 1);
        double c[TAPS];
#pragma unroll
        for (int j = 0; j < TAPS; ++j) c[j] = crow[i * TAPS + j];
        const double* row = src + (int64_t)i * stride;
        const int64_t at = origin + d;                               // scalar: index of tap -K+1 of the sample t = 0
#pragma unroll
        for (int k = 0; k < GRID_TU; ++k) {
            const int tk = t + k * 64;
            const int64_t idx = at + tk;
            double y[TAPS];
#pragma unroll
            for (int j = 0; j < TAPS; ++j) {
                y[j] = 0.0;
                if (LDS) { if (WHOLE || tk < W) y[j] = *((lds_f64)row + (int)idx + j); }
                else {                                               // (an unconditional load of a safe index and a select:
                    const int64_t at_j = idx + j;                    //  4 x TAPS divergent branches would cost registers)
                    const bool in = (WHOLE || tk < W) && at_j >= 0 && at_j < npts;
                    const double yy = row[in ? at_j : 0];
                    y[j] = in ? yy : 0.0;
                }
            }
            double v = 0.0;
#pragma unroll
            for (int j = 0; j < TAPS; ++j) v = v + c[j] * y[j];
            b[k] += v;
            q[k] += v * v;
        }
    }
#pragma unroll
    for (int k = 0; k < GRID_TU; ++k) {
        sb += b[k] * b[k];
        st += q[k];
    }
}

// The sums of one (unit, grid point) by one wave: the whole 256-sample steps, then the partial one.
template <bool LDS, int TAPS>
__device__ inline void grid_sums(const double* src, int64_t stride, int64_t origin, int64_t npts, int N, int W, int d_mine,
                                 const_f64 crow, int lane, double& sb, double& st) {
    int t0 = 0;
    if constexpr (TAPS > 0) {
        for (; t0 + GRID_BLOCK <= W; t0 += GRID_BLOCK)
            grid_step_steer<LDS, true, TAPS>(src, stride, origin, npts, N, W, d_mine, crow, t0 + lane, sb, st);
        if (t0 < W) grid_step_steer<LDS, false, TAPS>(src, stride, origin, npts, N, W, d_mine, crow, t0 + lane, sb, st);
    } else {
        for (; t0 + GRID_BLOCK <= W; t0 += GRID_BLOCK) grid_step<LDS, true>(src, stride, origin, npts, N, W, d_mine, t0 + lane, sb, st);
        if (t0 < W) grid_step<LDS, false>(src, stride, origin, npts, N, W, d_mine, t0 + lane, sb, st);
    }
}

// "F descending (+inf first), g ascending"; a NaN is no candidate, g < 0 is "none yet".
__device__ inline bool grid_better(double f, int g, double bf, int bg) {
    if (f != f) return false;
    if (bg < 0) return true;
    return f > bf || (f == bf && g < bg);
}

template <bool LDS, int TAPS>
__global__ __launch_bounds__(GRID_WAVES * 64) void beam_grid_kernel(GArgs a) {
    extern __shared__ double grid_win[];                             // LDS form: [N][W + 2H] the unit's block
    __shared__ double best_f[GRID_WAVES], best_p[GRID_WAVES];
    __shared__ int best_g[GRID_WAVES];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if ((int)blockIdx.x >= a.nunits) return;                         // (the same for every thread of the workgroup)
    const int u = a.u0 + blockIdx.x;
    const int row = a.unit_band[u], w = a.unit_win[u];
    const int W = a.Wb[row], N = a.N, H = a.halo;
    const int64_t s0 = (int64_t)w * a.incb[row];
    const int64_t cell = (int64_t)row * a.vector_len + w;
    const double* rowbase = a.filt + (int64_t)row * N * a.npts_pad;
    const bool staged = LDS && W <= a.maxW;                          // (never false for the units of one plan)
    const int L = W + 2 * H;
    if (staged) {                                                    // one coalesced pass, zeros outside the trace
        for (int e = 0; e < N; ++e)
            for (int n = tid; n < L; n += GRID_WAVES * 64) {
                const int64_t j = s0 - H + n;
                grid_win[e * L + n] = (j >= 0 && j < a.npts) ? rowbase[(int64_t)e * a.npts_pad + j] : 0.0;
            }
        __syncthreads();
    }
    const double n_ = (double)N;
    double bf = 0.0, bp = 0.0;
    int bg = -1;
    for (int g = wave; g < a.G; g += GRID_WAVES) {                   // (g is the same for every lane of the wave)
        const int d_mine = lane < N ? a.delay[(int64_t)g * N + lane] : 0;
        const_f64 crow = nullptr;                                    // (TAPS > 0: the coefficients of this grid point)
        if constexpr (TAPS > 0)
            crow = (const_f64)(uintptr_t)a.coef + (int64_t)__builtin_amdgcn_readfirstlane(g) * N * TAPS;
        double sb = 0.0, st = 0.0;
        if (staged) grid_sums<true, TAPS>(grid_win, L, H, a.npts, N, W, d_mine, crow, lane, sb, st);
        else grid_sums<false, TAPS>(rowbase, a.npts_pad, s0, a.npts, N, W, d_mine, crow, lane, sb, st);
        sb = nbls_wave::sum_f64(sb);
        st = nbls_wave::sum_f64(st);
        double f;
        if (st == 0.0) f = __builtin_nan("");
        else {
            const double dd = n_ * st - sb;                          // (a NaN sample: NaN all the way)
            f = (dd <= 0.0 && sb > 0.0) ? __builtin_inf() : (n_ - 1.0) * sb / dd;
        }
        if (a.map && lane == 0) a.map[cell * a.G + g] = f;
        if (grid_better(f, g, bf, bg)) { bf = f; bp = sb / (n_ * n_ * (double)W); bg = g; }
    }
    if (lane == 0) { best_f[wave] = bf; best_p[wave] = bp; best_g[wave] = bg; }
    __syncthreads();
    if (tid == 0) {
        bf = 0.0; bp = 0.0; bg = -1;
        for (int j = 0; j < GRID_WAVES; ++j)
            if (best_g[j] >= 0 && grid_better(best_f[j], best_g[j], bf, bg)) { bf = best_f[j]; bp = best_p[j]; bg = best_g[j]; }
        a.index[cell] = bg;
        a.fstat[cell] = bg < 0 ? __builtin_nan("") : bf;
        a.power[cell] = bg < 0 ? __builtin_nan("") : bp;
    }
}

template <bool LDS>
const void* grid_kernel_of(int taps) {
    switch (taps) {
    case 4: return (const void*)beam_grid_kernel<LDS, 4>;
    case 6: return (const void*)beam_grid_kernel<LDS, 6>;
    case 8: return (const void*)beam_grid_kernel<LDS, 8>;
    default: return (const void*)beam_grid_kernel<LDS, 0>;
    }
}

template <int TAPS>
void steer_rows(double mu, double* c) { nbls_steer_coefficients<TAPS>(mu, c); }

}  // namespace

size_t nbls_beam_grid_lds_bytes_of(int nelem, int W, int halo) {
    const size_t lds = (size_t)nelem * ((size_t)W + 2 * (size_t)halo) * sizeof(double);
    return lds <= GRID_LDS_MAX ? lds : 0;
}

// The plan's delay table d[G][nelem] and its halo, on the host: this translation unit is built without contraction, so
// the product sum below is the un-fused double arithmetic of the contract.  false: some |fs xij . s_g| reaches 2^30.
bool nbls_beam_grid_delays_of(const double* xij, int nelem, double fs, const double* grid, int G, int32_t* d, int* halo) {
    int hmax = 0;
    for (int g = 0; g < G; ++g) {
        const double s0 = grid[2 * g], s1 = grid[2 * g + 1];
        d[(size_t)g * nelem] = 0;
        for (int i = 1; i < nelem; ++i) {
            const double tau = fs * (xij[2 * (i - 1)] * s0 + xij[2 * (i - 1) + 1] * s1);
            if (!(std::fabs(tau) < GRID_MAX_DELAY)) return false;    // (NaN too)
            const int32_t di = (int32_t)std::nearbyint(tau);         // the default rounding mode: ties to even
            d[(size_t)g * nelem + i] = di;
            const int m = di < 0 ? -di : di;
            if (m > hmax) hmax = m;
        }
    }
    *halo = hmax;
    return true;
}

// The tables of an interpolated plan, n[G][nelem] = floor(tau), c[G][nelem][taps] and the halo max(|n - K + 1|, |n + K|), on
// the host as above (steer.h has the expressions).  false: some |fs xij . s_g| reaches 2^30.
bool nbls_beam_grid_steer_of(const double* xij, int nelem, double fs, const double* grid, int G, int taps, int32_t* n, double* c,
                             int* halo) {
    const int K = taps / 2;
    int hmax = 0;
    for (int g = 0; g < G; ++g) {
        const double s0 = grid[2 * g], s1 = grid[2 * g + 1];
        for (int i = 0; i < nelem; ++i) {
            double tau = 0.0;                                        // the reference element
            if (i > 0) tau = fs * (xij[2 * (i - 1)] * s0 + xij[2 * (i - 1) + 1] * s1);
            if (!(std::fabs(tau) < GRID_MAX_DELAY)) return false;    // (NaN too)
            int ni;
            double mu;
            nbls_steer_split(tau, ni, mu);
            n[(size_t)g * nelem + i] = ni;
            double* ci = c + ((size_t)g * nelem + i) * taps;
            if (taps == 4) steer_rows<4>(mu, ci);
            else if (taps == 6) steer_rows<6>(mu, ci);
            else steer_rows<8>(mu, ci);
            const int lo = ni - K + 1, hi = ni + K;
            const int m = std::max(lo < 0 ? -lo : lo, hi < 0 ? -hi : hi);
            if (m > hmax) hmax = m;
        }
    }
    *halo = hmax;
    return true;
}

hipError_t nbls_launch_beam_grid(nbls_handle* h, int64_t u0, int64_t nu, hipStream_t st) {
    if (nu <= 0) return hipSuccess;
    if (h->nelem > GRID_MAX_ELEMENTS) return hipErrorInvalidValue;   // one element per lane (see GRID_MAX_ELEMENTS)
    const size_t cells = (size_t)h->nbands * h->vector_len;
    GArgs a{};
    a.filt = h->d_filt;
    a.npts = h->npts; a.npts_pad = h->npts_pad;
    a.N = h->nelem;
    a.Wb = h->d_W; a.incb = h->d_inc;
    a.unit_band = h->d_unit_band; a.unit_win = h->d_unit_win;
    a.vector_len = h->vector_len; a.u0 = (int)u0; a.nunits = (int)nu;
    a.G = h->derived.grid_n; a.halo = h->derived.grid_halo;
    a.maxW = h->maxW;
    a.delay = h->d_grid_delay;
    a.coef = h->req.grid_taps() ? h->d_grid_coef.p : nullptr;
    a.index = h->d_grid_index;
    a.fstat = h->d_grid_fp; a.power = h->d_grid_fp + cells;
    a.map = h->req.grid_map() ? h->d_grid_map.p : nullptr;
    // the units of a plan are windows of up to maxW samples: their block in LDS where the longest one fits
    const size_t lds = nbls_beam_grid_lds_bytes_of(h->nelem, h->maxW, h->derived.grid_halo);
    if (lds) {
        const unsigned bit = 1u << (h->req.grid_taps() / 2);
        if (!(h->grid_attr_set & bit)) {   // once per handle and instance (a streamed pass launches per unit batch)
            const hipError_t e = hipFuncSetAttribute(grid_kernel_of<true>(h->req.grid_taps()), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     (int)GRID_LDS_MAX);
            if (e != hipSuccess) return e;
            h->grid_attr_set |= bit;
        }
    }
    void* args[] = {&a};
    return hipLaunchKernel(lds ? grid_kernel_of<true>(h->req.grid_taps()) : grid_kernel_of<false>(h->req.grid_taps()), dim3((unsigned)nu),
                           dim3(GRID_WAVES * 64), args, lds, st);
}
