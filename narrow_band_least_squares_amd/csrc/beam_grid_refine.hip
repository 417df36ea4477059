// Refinement of the slowness-grid maximum between grid points (nbls_set_beam_grid_refinement).
//
// A plan with a slowness grid (beam_grid.hip) steered at fractional-sample delays (steer.h, TAPS = 4, 6 or 8) and the
// request (levels R in 1..12, step (h0, h1) s/km).  Per unit (result row r, window w), behind the grid search of the unit:
//   start   g* = grid_index;  g* = -1: slowness, fstat, power, stencil NaN, every path entry -1.
//           Otherwise c = grid[g*], Fc = grid_fstat, Pc = grid_power (the grid kernel's own bits).
//   level   l = 1 .. R:  e = (ldexp(h0, -l), ldexp(h1, -l))
//           candidates j = 0 .. 8:  a = j / 3 - 1, b = j % 3 - 1,  s_j = (c0 + a * e0, c1 + b * e1)
//           j = 4 is the centre: F_4 = Fc, P_4 = Pc, not evaluated again.  j != 4: F and P of a grid point of slowness s_j:
//             tau_i = fs * (xij[i-1][0] * s_j0 + xij[i-1][1] * s_j1) un-fused, tau_0 = 0, n = floor(tau), mu = tau - n, the
//             coefficients of steer.h, and behind them the sums, the F / P expressions, the +inf and NaN rules, the mapping
//             of t to lanes and the reduction orders of beam_grid_kernel<.., TAPS>.
//           j* = the best under "F descending (+inf first); the centre before any other; then j ascending", a NaN F being
//           no candidate;  path[l-1] = j*;  on the last level stencil[j] = F_j;  then c = s_j*, Fc = F_j*, Pc = P_j*.
//   outputs slowness (2) = c, fstat = Fc, power = Pc, path (R int32), stencil (9).
//
// Mapping: one workgroup of REFINE_WAVES = 8 waves per unit; in every level wave j takes the j-th non-centre candidate:
// lane i works out n_i and the TAPS coefficients of element i for the wave's slowness (beam.hip's interpolated instances
// do the same per unit) and the element loop reads them back with readlane — SGPR pairs; the coefficients change per level
// and per wave, so there is no table of them anywhere.  ONE wave sums one candidate exactly as a wave of beam_grid_kernel
// sums a grid point: the lanes stride over t in steps of 256 samples, four samples of a lane together, the lanes are added
// with the DPP tree of wave_ops.h.  The eight (F, P) pairs of a level meet in static LDS; every wave then applies the same
// total order to them and moves its own copy of (c, Fc, Pc): one barrier pair per level.  Thread 0 writes the unit's
// results with plain stores.  No atomics, and nothing depends on the launch's unit range.
//
// Two forms of the one loop, as beam_grid.hip has.  Where the unit's block N x (W + 2 H_r) fits REFINE_LDS_MAX bytes it is
// staged once, zeros outside the trace, and serves all 8 R evaluations; H_r, the plan's bound of every candidate's reach, is
// derived by nbls_beam_grid_refine_halo_of below, so the loop has no bounds test and the taps are single ds_read_b64
// (beam_grid.hip says why).  Larger blocks read d_filt with the select-not-branch bounds handling of the grid kernel's
// global form.  A wave adds the same values in the same order either way: the two forms give the same bits.
#include "nbls_internal.h"
#include "steer.h"
#include "wave_ops.h"
#include <cmath>

namespace {

constexpr int REFINE_WAVES = 8;                    // the non-centre candidates of a level
constexpr int REFINE_TU = 4;                       // samples of a lane that go through the element loop together (as GRID_TU)
constexpr int REFINE_BLOCK = 64 * REFINE_TU;
constexpr size_t REFINE_LDS_MAX = 156 * 1024;      // the grid kernel's cap
constexpr int REFINE_MAX_ELEMENTS = 64;            // lane i of a wave holds n_i and the coefficients of element i
constexpr double REFINE_MAX_DELAY = 1073741824.0;  // 2^30 samples
typedef const volatile __attribute__((address_space(3))) double* lds_f64;   // a read of the staged block

struct RArgs {
    const double* filt;       // [B][nelem][npts_pad]
    int64_t npts, npts_pad;
    int N;
    const int32_t* Wb;        // [B]
    const int32_t* incb;      // [B]
    const int32_t* unit_band; // [U]
    const int32_t* unit_win;  // [U]
    int vector_len, u0, nunits;
    int halo;                 // H_r
    int maxW;                 // LDS form: the window length the dynamic LDS was sized for
    const double* xij;        // [P][2] the co-array: rows 0 .. N-2 are the pairs (0, i)
    double fs;
    const double* grid;       // [G][2]
    const int32_t* gindex;    // [B][VL] the grid search's results
    const double* gfstat;     // [B][VL]
    const double* gpower;     // [B][VL]
    int levels;               // R
    double h0, h1;            // step
    double* slow;             // [B][VL][2]
    double* fstat;            // [B][VL]
    double* power;            // [B][VL]
    int32_t* path;            // [B][VL][R]
    double* stencil;          // [B][VL][9]
};

// One step of the t loop of a wave, grid_step_steer of beam_grid.hip with the coefficients in lanes: lane i < N holds n_i
// in n_mine and c_{j-K+1} of element i in c_mine[j].  The same loads, products and additions in the same order.
template <bool LDS, bool WHOLE, int TAPS>
__device__ inline void refine_step(const double* src, int64_t stride, int64_t origin, int64_t npts, int N, int W, int n_mine,
                                   const double* c_mine, int t, double& sb, double& st) {
    double b[REFINE_TU], q[REFINE_TU];
#pragma unroll
    for (int k = 0; k < REFINE_TU; ++k) { b[k] = 0.0; q[k] = 0.0; }
    for (int i = 0; i < N; ++i) {
        const int d = __builtin_amdgcn_readlane(n_mine, i) - (TAPS / 2 - 1);
        double c[TAPS];
#pragma unroll
        for (int j = 0; j < TAPS; ++j) c[j] = nbls_wave::readlane_f64(c_mine[j], i);
        const double* row = src + (int64_t)i * stride;
        const int64_t at = origin + d;                               // scalar: index of tap -K+1 of the sample t = 0
#pragma unroll
        for (int k = 0; k < REFINE_TU; ++k) {
            const int tk = t + k * 64;
            const int64_t idx = at + tk;
            double y[TAPS];
#pragma unroll
            for (int j = 0; j < TAPS; ++j) {
                y[j] = 0.0;
                if (LDS) { if (WHOLE || tk < W) y[j] = *((lds_f64)row + (int)idx + j); }
                else {                                               // (an unconditional load of a safe index and a select)
                    const int64_t at_j = idx + j;
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
    for (int k = 0; k < REFINE_TU; ++k) {
        sb += b[k] * b[k];
        st += q[k];
    }
}

// The sums of one candidate by one wave: the whole 256-sample steps, then the partial one (grid_sums of beam_grid.hip).
template <bool LDS, int TAPS>
__device__ inline void refine_sums(const double* src, int64_t stride, int64_t origin, int64_t npts, int N, int W, int n_mine,
                                   const double* c_mine, int lane, double& sb, double& st) {
    int t0 = 0;
    for (; t0 + REFINE_BLOCK <= W; t0 += REFINE_BLOCK)
        refine_step<LDS, true, TAPS>(src, stride, origin, npts, N, W, n_mine, c_mine, t0 + lane, sb, st);
    if (t0 < W) refine_step<LDS, false, TAPS>(src, stride, origin, npts, N, W, n_mine, c_mine, t0 + lane, sb, st);
}

template <bool LDS, int TAPS>
__global__ __launch_bounds__(REFINE_WAVES * 64) void grid_refine_kernel(RArgs a) {
    extern __shared__ double refine_win[];                           // LDS form: [N][W + 2 H_r] the unit's block
    __shared__ double cand_f[REFINE_WAVES], cand_p[REFINE_WAVES];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if ((int)blockIdx.x >= a.nunits) return;                         // (the same for every thread of the workgroup)
    const int u = a.u0 + blockIdx.x;
    const int row = a.unit_band[u], w = a.unit_win[u];
    const int W = a.Wb[row], N = a.N, H = a.halo, R = a.levels;
    const int64_t s0 = (int64_t)w * a.incb[row];
    const int64_t cell = (int64_t)row * a.vector_len + w;
    const int gstar = a.gindex[cell];
    if (gstar < 0) {                                                 // (the same for every thread: no grid point had a ratio)
        if (tid == 0) {
            const double nan_ = __builtin_nan("");
            a.slow[2 * cell] = nan_; a.slow[2 * cell + 1] = nan_;
            a.fstat[cell] = nan_; a.power[cell] = nan_;
            for (int j = 0; j < 9; ++j) a.stencil[9 * cell + j] = nan_;
        }
        for (int l = tid; l < R; l += REFINE_WAVES * 64) a.path[cell * R + l] = -1;
        return;
    }
    const double* rowbase = a.filt + (int64_t)row * N * a.npts_pad;
    const bool staged = LDS && W <= a.maxW;                          // (never false for the units of one plan)
    const int L = W + 2 * H;
    if (staged) {                                                    // one coalesced pass, zeros outside the trace
        for (int e = 0; e < N; ++e)
            for (int n = tid; n < L; n += REFINE_WAVES * 64) {
                const int64_t j = s0 - H + n;
                refine_win[e * L + n] = (j >= 0 && j < a.npts) ? rowbase[(int64_t)e * a.npts_pad + j] : 0.0;
            }
        __syncthreads();
    }
    const double n_ = (double)N;
    double c0 = a.grid[2 * gstar], c1 = a.grid[2 * gstar + 1], fc = a.gfstat[cell], pc = a.gpower[cell];
    const int jmine = wave < 4 ? wave : wave + 1;                    // the wave's candidate: 0 .. 8 without the centre
    const double am = (double)(jmine / 3 - 1), bm = (double)(jmine % 3 - 1);
    double x0 = 0.0, x1 = 0.0;                                       // lane i: the co-array row of pair (0, i)
    if (lane > 0 && lane < N) { x0 = a.xij[2 * (lane - 1)]; x1 = a.xij[2 * (lane - 1) + 1]; }
    for (int l = 1; l <= R; ++l) {
        const double e0 = ldexp(a.h0, -l), e1 = ldexp(a.h1, -l);
        const double sj0 = c0 + am * e0, sj1 = c1 + bm * e1;
        int n_mine = 0;
        double c_mine[TAPS];
        bool out_l = false;                                          // a delay the plan's bound does not cover (never, see halo_of)
        {
            const double tau = (lane > 0 && lane < N) ? a.fs * (x0 * sj0 + x1 * sj1) : 0.0;
            double mu = 0.0;
            if (fabs(tau) < REFINE_MAX_DELAY) nbls_steer_split(tau, n_mine, mu);
            else out_l = true;                                       // (NaN too)
            nbls_steer_coefficients<TAPS>(mu, c_mine);
            const int lo = n_mine - TAPS / 2 + 1, hi = n_mine + TAPS / 2;
            if (lo < -H || hi > H) out_l = true;                     // (either form: the same bits whatever the bound)
        }
        const bool out = __any(out_l) != 0;
        double sb = 0.0, st = 0.0, f = __builtin_nan("");
        if (!out) {                                                  // (the same for every lane of the wave)
            if (staged) refine_sums<true, TAPS>(refine_win, L, H, a.npts, N, W, n_mine, c_mine, lane, sb, st);
            else refine_sums<false, TAPS>(rowbase, a.npts_pad, s0, a.npts, N, W, n_mine, c_mine, lane, sb, st);
            sb = nbls_wave::sum_f64(sb);
            st = nbls_wave::sum_f64(st);
            if (st != 0.0) {
                const double dd = n_ * st - sb;                      // (a NaN sample: NaN all the way)
                f = (dd <= 0.0 && sb > 0.0) ? __builtin_inf() : (n_ - 1.0) * sb / dd;
            }
        }
        if (lane == 0) { cand_f[wave] = f; cand_p[wave] = sb / (n_ * n_ * (double)W); }
        __syncthreads();
        // "F descending (+inf first); the centre before any other; then j ascending": the centre holds until a strictly
        // larger F comes, the candidates in ascending j; a NaN compares false
        int jbest = 4;
        double fbest = fc, pbest = pc;
        for (int k = 0; k < REFINE_WAVES; ++k) {
            const double fk = cand_f[k];
            if (fk > fbest) { fbest = fk; pbest = cand_p[k]; jbest = k < 4 ? k : k + 1; }
        }
        if (tid == 0) {
            a.path[cell * R + (l - 1)] = jbest;
            if (l == R)
                for (int j = 0; j < 9; ++j) a.stencil[9 * cell + j] = j == 4 ? fc : cand_f[j < 4 ? j : j - 1];
        }
        if (jbest != 4) {                                            // s_j* (the wave that summed it formed the same bits)
            c0 = c0 + (double)(jbest / 3 - 1) * e0;
            c1 = c1 + (double)(jbest % 3 - 1) * e1;
            fc = fbest; pc = pbest;
        }
        __syncthreads();                                             // cand_f / cand_p are free for the next level
    }
    if (tid == 0) {
        a.slow[2 * cell] = c0; a.slow[2 * cell + 1] = c1;
        a.fstat[cell] = fc; a.power[cell] = pc;
    }
}

template <bool LDS>
const void* refine_kernel_of(int taps) {
    switch (taps) {
    case 4: return (const void*)grid_refine_kernel<LDS, 4>;
    case 6: return (const void*)grid_refine_kernel<LDS, 6>;
    default: return (const void*)grid_refine_kernel<LDS, 8>;
    }
}

}  // namespace

size_t nbls_beam_grid_refine_lds_bytes_of(int nelem, int W, int halo) {
    const size_t lds = (size_t)nelem * ((size_t)W + 2 * (size_t)halo) * sizeof(double);
    return lds <= REFINE_LDS_MAX ? lds : 0;
}

// The plan's bound of every candidate's reach: H_r = grid_halo + ceil(fs max_i(|xij[i][0]| h0 + |xij[i][1]| h1)) + 1 over
// the pairs (0, i) of the array.  A centre is never further than step (1 - 2^-R) from its grid point on either axis, so a
// candidate's delay differs from the grid point's by less than the ceil term; the grid halo covers the grid point's taps
// and the 1 the roundings of the two delays.  -1: the bound reaches 2^30 (or is not a number).
int64_t nbls_beam_grid_refine_halo_of(const double* xij, int nelem, double fs, int grid_halo, const double* step) {
    double m = 0.0;
    for (int i = 1; i < nelem; ++i) {
        const double r = std::fabs(xij[2 * (i - 1)]) * step[0] + std::fabs(xij[2 * (i - 1) + 1]) * step[1];
        if (!(r <= m)) m = r;                                        // (a NaN stays)
    }
    const double reach = std::ceil(fs * m);
    if (!(reach < REFINE_MAX_DELAY)) return -1;
    const int64_t H = (int64_t)grid_halo + (int64_t)reach + 1;
    return H < (int64_t)REFINE_MAX_DELAY ? H : -1;
}

hipError_t nbls_launch_beam_grid_refine(nbls_handle* h, int64_t u0, int64_t nu, hipStream_t st) {
    if (nu <= 0) return hipSuccess;
    const int taps = h->req.grid_taps();
    if (h->nelem > REFINE_MAX_ELEMENTS || (taps != 4 && taps != 6 && taps != 8)) return hipErrorInvalidValue;   // (nbls_plan has refused such a plan)
    const size_t cells = (size_t)h->nbands * h->vector_len;
    RArgs a{};
    a.filt = h->d_filt;
    a.npts = h->npts; a.npts_pad = h->npts_pad;
    a.N = h->nelem;
    a.Wb = h->d_W; a.incb = h->d_inc;
    a.unit_band = h->d_unit_band; a.unit_win = h->d_unit_win;
    a.vector_len = h->vector_len; a.u0 = (int)u0; a.nunits = (int)nu;
    a.halo = h->derived.grid_refine_halo;
    a.maxW = h->maxW;
    a.xij = h->est[0].d_xij;
    a.fs = h->fs;
    a.grid = h->d_grid;
    a.gindex = h->d_grid_index;
    a.gfstat = h->d_grid_fp; a.gpower = h->d_grid_fp + cells;
    a.levels = h->req.grid_refine.levels;
    a.h0 = h->req.grid_refine.step[0]; a.h1 = h->req.grid_refine.step[1];
    a.slow = h->d_grid_refine_fp; a.fstat = h->d_grid_refine_fp + 2 * cells; a.power = h->d_grid_refine_fp + 3 * cells;
    a.stencil = h->d_grid_refine_fp + 4 * cells;
    a.path = h->d_grid_refine_path;
    const size_t lds = nbls_beam_grid_refine_lds_bytes_of(h->nelem, h->maxW, h->derived.grid_refine_halo);
    if (lds) {
        const unsigned bit = 1u << (taps / 2);
        if (!(h->grid_refine_attr_set & bit)) {   // once per handle and instance (a streamed pass launches per unit batch)
            const hipError_t e = hipFuncSetAttribute(refine_kernel_of<true>(taps), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     (int)REFINE_LDS_MAX);
            if (e != hipSuccess) return e;
            h->grid_refine_attr_set |= bit;
        }
    }
    void* args[] = {&a};
    return hipLaunchKernel(lds ? refine_kernel_of<true>(taps) : refine_kernel_of<false>(taps), dim3((unsigned)nu),
                           dim3(REFINE_WAVES * 64), args, lds, st);
}
