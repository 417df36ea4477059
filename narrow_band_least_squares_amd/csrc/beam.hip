// Beam power and Fisher F-statistic of the delay-and-sum beam at the solved slowness (nbls_set_beam).
//
// Per unit (result row r, window w, start s0 = w * inc[r], length W) and estimator with elements e_0 < ... < e_{N-1}:
//   d_0 = 0,  d_i = rint(fs * (xij[i-1][0] * z0 + xij[i-1][1] * z1))     pair (0, i) is pair i - 1 of the estimator's list
//   x_i[t] = filt[r][e_i][s0 + t + d_i], 0.0 outside [0, npts)           (the padding up to npts_pad is never data)
//   b[t] = sum_i x_i[t],  S_b = sum_t b[t]^2,  S_t = sum_t sum_i x_i[t]^2,  D = N S_t - S_b
//   beam_power = S_b / (N^2 W),  fstat = (N - 1) S_b / D
// The measured lag of pair (0, i) is W-1-argmax of np.correlate(x_0, x_i, 'full'): x_i[n] ~ x_0[n - lag], element i lags
// element 0 by d_i samples, so reading element i at +d_i lines it up with element 0.
//
// Mapping: a workgroup of four waves takes four consecutive units.  A unit of at most BEAM_WAVE_W samples is summed by
// ONE wave (wave j of the workgroup takes unit j), a longer one by all four waves, one unit after the other.  The lanes
// stride over t — consecutive lanes read consecutive samples of a channel row — and loop over the elements; every lane
// keeps its own two sums in t order, the wave adds them with the fixed DPP tree of wave_ops.h, the four waves of a long
// unit are added in wave order through LDS.  The order of every sum depends on (N, W) alone: no atomics, and nothing
// depends on the launch's unit range, so single, batched and streamed passes give the same bits.
//
// A plan that asked for the beam of the elements LTS kept (nbls_set_kept_elements with NBLS_KEPT_BEAM) runs the
// KEPT instance: "lane i holds e_i and d_i" is filled per unit instead of per launch, from the unit's dropped mask
// (kept.hip has written it on the same stream): e_i is the i-th set bit of the kept bits, the reference element is e_0 and
// d_i comes from the co-array row of pair (e_0, e_i).  The element count of the unit's sums and of its F is M; beam_sums is
// the same function.  A unit without a dropped element fills the registers as the plain instance does: the same bits.
//
// A plan that asked for fractional-sample steering (nbls_set_beam_interpolation) runs the TAPS = 4, 6 or 8
// instances (built from this file by beam_steer.hip, a translation unit of their own: this one holds the two whole-sample
// instances and their launch, as it did): lane i holds n_i = floor(tau_i) where it held d_i, and the TAPS Lagrange
// coefficients of mu_i = tau_i - n_i in registers of its own; the element loop reads them back with readlane (two halves
// per double: SGPR pairs, no LDS, no private segment) and forms x_i[t] from TAPS samples.  Everything behind x_i[t] is the
// code of the TAPS = 0 instances.
#include "nbls_internal.h"
#include "steer.h"
#include "wave_ops.h"

namespace {

constexpr int BEAM_WAVES = 4;
constexpr int BEAM_WAVE_W = 512;         // windows up to this length: one wave per unit
constexpr double BEAM_MAX_DELAY = 1073741824.0;   // 2^30 samples: beyond, the unit's results are NaN
// Lane i of a wave holds d_i and the row of element i, read back with readlane: an estimator has at most 64 elements.
// The plan's pair limit keeps every array below that (65 elements are 2080 pairs); nbls_launch_beam checks it again.
constexpr int BEAM_MAX_ELEMENTS = 64;
static_assert((BEAM_MAX_ELEMENTS + 1) * BEAM_MAX_ELEMENTS / 2 > NBLS_MAX_PAIRS,
              "beam_fstat_kernel keeps one element per lane: split the delays over several registers before lifting the pair limit");

struct BArgs {
    const double* filt;       // [B][nelem][npts_pad]
    int64_t npts, npts_pad;
    int nelem;                // rows per result row
    int N;                    // elements of this estimator
    const int32_t* kept;      // [N] their rows, NULL: all of them (N == nelem)
    const double* xij;        // [P'][2] the estimator's co-array
    const double* z;          // [B][VL][2]
    double fs;
    const int32_t* Wb;        // [B]
    const int32_t* incb;      // [B]
    const int32_t* unit_band; // [U]
    const int32_t* unit_win;  // [U]
    int vector_len, u0, nunits;
    double* power;            // [B][VL]
    double* fstat;            // [B][VL]
    const uint32_t* dropped;  // [B][VL] the KEPT instance: bit m set, element m is dropped (kept.hip)
};

// The sums of the samples t = tl, tl + STRIDE, ... of one unit.  d_mine / el_mine: lane i < n holds d_i and e_i.  Four
// samples of a lane go through the element loop together (four independent loads in flight per element); their squares
// are added in t order, so the unrolling does not show in the result.
constexpr int BEAM_TU = 4;
template <int STRIDE>
__device__ inline void beam_sums(const BArgs& a, const double* rowbase, int64_t s0, int W, int d_mine, int el_mine, int n, int tl,
                                 double& sb, double& st) {
    for (int t = tl; t < W; t += BEAM_TU * STRIDE) {
        double b[BEAM_TU], q[BEAM_TU];
#pragma unroll
        for (int k = 0; k < BEAM_TU; ++k) { b[k] = 0.0; q[k] = 0.0; }
        for (int i = 0; i < n; ++i) {
            const int d = __builtin_amdgcn_readlane(d_mine, i), el = __builtin_amdgcn_readlane(el_mine, i);
            const double* row = rowbase + (int64_t)el * a.npts_pad;
#pragma unroll
            for (int k = 0; k < BEAM_TU; ++k) {
                const int tk = t + k * STRIDE;
                const int64_t idx = s0 + tk + d;
                double v = 0.0;
                if (tk < W && idx >= 0 && idx < a.npts) v = row[idx];
                b[k] += v;
                q[k] += v * v;
            }
        }
#pragma unroll
        for (int k = 0; k < BEAM_TU; ++k) {      // (samples beyond the window contributed zeros)
            sb += b[k] * b[k];
            st += q[k];
        }
    }
}

// beam_sums with x_i[t] interpolated at tau_i = n_i + mu_i (steer.h): n_mine / c_mine[j]: lane i < n holds n_i and
// c_{j-K+1}(mu_i).  x = ((0.0 + c y) + c y) + ..., the taps ascending, every product rounded before its addition; a tap
// outside the trace (or a sample beyond the window) reads 0.0 and is still multiplied.  The TAPS loads of a sample and the
// four samples of a lane are independent of each other.
template <int STRIDE, int TAPS>
__device__ inline void beam_sums_steer(const BArgs& a, const double* rowbase, int64_t s0, int W, int n_mine, const double* c_mine,
                                       int el_mine, int n, int tl, double& sb, double& st) {
    for (int t = tl; t < W; t += BEAM_TU * STRIDE) {
        double b[BEAM_TU], q[BEAM_TU];
#pragma unroll
        for (int k = 0; k < BEAM_TU; ++k) { b[k] = 0.0; q[k] = 0.0; }
        for (int i = 0; i < n; ++i) {
            const int d = __builtin_amdgcn_readlane(n_mine, i) - (TAPS / 2 - 1), el = __builtin_amdgcn_readlane(el_mine, i);
            double c[TAPS];
#pragma unroll
            for (int j = 0; j < TAPS; ++j) c[j] = nbls_wave::readlane_f64(c_mine[j], i);
            const double* row = rowbase + (int64_t)el * a.npts_pad;
#pragma unroll
            for (int k = 0; k < BEAM_TU; ++k) {
                const int tk = t + k * STRIDE;
                const int64_t idx = s0 + tk + d;                 // the sample of tap -K+1
                double y[TAPS];
#pragma unroll
                for (int j = 0; j < TAPS; ++j) {
                    const int64_t at_j = idx + j;                // (an unconditional load of a safe index and a select:
                    const bool in = tk < W && at_j >= 0 && at_j < a.npts;    //  4 x TAPS divergent branches would cost registers)
                    const double yy = row[in ? at_j : 0];
                    y[j] = in ? yy : 0.0;
                }
                double v = 0.0;
#pragma unroll
                for (int j = 0; j < TAPS; ++j) v = v + c[j] * y[j];
                b[k] += v;
                q[k] += v * v;
            }
        }
#pragma unroll
        for (int k = 0; k < BEAM_TU; ++k) {
            sb += b[k] * b[k];
            st += q[k];
        }
    }
}

// lane's own delay: the whole-sample instances round tau, the interpolated ones split it (c: TAPS registers, 1 if TAPS == 0)
template <int TAPS>
__device__ inline void beam_delay_of(double tau, int& d_mine, double* c_mine) {
    if constexpr (TAPS == 0) d_mine = (int)rint(tau);
    else {
        double mu;
        nbls_steer_split(tau, d_mine, mu);
        nbls_steer_coefficients<TAPS>(mu, c_mine);
    }
}

__device__ inline void beam_store(const BArgs& a, int64_t cell, int W, int nel, bool bad, double sb, double st) {
    const double n = (double)nel, nan_ = __builtin_nan("");
    double p, f;
    if (bad) { p = nan_; f = nan_; }
    else if (st == 0.0) { p = 0.0; f = nan_; }
    else {
        const double dd = n * st - sb;
        p = sb / (n * n * (double)W);
        f = (dd <= 0.0 && sb > 0.0) ? __builtin_inf() : (n - 1.0) * sb / dd;
    }
    a.power[cell] = p;
    a.fstat[cell] = f;
}

template <bool KEPT, int TAPS>
__global__ __launch_bounds__(BEAM_WAVES * 64) void beam_fstat_kernel(BArgs a) {
    __shared__ double red[2 * BEAM_WAVES];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int base = blockIdx.x * BEAM_WAVES;
    for (int j = 0; j < BEAM_WAVES; ++j) {
        const int ul = base + j;
        if (ul >= a.nunits) break;                               // (the same for every thread of the workgroup)
        const int u = a.u0 + ul;
        const int row = a.unit_band[u], w = a.unit_win[u];
        const int W = a.Wb[row];
        const bool coop = W > BEAM_WAVE_W;                       // ... and so is this: the barriers below are uniform
        if (!coop && wave != j) continue;
        const int64_t s0 = (int64_t)w * a.incb[row];
        const int64_t cell = (int64_t)row * a.vector_len + w;
        // the delays, once per unit (every wave of a long unit works them out for itself: N loads)
        const double z0 = a.z[2 * cell], z1 = a.z[2 * cell + 1];
        bool bad_l = !nbls_wave::finite_f64(z0) || !nbls_wave::finite_f64(z1);
        int d_mine = 0, el_mine = 0;
        double c_mine[TAPS ? TAPS : 1];                          // (TAPS > 0: the element's coefficients; tau = 0 is mu = 0)
        if constexpr (TAPS > 0) nbls_steer_coefficients<TAPS>(0.0, c_mine);
        int n = a.N;                                             // elements of this unit's sums
        if (KEPT) {
            // the unit's kept elements (the full array, est[0]: a.kept is NULL and N <= 32): lane i < M takes the i-th set
            // bit of the kept bits and the co-array row of pair (e_0, e_i) of the full lexicographic list
            const uint32_t bits = nbls_kept_bits_of(a.dropped[cell], a.N, n);
            const int e0 = __builtin_ctz(bits);
            uint32_t b = bits;
            for (int i = 0; i < n; ++i) {                        // (n and bits are the same in every lane)
                if (i == lane) el_mine = __builtin_ctz(b);
                b &= b - 1;
            }
            if (lane > 0 && lane < n) {
                const int k = e0 * (2 * a.N - e0 - 1) / 2 + (el_mine - e0 - 1);
                const double tau = a.fs * (a.xij[2 * k] * z0 + a.xij[2 * k + 1] * z1);
                if (fabs(tau) < BEAM_MAX_DELAY) beam_delay_of<TAPS>(tau, d_mine, c_mine);
                else bad_l = true;                               // (NaN too)
            }
        } else if (lane < a.N) {                                 // N <= 64 = BEAM_MAX_ELEMENTS: one element per lane
            el_mine = a.kept ? a.kept[lane] : lane;
            if (lane > 0) {
                const double tau = a.fs * (a.xij[2 * (lane - 1)] * z0 + a.xij[2 * (lane - 1) + 1] * z1);
                if (fabs(tau) < BEAM_MAX_DELAY) beam_delay_of<TAPS>(tau, d_mine, c_mine);
                else bad_l = true;                               // (NaN too)
            }
        }
        const bool bad = __any(bad_l) != 0;
        const double* rowbase = a.filt + (int64_t)row * a.nelem * a.npts_pad;
        double sb = 0.0, st = 0.0;
        if constexpr (TAPS > 0) {
            if (coop) beam_sums_steer<BEAM_WAVES * 64, TAPS>(a, rowbase, s0, W, d_mine, c_mine, el_mine, n, tid, sb, st);
            else beam_sums_steer<64, TAPS>(a, rowbase, s0, W, d_mine, c_mine, el_mine, n, lane, sb, st);
        } else if (coop) beam_sums<BEAM_WAVES * 64>(a, rowbase, s0, W, d_mine, el_mine, n, tid, sb, st);
        else beam_sums<64>(a, rowbase, s0, W, d_mine, el_mine, n, lane, sb, st);
        sb = nbls_wave::sum_f64(sb);
        st = nbls_wave::sum_f64(st);
        if (!coop) {
            if (lane == 0) beam_store(a, cell, W, n, bad, sb, st);
            continue;
        }
        if (lane == 0) { red[wave] = sb; red[BEAM_WAVES + wave] = st; }
        __syncthreads();
        if (tid == 0) {
            sb = (red[0] + red[1]) + (red[2] + red[3]);
            st = (red[BEAM_WAVES] + red[BEAM_WAVES + 1]) + (red[BEAM_WAVES + 2] + red[BEAM_WAVES + 3]);
            beam_store(a, cell, W, n, bad, sb, st);
        }
        __syncthreads();
    }
}

}  // namespace

#ifdef NBLS_BEAM_STEER
// the interpolated instances (beam_steer.hip): args is the BArgs nbls_launch_beam below has filled; taps 4, 6 or 8
namespace {
template <bool KEPT>
void steer_launch(int taps, dim3 grid, dim3 block, hipStream_t st, const BArgs& a) {
    switch (taps) {
    case 4: hipLaunchKernelGGL((beam_fstat_kernel<KEPT, 4>), grid, block, 0, st, a); break;
    case 6: hipLaunchKernelGGL((beam_fstat_kernel<KEPT, 6>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((beam_fstat_kernel<KEPT, 8>), grid, block, 0, st, a); break;
    }
}
}  // namespace

hipError_t nbls_launch_beam_steer(int taps, bool kept, dim3 grid, dim3 block, hipStream_t st, const void* args) {
    const BArgs& a = *(const BArgs*)args;
    if (kept) steer_launch<true>(taps, grid, block, st, a);
    else steer_launch<false>(taps, grid, block, st, a);
    return hipGetLastError();
}
#else
hipError_t nbls_launch_beam(nbls_handle* h, const nbls_estimator& s, int64_t u0, int64_t nu, hipStream_t st) {
    if (nu <= 0) return hipSuccess;
    const size_t cells = (size_t)h->nbands * h->vector_len;
    BArgs a{};
    a.filt = h->d_filt;
    a.npts = h->npts; a.npts_pad = h->npts_pad;
    a.nelem = h->nelem;
    a.N = s.kept.empty() ? h->nelem : (int)s.kept.size();
    if (a.N > BEAM_MAX_ELEMENTS) return hipErrorInvalidValue;   // one element per lane (see BEAM_MAX_ELEMENTS)
    a.kept = s.kept.empty() ? nullptr : (const int32_t*)s.d_kept;
    a.xij = s.d_xij;
    a.z = s.d_z;
    a.fs = h->fs;
    a.Wb = h->d_W; a.incb = h->d_inc;
    a.unit_band = h->d_unit_band; a.unit_win = h->d_unit_win;
    a.vector_len = h->vector_len; a.u0 = (int)u0; a.nunits = (int)nu;
    a.power = s.d_beam; a.fstat = s.d_beam + cells;
    const dim3 grid((unsigned)((nu + BEAM_WAVES - 1) / BEAM_WAVES)), block(BEAM_WAVES * 64);
    if (h->req.kept_beam() && &s == &h->est[0]) {                     // the beam of the elements LTS kept (nbls_set_kept_elements)
        if (a.kept || a.N > 32 || !h->d_kept_mask) return hipErrorInvalidValue;   // (nbls_plan has refused such a plan)
        a.dropped = h->d_kept_mask;
        if (h->req.steer_taps) return nbls_launch_beam_steer(h->req.steer_taps, true, grid, block, st, &a);
        hipLaunchKernelGGL((beam_fstat_kernel<true, 0>), grid, block, 0, st, a);
    } else {
        if (h->req.steer_taps) return nbls_launch_beam_steer(h->req.steer_taps, false, grid, block, st, &a);
        hipLaunchKernelGGL((beam_fstat_kernel<false, 0>), grid, block, 0, st, a);
    }
    return hipGetLastError();
}
#endif
