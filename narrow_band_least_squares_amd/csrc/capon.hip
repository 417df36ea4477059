// Per-window Capon (MVDR) and Bartlett slowness spectra of the narrow band's cross-spectral matrix (nbls_set_capon;
// DESIGN.md §18).
//
// The caller gives G slowness vectors grid[G][2] (s/km, the convention of nbls_set_beam_grid), per band b a frequency f_b
// (Hz), a snapshot length Ls_b and hop Hs_b (samples), and one diagonal loading delta.  N = nelem, W the band's window.
// Once per plan, on the host in float64 (un-fused: this translation unit is built without contraction):
//   c_b[n]    = (0.5 - 0.5 cos((2 pi (n + 0.5)) / Ls)) * (cos p, sin p),  p = -(((2 pi f) n) / fs),  n < Ls
//   a_b[g][0] = 1,  a_b[g][i] = (cos q, sin q),  q = -((2 pi f) tau_i(g)),  tau_i(g) = xij[i-1][0] s_g0 + xij[i-1][1] s_g1
//   K_b       = 1 + (W - Ls) div Hs
// Per unit (result row r, window w, start s0 = w * inc[r]):
//   X_i[k] = sum_{n < Ls} c[n] filt[r][i][s0 + k Hs + n]        every index inside the window: no halo
//   R      = (1 / K) sum_k X[k] X[k]^H                          N x N Hermitian
//   t      = sum_i Re R_ii,  R' = R + delta (t / N) I
//   P_B(g) = Re(a^H R a) / N^2                                  on the unloaded R
//   R' = L L^H (Cholesky), L y = a (forward substitution), P_C(g) = 1 / |y|^2
// and the unit's results are the arg-max of either spectrum under "P descending, g ascending" (a NaN is no candidate; -1
// and NaN if there is none), on request both maps and R.  t == 0, t NaN or a NaN entry of R: every result NaN / -1.  A
// pivot that is not > 0: the Capon results NaN / -1, the Bartlett results stay.
//
// Mapping: one workgroup of CAPON_THREADS threads per unit.
//   snapshots  chunks of CAPON_CHUNK snapshots; a wave takes (snapshot, element) dots, its lanes stride n and the fixed
//              DPP tree of wave_ops.h adds them; X of the chunk goes to LDS, so no (Ls, Hs) is refused
//   R          thread e takes the entries e, e + CAPON_THREADS, ... of the lower triangle and adds the chunk's snapshots in
//              k order; the upper triangle is the conjugate, bit for bit
//   Cholesky   in LDS, thread i owns row i, one barrier per column; every thread forms the pivot itself, so the decision
//              "not > 0" is the same in all of them
//   grid       one lane per grid point.  N is a run-time value <= 32: a register array of y indexed by it would go to
//              scratch, and the full unrolling that makes every index a constant is a program of 4000 FMAs that the
//              compiler does not get through; so a (then y, in place) lives in LDS, column `lane` of Y [N][2][THREADS],
//              consecutive lanes on consecutive banks (conflict-free ds_read_b64), in the place X had.  R and L are
//              wave-uniform LDS reads (broadcast), the steering table is laid out [band][element][G] so that consecutive
//              lanes read consecutive g.  y is substituted, R'^-1 is never formed: the error of P_C grows with kappa(R'),
//              not its square.  The diagonal of L is held as its reciprocal.
//   LDS        dynamic, sized by N: R and L (N^2 complex each), N reciprocals, and max(CHUNK, THREADS) N complex for X / Y:
//              6.3 KiB at N = 3, 18 KiB at 8, 96 KiB at 32
// The order of every sum depends on (N, W, Ls, Hs, G) alone, the arg-max is a total order, there are no atomics and nothing
// depends on the launch's unit range: single, streamed, batched and window-sliced passes give the same bits.
//
// A plan with a peak request (nbls_set_capon_peaks; the definition is in include/nbls.h) runs an instance of
// the kernel that also keeps both spectra of the unit and picks the K strongest kept peaks of either behind the arg-max
// (capon_peaks_of); the instance without is the code as it was.  Where the two maps [2][G] wait:
//   LDS route  behind the kernel's own dynamic LDS
//   HBM route  in the unit's rows of the maps where the plan keeps them, else in the workgroup's slab of a scratch buffer; the
//              units go in launches of at most as many workgroups as there are slabs; the stream's order hands them on,
//              and an event where a pass solves on two streams
// Both instances run the same function on the same values (the pointer's address space is the compiler's business) and
// give the same bits; nbls_capon_peak_route_of chooses.
//
// A plan that asked for the spectra of the elements LTS kept (nbls_set_kept_elements with NBLS_KEPT_CAPON) runs
// the KEPT instances.  R is formed and written to csdm for all N elements as above; then, where the unit's dropped mask
// (kept.hip has written it on the same stream) names an element, the workgroup compacts R_K = R[e_i][e_j] through the place
// of L (free until the loading) to the head of R, row stride M, and the loading, the Cholesky factor and the grid run with
// M in the place of N (count and row stride are one value, as in the plain instance) and the steering rows e_i.  The index
// list e[] lies in LDS and is read wave-uniformly (a broadcast), so the gather of a steering row changes nothing about where
// y lives.  A unit without a dropped element takes none of this: the same bits as the plain instance.
#include "nbls_internal.h"
#include "wave_ops.h"
#include "refine_fraction.h"
#include "capon_point.h"
#include "capon_peaks.h"
#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

namespace {

using namespace nbls_capon;                  // CT, CW, capon_better, capon_best, capon_bartlett_point (capon_point.h)
constexpr int CCH = NBLS_CAPON_CHUNK;        // snapshots per chunk of X in LDS
constexpr int CMAXN = NBLS_CAPON_MAX_ELEMENTS;
constexpr int CTRI = (CMAXN * (CMAXN + 1) / 2 + CT - 1) / CT;     // lower-triangle entries per thread

struct CArgs {
    const double* filt;       // [B][nelem][npts_pad]
    int64_t npts_pad;
    int N, nseg;
    const int32_t* Wb;        // [B]
    const int32_t* incb;      // [B]
    const int32_t* unit_band; // [U]
    const int32_t* unit_win;  // [U]
    int vector_len, u0, nunits;
    int G, maxLs;
    const int32_t* par;       // [fbands][3]: Ls, Hs, K
    const double* coef;       // [fbands][maxLs][2]
    const double* steer;      // [fbands][N][G][2]
    double loading;
    int32_t* index;           // [2][B][VL]: capon | bartlett
    double* power;            // [2][B][VL]
    double* map;              // [2][B][VL][G] or NULL
    double* csdm;             // [B][VL][N][N][2] or NULL
    int64_t cells;
    // ---- the peak request (nbls_set_capon_peaks): read by the instances with peaks alone ----
    const int32_t* nbr;       // [8][G] neighbour table, -1: absent
    int pk;                   // K
    double pfloor;
    double* slab;             // HBM route without the maps: [launch's workgroups][2][G]
    int32_t* pk_count;        // [2][B][VL]
    int32_t* pk_index;        // [2][B][VL][K]
    double* pk_power;         // [2][B][VL][K]
    double* pk_offset;        // [2][B][VL][K][2]
    // ---- the elements LTS kept (nbls_set_kept_elements): read by the KEPT instances alone ----
    const uint32_t* dropped;  // [B][VL] bit m set: element m is dropped (kept.hip)
};

// doubles of the kernel's dynamic LDS without the peak maps (nbls_capon_lds_bytes_of)
__host__ __device__ inline size_t nbls_capon_lds_doubles(int nelem) {
    const size_t n = (size_t)nelem, xy = (size_t)(CCH > CT ? CCH : CT) * n * 2;
    return 2 * n * n * 2 + ((n + 1) & ~(size_t)1) + xy;
}

// ---- the K strongest peaks of one spectrum of the unit (nbls_set_capon_peaks) ----
// the peak request's results of spectrum `which` (capon_peaks.h: the picker is shared with capon_music_kernel)
__device__ inline PeakOut capon_peak_out(const CArgs& a, int which) {
    return PeakOut{a.nbr, a.G, a.pk, a.pfloor, a.pk_count + which * a.cells, a.pk_index + which * a.cells * a.pk,
                   a.pk_power + which * a.cells * a.pk, a.pk_offset + which * a.cells * a.pk * 2};
}

// The KEPT instances' index list e[] (static LDS of those instances alone: its address is a constant, not a register).
__device__ inline int* capon_kept_index() {
    __shared__ int kidx[CMAXN];
    return kidx;
}

// PK: 0 no peaks (the kernel as it was), 1 the unit's two maps in LDS behind Y, 2 in the unit's slab of HBM
// KEPT: the spectra of the elements LTS kept in this unit
template <int PK, bool KEPT>
__global__ __launch_bounds__(CT) void capon_kernel(CArgs a) {
    // dynamic LDS, sized by N (capon_lds_bytes): Rm [N][N] complex, Lm [N][N] complex, invd [N], then X [CHUNK][N] complex
    // and, in its place once R is there, Y [N][2][THREADS]: the grid phase's vector of every lane
    extern __shared__ __attribute__((aligned(16))) double capon_lds[];
    __shared__ double red_p[CW];
    __shared__ int red_g[CW];
    int SN = a.N;                                                    // row stride of Rm, Lm and X (KEPT: of R_K and its factor, once compacted)
    double* const Rm = capon_lds;
    double* const Lm = Rm + SN * SN * 2;
    double* const invd = Lm + SN * SN * 2;
    double* const X = invd + ((SN + 1) & ~1);
    double* const Y = X;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if ((int)blockIdx.x >= a.nunits) return;                         // (the same for every thread of the workgroup)
    const int u = a.u0 + blockIdx.x;
    const int row = a.unit_band[u], w = a.unit_win[u];
    const int band = row / a.nseg;
    const int N = a.N, G = a.G;
    const int Ls = a.par[3 * band], Hs = a.par[3 * band + 1], K = a.par[3 * band + 2];
    const int64_t s0 = (int64_t)w * a.incb[row];
    const int64_t cell = (int64_t)row * a.vector_len + w;
    const double* rowbase = a.filt + (int64_t)row * N * a.npts_pad + s0;
    const double* coef = a.coef + (int64_t)band * a.maxLs * 2;

    // this thread's entries of the lower triangle: e = i (i + 1) / 2 + j, j <= i
    const int ntri = N * (N + 1) / 2;
    int ei[CTRI], ej[CTRI];
    double accr[CTRI], acci[CTRI];
#pragma unroll
    for (int m = 0; m < CTRI; ++m) {
        const int e = tid + m * CT;
        int i = 0;
        while ((i + 1) * (i + 2) / 2 <= e) ++i;
        ei[m] = i; ej[m] = e - i * (i + 1) / 2;
        accr[m] = 0.0; acci[m] = 0.0;
    }
    for (int k0 = 0; k0 < K; k0 += CCH) {
        const int kc = K - k0 < CCH ? K - k0 : CCH;
        for (int item = wave; item < kc * N; item += CW) {           // (item is the same for every lane of the wave)
            const int kl = item / N, i = item - kl * N;
            const double* x = rowbase + (int64_t)i * a.npts_pad + (int64_t)(k0 + kl) * Hs;
            double sr = 0.0, si = 0.0;
            for (int n = lane; n < Ls; n += 64) {
                const double v = x[n];
                sr += coef[2 * n] * v;
                si += coef[2 * n + 1] * v;
            }
            sr = nbls_wave::sum_f64(sr);
            si = nbls_wave::sum_f64(si);
            if (lane == 0) { X[(kl * SN + i) * 2] = sr; X[(kl * SN + i) * 2 + 1] = si; }
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < CTRI; ++m) {
            if (tid + m * CT >= ntri) continue;
            const int i = ei[m], j = ej[m];
            double re = accr[m], im = acci[m];
            for (int kl = 0; kl < kc; ++kl) {                        // X_i conj(X_j)
                const double ar = X[(kl * SN + i) * 2], ai = X[(kl * SN + i) * 2 + 1];
                const double br = X[(kl * SN + j) * 2], bi = X[(kl * SN + j) * 2 + 1];
                re += ar * br;
                re += ai * bi;
                im += ai * br;
                im -= ar * bi;
            }
            accr[m] = re; acci[m] = im;
        }
        __syncthreads();
    }
    int nan_here = 0;
    const double kd = (double)K;
#pragma unroll
    for (int m = 0; m < CTRI; ++m) {
        if (tid + m * CT >= ntri) continue;
        const int i = ei[m], j = ej[m];
        const double re = accr[m] / kd, im = i == j ? 0.0 : acci[m] / kd;
        nan_here |= (re != re) || (im != im);
        Rm[(i * SN + j) * 2] = re; Rm[(i * SN + j) * 2 + 1] = im;
        Rm[(j * SN + i) * 2] = re; Rm[(j * SN + i) * 2 + 1] = -im;
    }
    const int any_nan = __syncthreads_or(nan_here);                  // (and the barrier behind the writes of Rm)
    if (a.csdm)
        for (int e = tid; e < N * N; e += CT) {
            const int i = e / N, j = e - i * N;
            a.csdm[(cell * N * N + e) * 2] = Rm[(i * SN + j) * 2];
            a.csdm[(cell * N * N + e) * 2 + 1] = Rm[(i * SN + j) * 2 + 1];
        }
    int bad_r = any_nan;
    if constexpr (KEPT) {
        int* const kidx = capon_kept_index();                        // e_i, the kept elements in ascending order
        int M;
        const uint32_t bits = nbls_kept_bits_of(a.dropped[cell], N, M);     // (the same in every thread)
        if (tid < M) {                                               // the tid-th set bit
            uint32_t b = bits;
            for (int i = 0; i < tid; ++i) b &= b - 1;
            kidx[tid] = __builtin_ctz(b);
        }
        __syncthreads();                                             // (and every thread is through with Rm -> csdm)
        if (M < N) {
            for (int e = tid; e < M * M; e += CT) {                  // R_K, row stride M, through the place of L ...
                const int i = e / M, j = e - i * M;
                const int src = kidx[i] * N + kidx[j];
                Lm[e * 2] = Rm[src * 2];
                Lm[e * 2 + 1] = Rm[src * 2 + 1];
            }
            __syncthreads();
            int nan_k = 0;
            for (int e = tid; e < M * M; e += CT) {                  // ... to the head of R
                const double re = Lm[e * 2], im = Lm[e * 2 + 1];
                nan_k |= (re != re) || (im != im);
                Rm[e * 2] = re;
                Rm[e * 2 + 1] = im;
            }
            bad_r = __syncthreads_or(nan_k);                         // (a NaN entry of R_K; and the barrier behind the writes)
            SN = M;                                                  // from here on: M elements, rows of M
        }
    }
    double t = 0.0;
    for (int i = 0; i < SN; ++i) t += Rm[(i * SN + i) * 2];       // (every thread, the same order)
    const double nan_ = __builtin_nan("");
    if (bad_r || t == 0.0 || t != t) {
        if (a.map)
            for (int g = tid; g < G; g += CT) { a.map[cell * G + g] = nan_; a.map[(a.cells + cell) * G + g] = nan_; }
        if (tid == 0) {
            a.index[cell] = -1; a.index[a.cells + cell] = -1;
            a.power[cell] = nan_; a.power[a.cells + cell] = nan_;
        }
        if (PK) { capon_peaks_none(capon_peak_out(a, 0), cell, tid); capon_peaks_none(capon_peak_out(a, 1), cell, tid); }
        return;
    }
    // R' = R + delta (t / N) I, then its Cholesky factor column by column
    const double lam = a.loading * (t / (double)SN);
    for (int e = tid; e < SN * SN; e += CT) {
        const int i = e / SN, j = e - i * SN;
        Lm[(i * SN + j) * 2] = Rm[(i * SN + j) * 2] + (i == j ? lam : 0.0);
        Lm[(i * SN + j) * 2 + 1] = Rm[(i * SN + j) * 2 + 1];
    }
    __syncthreads();
    bool chol_ok = true;
    for (int j = 0; j < SN; ++j) {
        double d = Lm[(j * SN + j) * 2];
        for (int k = 0; k < j; ++k) {
            const double lr = Lm[(j * SN + k) * 2], li = Lm[(j * SN + k) * 2 + 1];
            d -= lr * lr;
            d -= li * li;
        }
        if (!(d > 0.0)) { chol_ok = false; break; }                  // (the same d in every thread)
        const double ljj = sqrt(d);
        if (tid == j) invd[j] = 1.0 / ljj;
        if (tid > j && tid < SN) {
            double sr = Lm[(tid * SN + j) * 2], si = Lm[(tid * SN + j) * 2 + 1];
            for (int k = 0; k < j; ++k) {                            // L_ik conj(L_jk)
                const double ar = Lm[(tid * SN + k) * 2], ai = Lm[(tid * SN + k) * 2 + 1];
                const double br = Lm[(j * SN + k) * 2], bi = Lm[(j * SN + k) * 2 + 1];
                sr -= ar * br;
                sr -= ai * bi;
                si -= ai * br;
                si += ar * bi;
            }
            Lm[(tid * SN + j) * 2] = sr / ljj;
            Lm[(tid * SN + j) * 2 + 1] = si / ljj;
        }
        __syncthreads();
    }
    // the grid: one lane per point, its vector in LDS column tid of Y (consecutive lanes, consecutive banks)
    const double2* steer = (const double2*)a.steer + (int64_t)band * N * G;
    const double2* R2 = (const double2*)Rm;
    const double2* L2 = (const double2*)Lm;
    double* const yr = Y + tid;                                      // y_i = (yr[i * 2 CT], yr[i * 2 CT + CT])
    const double nn = (double)SN * (double)SN;
    double bc = 0.0, bb = 0.0;
    int gc = -1, gb = -1;
    // with peaks: where the unit's two spectra stay until they are picked
    double* mc = nullptr;
    double* mb = nullptr;
    if (PK == 1) {
        mc = capon_lds + nbls_capon_lds_doubles(N);
        mb = mc + G;
    } else if (PK == 2) {
        mc = a.map ? a.map + cell * G : a.slab + (int64_t)blockIdx.x * 2 * G;
        mb = a.map ? a.map + (a.cells + cell) * G : mc + G;
    }
    for (int g = tid; g < G; g += CT) {
        for (int i = 0; i < SN; ++i) {
            int er = i;                                              // the element's row of the steering table
            if constexpr (KEPT) er = capon_kept_index()[i];          // (a wave-uniform LDS read)
            const double2 v = steer[(int64_t)er * G + g];
            yr[i * 2 * CT] = v.x; yr[i * 2 * CT + CT] = v.y;
        }
        // Bartlett: sum_i R_ii |a_i|^2 + 2 Re(conj(a_i) sum_{j<i} R_ij a_j)
        const double pb = capon_bartlett_point(R2, yr, SN, nn);
        // Capon: y in place of a
        double pc = nan_;
        if (chol_ok) {
            double q = 0.0;
            for (int i = 0; i < SN; ++i) {
                double sr = yr[i * 2 * CT], si = yr[i * 2 * CT + CT];
                for (int j = 0; j < i; ++j) {
                    const double2 l = L2[i * SN + j];
                    const double vr = yr[j * 2 * CT], vi = yr[j * 2 * CT + CT];
                    sr = __builtin_fma(-l.x, vr, sr);
                    sr = __builtin_fma(l.y, vi, sr);
                    si = __builtin_fma(-l.x, vi, si);
                    si = __builtin_fma(-l.y, vr, si);
                }
                const double id = invd[i];
                sr *= id; si *= id;
                yr[i * 2 * CT] = sr; yr[i * 2 * CT + CT] = si;
                q = __builtin_fma(sr, sr, q);
                q = __builtin_fma(si, si, q);
            }
            pc = 1.0 / q;
        }
        if (a.map) { a.map[cell * G + g] = pc; a.map[(a.cells + cell) * G + g] = pb; }
        if (PK == 1 || (PK == 2 && !a.map)) { mc[g] = pc; mb[g] = pb; }
        if (capon_better(pc, g, bc, gc)) { bc = pc; gc = g; }
        if (capon_better(pb, g, bb, gb)) { bb = pb; gb = g; }
    }
    capon_best(bc, gc, red_p, red_g, tid);
    capon_best(bb, gb, red_p, red_g, tid);
    if (tid == 0) {
        a.index[cell] = gc; a.index[a.cells + cell] = gb;
        a.power[cell] = gc < 0 ? nan_ : bc;
        a.power[a.cells + cell] = gb < 0 ? nan_ : bb;
    }
    if (PK) {
        // the maps are this workgroup's own writes: a fence and a barrier make them its reads (capon_best has given the
        // barrier already; the fence is for the slab)
        if (PK == 2) __threadfence_block();
        __syncthreads();
        capon_peaks_of(capon_peak_out(a, 0), mc, cell, gc < 0 ? nan_ : bc, gc, red_p, red_g, tid);
        capon_peaks_of(capon_peak_out(a, 1), mb, cell, gb < 0 ? nan_ : bb, gb, red_p, red_g, tid);
    }
}

}  // namespace

// dynamic LDS bytes of capon_kernel for an array of nelem elements (see the kernel's head)
size_t nbls_capon_lds_bytes_of(int nelem) {
    return nbls_capon_lds_doubles(nelem) * sizeof(double);
}

// ... and of the instance that keeps the unit's two maps of G points in LDS behind it (0: more than a workgroup's 160 KiB,
// less the kernel's static arrays)
size_t nbls_capon_peak_lds_bytes_of(int nelem, int G) {
    const size_t b = nbls_capon_lds_bytes_of(nelem) + (size_t)2 * (size_t)G * sizeof(double);
    return b + 1024 <= (size_t)160 * 1024 ? b : 0;
}

// The automatic route of a plan with a peak request: 1 (LDS) or 2 (HBM).  A workgroup is two waves of 96 VGPRs, so a CU
// holds 10 of them at most, and fewer where the dynamic LDS says so (8 at N = 8).  The maps in LDS take that down further
// (4 at N = 8, G = 1257), and at cfg-3 that costs more than the slab's trip through the vector cache and L2: the peaks add
// 6.5 ms to the pass on the LDS route and 3.2 ms on the HBM route.  So the LDS route is taken only
// where the maps fit without lowering the workgroups per CU (large arrays, whose own LDS leaves one or two per CU anyway).
int nbls_capon_peak_route_of(int nelem, int G) {
    const size_t with = nbls_capon_peak_lds_bytes_of(nelem, G);
    if (!with) return 2;
    const size_t cu = (size_t)160 * 1024, fixed = 1024, most = 10;
    const size_t before = std::min(most, cu / (nbls_capon_lds_bytes_of(nelem) + fixed));
    const size_t after = std::min(most, cu / (with + fixed));
    return after == before ? 1 : 2;
}

// The neighbour table [8][G] of the lattice cells cell [G][2] (distinct, 0 <= c < 32768), in the order (-1,0), (+1,0),
// (0,-1), (0,+1), (-1,-1), (-1,+1), (+1,-1), (+1,+1); -1 where there is no such point.
void nbls_capon_neighbours_of(const int32_t* cell, int G, int32_t* nbr) {
    static const int di[8] = {-1, 1, 0, 0, -1, -1, 1, 1}, dj[8] = {0, 0, -1, 1, -1, 1, -1, 1};
    std::vector<std::pair<int32_t, int32_t>> key((size_t)G);       // (i * 32768 + j, g), sorted
    for (int g = 0; g < G; ++g) key[g] = {cell[2 * g] * 32768 + cell[2 * g + 1], g};
    std::sort(key.begin(), key.end());
    for (int g = 0; g < G; ++g)
        for (int d = 0; d < 8; ++d) {
            const int i = cell[2 * g] + di[d], j = cell[2 * g + 1] + dj[d];
            int32_t n = -1;
            if (i >= 0 && i < 32768 && j >= 0 && j < 32768) {
                const auto it = std::lower_bound(key.begin(), key.end(), std::make_pair((int32_t)(i * 32768 + j), (int32_t)-1));
                if (it != key.end() && it->first == i * 32768 + j) n = it->second;
            }
            nbr[(size_t)d * G + g] = n;
        }
}

// The plan's tables on the host, float64, un-fused (see the head of this file).  coef [nbands][maxLs][2] (zeros beyond
// Ls_b), steer [nbands][nelem][G][2].
void nbls_capon_tables_of(const double* xij, int nelem, double fs, const double* grid, int G, const double* freq,
                          const int32_t* snap_len, int nbands, int maxLs, double* coef, double* steer) {
    const double two_pi = 2.0 * M_PI;
    for (int b = 0; b < nbands; ++b) {
        const double wf = two_pi * freq[b];
        const int Ls = snap_len[b];
        double* c = coef + (size_t)b * maxLs * 2;
        for (int n = 0; n < maxLs; ++n) {
            if (n >= Ls) { c[2 * n] = 0.0; c[2 * n + 1] = 0.0; continue; }
            const double hann = 0.5 - 0.5 * std::cos((two_pi * ((double)n + 0.5)) / (double)Ls);
            const double p = -((wf * (double)n) / fs);
            c[2 * n] = hann * std::cos(p);
            c[2 * n + 1] = hann * std::sin(p);
        }
        double* s = steer + (size_t)b * nelem * G * 2;
        for (int g = 0; g < G; ++g) {
            const double s0 = grid[2 * g], s1 = grid[2 * g + 1];
            s[2 * g] = 1.0; s[2 * g + 1] = 0.0;
            for (int i = 1; i < nelem; ++i) {
                const double tau = xij[2 * (i - 1)] * s0 + xij[2 * (i - 1) + 1] * s1;
                const double q = -(wf * tau);
                s[((size_t)i * G + g) * 2] = std::cos(q);
                s[((size_t)i * G + g) * 2 + 1] = std::sin(q);
            }
        }
    }
}

hipError_t nbls_launch_capon(nbls_handle* h, int64_t u0, int64_t nu, hipStream_t st) {
    if (nu <= 0) return hipSuccess;
    if (h->nelem > CMAXN || h->nelem < 1) return hipErrorInvalidValue;   // (nbls_plan has refused such a plan)
    CArgs a{};
    a.filt = h->d_filt;
    a.npts_pad = h->npts_pad;
    a.N = h->nelem; a.nseg = h->nbands / h->fbands;      // result row r is band r / nseg
    a.Wb = h->d_W; a.incb = h->d_inc;
    a.unit_band = h->d_unit_band; a.unit_win = h->d_unit_win;
    a.vector_len = h->vector_len; a.u0 = (int)u0; a.nunits = (int)nu;
    a.G = h->derived.capon_n; a.maxLs = h->derived.capon_maxls;
    a.par = h->d_capon_par; a.coef = h->d_capon_coef; a.steer = h->d_capon_steer;
    a.loading = h->req.capon.loading;
    a.cells = (int64_t)h->nbands * h->vector_len;
    a.index = h->d_capon_index; a.power = h->d_capon_power;
    a.map = h->req.capon_maps() ? h->d_capon_map.p : nullptr;
    a.csdm = (h->req.capon_csdm() || h->req.clean.iterations > 0 || h->req.music.sources >= 0) ? h->d_capon_csdm.p : nullptr;     // (capon_clean_kernel and capon_music_kernel read R there)
    const size_t lds = nbls_capon_lds_bytes_of(h->nelem);
    const bool kept = h->req.kept_capon();       // the spectra of the elements LTS kept (nbls_set_kept_elements): the KEPT instances
    if (kept) {
        if (!h->d_kept_mask) return hipErrorInvalidValue;                // (nbls_plan has refused such a plan)
        a.dropped = h->d_kept_mask;
    }
    // instance PK of the plan, given its dynamic LDS limit `limit` once per handle
    const auto instance = [&](int pk, int limit, const void** fn) -> hipError_t {
        static const void* const table[2][3] = {
            {(const void*)capon_kernel<0, false>, (const void*)capon_kernel<1, false>, (const void*)capon_kernel<2, false>},
            {(const void*)capon_kernel<0, true>, (const void*)capon_kernel<1, true>, (const void*)capon_kernel<2, true>}};
        *fn = table[kept][pk];
        bool& set = kept ? h->capon_kept_attr_set[pk] : (pk == 0 ? h->capon_attr_set : h->capon_peak_attr_set[pk - 1]);
        if (set) return hipSuccess;
        const hipError_t e = hipFuncSetAttribute(*fn, hipFuncAttributeMaxDynamicSharedMemorySize, limit);
        if (e == hipSuccess) set = true;
        return e;
    };
    const auto run = [&](const void* fn, unsigned nblocks, size_t shm) -> hipError_t {
        void* params[] = {(void*)&a};
        return hipLaunchKernel(fn, dim3(nblocks), dim3(CT), params, shm, st);
    };
    const void* fn = nullptr;
    if (h->req.peaks.k > 0) {              // a plan with a peak request (nbls_set_capon_peaks)
        a.nbr = h->d_capon_nbr; a.pk = h->req.peaks.k; a.pfloor = h->req.peaks.floor;
        a.pk_count = h->d_capon_peak_count; a.pk_index = h->d_capon_peak_index;
        a.pk_power = h->d_capon_peak_power; a.pk_offset = h->d_capon_peak_offset;
        if (h->derived.peak_route == 1) {
            const size_t plds = nbls_capon_peak_lds_bytes_of(h->nelem, h->derived.capon_n);
            if (!plds) return hipErrorInvalidValue;                      // (nbls_plan has refused such a plan)
            const hipError_t e = instance(1, 160 * 1024 - 1024, &fn);
            if (e != hipSuccess) return e;
            return run(fn, (unsigned)nu, plds);
        }
        {
            const hipError_t e = instance(2, (int)nbls_capon_lds_bytes_of(CMAXN), &fn);
            if (e != hipSuccess) return e;
        }
        // the maps of a unit lie in its own rows of d_capon_map where the plan keeps them; else in the slab of its
        // workgroup: at most capon_peak_slabs workgroups per launch.  On one stream its order hands the slabs on; the
        // solves of a pass may be on two (solve_on_stream2), so a launch on the other stream than the last one waits
        // for that one's event first
        a.slab = a.map ? nullptr : h->d_capon_peak_slab.p;
        if (a.slab) {
            if (!h->ev_capon_slab) {
                const hipError_t e = hipEventCreateWithFlags(&h->ev_capon_slab, hipEventDisableTiming);
                if (e != hipSuccess) { h->ev_capon_slab = nullptr; return e; }
            }
            if (h->capon_slab_stream && h->capon_slab_stream != st) {
                const hipError_t e = hipStreamWaitEvent(st, h->ev_capon_slab, 0);
                if (e != hipSuccess) return e;
            }
        }
        const int64_t step = a.map ? nu : h->derived.peak_slabs;
        for (int64_t o = 0; o < nu; o += step) {
            a.u0 = (int)(u0 + o);
            a.nunits = (int)(nu - o < step ? nu - o : step);
            const hipError_t e = run(fn, (unsigned)a.nunits, lds);
            if (e != hipSuccess) return e;
        }
        if (a.slab) {
            const hipError_t e = hipEventRecord(h->ev_capon_slab, st);
            if (e != hipSuccess) return e;
            h->capon_slab_stream = st;
        }
        return hipSuccess;
    }
    const hipError_t e = instance(0, (int)nbls_capon_lds_bytes_of(CMAXN), &fn);      // once per handle (a streamed pass launches per unit batch)
    if (e != hipSuccess) return e;
    return run(fn, (unsigned)nu, lds);
}
