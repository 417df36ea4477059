// A window's eigenvalues and its MUSIC pseudo-spectrum from the narrow band's cross-spectral matrix (nbls_set_capon_music;
// DESIGN.md §25; the definition is in include/nbls.h and this kernel follows it literally).
//
// Per unit, from the R that capon_kernel has just written to the plan's csdm buffer on the same stream: a cyclic Jacobi
// eigen-decomposition of R in LDS (round-robin tournament order, stable rotations), the eigenvalues sorted under a total
// order, the number of sources M, and one scan of the grid with the noise subspace: D(g) = sum_{k > M} |e_k^H a(g)|^2 / N,
// P(g) = 1 / D(g).
//
// Mapping: one workgroup of CAPON_THREADS threads per unit, the unit range of nbls_launch_capon.
//   R        read from HBM into A in LDS once; E = I beside it
//   step     threads r < ceil(N / 2) own the step's pairs: each forms (c, sigma, t |a_pq|) of its pair from the same LDS
//            values; a barrier; the 2 x 2 blocks of J^H A J on and above the block diagonal go by ownership (block b of
//            thread b, b + THREADS), each reading and writing its own four entries and their mirrors, and the column pairs
//            of E J by (row, pair) ownership; a second barrier.  The rotated entry is stored as 0, the diagonal real, the
//            mirror as the conjugate: the matrix stays Hermitian bit for bit
//   stop     before every sweep every thread forms off(A)^2 from the same LDS values in the same order: one decision
//   sort     thread i < N ranks lambda_i among all under "value descending, index ascending"
//   scan     one lane per grid point, the lane's a in its column of Y [N][2][THREADS] (consecutive lanes on consecutive
//            banks), E read wave-uniformly.  No register array is indexed by N
//   arg-max  capon_better / capon_best (capon_point.h)
//   peaks    (NBLS_MUSIC_PEAKS, the PK instance) the map is complete in the unit's row of the map buffer where the plan keeps
//            maps, else in the workgroup's slab of HBM [launch's workgroups][G]: one route; the picker is capon_kernel's own
//            (capon_peaks.h) behind a fence and a barrier
//   LDS      dynamic, (4 N^2 + 2 THREADS N + 4 N + 4) doubles (nbls_capon_music_lds_bytes_of): A, E, Y, the step's
//            rotations, lambda and the order
// No atomics, every order total, nothing depends on the launch's unit range.  Results leave by plain vector stores.
#include "nbls_internal.h"
#include "capon_point.h"
#include "capon_peaks.h"

namespace {

using namespace nbls_capon;
constexpr int CMAXN = NBLS_CAPON_MAX_ELEMENTS;
constexpr int MHALF = (CMAXN + 1) / 2;                               // pairs of a step at most
constexpr int MBLK = (MHALF * (MHALF + 1) / 2 + CT - 1) / CT;        // 2 x 2 blocks per thread
constexpr int SWEEP_CAP = NBLS_MUSIC_SWEEP_CAP;

struct MUArgs {
    const int32_t* unit_band; // [U]
    const int32_t* unit_win;  // [U]
    int vector_len, u0, nunits;
    int N, nseg, G;
    const double* steer;      // [fbands][N][G][2]
    const double* csdm;       // [B][VL][N][N][2]: R of every unit (capon_kernel)
    int sources;              // M, or 0: by the floor
    double eig_floor;         // rho
    double* eigenvalues;      // [B][VL][N]
    int32_t* nsrc;            // [B][VL]
    int32_t* sweeps;          // [B][VL]
    int32_t* index;           // [B][VL]
    double* power;            // [B][VL]
    double* map;              // [B][VL][G] or NULL
    double* vectors;          // [B][VL][N][N][2] or NULL
    // ---- the peak request (NBLS_MUSIC_PEAKS): read by the PK instance alone ----
    double* slab;             // [launch's workgroups][G] where the plan keeps no map
    PeakOut pk;               // K and the neighbour table of nbls_set_capon_peaks, the request's own floor, the four results
};

// the pair r of step k of the tournament over NP = 2 * ceil(N / 2) players; q = -1: p has the bye (odd N, the player N)
__device__ inline void music_pair(int k, int r, int NP, int N, int& p, int& q) {
    const int m = NP - 1;
    int x, y;
    if (r == 0) { x = m; y = k; }
    else { x = k + r; if (x >= m) x -= m; y = k - r; if (y < 0) y += m; }
    p = x < y ? x : y;
    q = x < y ? y : x;
    if (q >= N) q = -1;
}

// PK: the K strongest peaks of the map as well
template <bool PK>
__global__ __launch_bounds__(CT) void capon_music_kernel(MUArgs a) {
    // dynamic LDS, sized by N (nbls_capon_music_lds_bytes_of): A [N][N] complex, E [N][N] complex, Y [N][2][THREADS],
    // rot [ceil(N / 2)][4], lam [N], ord [N] (int)
    extern __shared__ __attribute__((aligned(16))) double music_lds[];
    __shared__ double red_p[CW];
    __shared__ int red_g[CW];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= a.nunits) return;                         // (the same for every thread of the workgroup)
    const int u = a.u0 + blockIdx.x;
    const int row = a.unit_band[u], w = a.unit_win[u];
    const int band = row / a.nseg;
    const int N = a.N, G = a.G;
    const int64_t cell = (int64_t)row * a.vector_len + w;
    double* const A = music_lds;
    double* const E = A + N * N * 2;
    double* const Y = E + N * N * 2;
    double* const rot = Y + 2 * CT * N;
    double* const lam = rot + 2 * N + 4;
    int* const ord = (int*)(lam + N);
    const double2* Rin = (const double2*)a.csdm + cell * N * N;
    int nan_here = 0;
    for (int e = tid; e < N * N; e += CT) {
        const double2 r = Rin[e];
        nan_here |= (r.x != r.x) || (r.y != r.y);
        const int i = e / N, j = e - i * N;
        A[e * 2] = r.x; A[e * 2 + 1] = r.y;
        E[e * 2] = i == j ? 1.0 : 0.0; E[e * 2 + 1] = 0.0;
    }
    const int bad_r = __syncthreads_or(nan_here);                    // (and the barrier behind the writes of A and E)
    double t = 0.0;
    for (int i = 0; i < N; ++i) t += A[(i * N + i) * 2];             // (every thread, the same order)
    const double nan_ = __builtin_nan("");
    if (bad_r || t == 0.0 || t != t) {
        if (tid == 0) { a.nsrc[cell] = -1; a.sweeps[cell] = 0; a.index[cell] = -1; a.power[cell] = nan_; }
        if (tid < N) a.eigenvalues[cell * N + tid] = nan_;
        if (a.map)
            for (int g = tid; g < G; g += CT) a.map[cell * G + g] = nan_;
        if (a.vectors)
            for (int e = tid; e < 2 * N * N; e += CT) a.vectors[cell * 2 * N * N + e] = nan_;
        if constexpr (PK) capon_peaks_none(a.pk, cell, tid);
        return;
    }
    const int M2 = (N + 1) / 2, NP = 2 * M2, steps = NP - 1;
    // this thread's blocks on and above the block diagonal: b = c (c + 1) / 2 + r, r <= c
    const int nblk = M2 * (M2 + 1) / 2;
    int br[MBLK], bc[MBLK];
#pragma unroll
    for (int m = 0; m < MBLK; ++m) {
        const int b = tid + m * CT;
        int c = 0;
        while ((c + 1) * (c + 2) / 2 <= b) ++c;
        bc[m] = c; br[m] = b - c * (c + 1) / 2;
    }
    double nrm2 = 0.0;                                               // ||R||_F^2, every entry in storage order
    for (int e = 0; e < N * N; ++e) {
        nrm2 = __builtin_fma(A[2 * e], A[2 * e], nrm2);
        nrm2 = __builtin_fma(A[2 * e + 1], A[2 * e + 1], nrm2);
    }
    const double tol2 = NBLS_MUSIC_STOP_SQUARED * nrm2;
    int sweeps = 0;
    while (sweeps < SWEEP_CAP) {
        double off2 = 0.0;                                           // the strict lower triangle, rows ascending
        for (int i = 1; i < N; ++i)
            for (int j = 0; j < i; ++j) {
                off2 = __builtin_fma(A[(i * N + j) * 2], A[(i * N + j) * 2], off2);
                off2 = __builtin_fma(A[(i * N + j) * 2 + 1], A[(i * N + j) * 2 + 1], off2);
            }
        if (2.0 * off2 <= tol2) break;                               // (the same values in every thread: one decision)
        for (int k = 0; k < steps; ++k) {
            if (tid < M2) {                                          // the pair's rotation
                int p, q;
                music_pair(k, tid, NP, N, p, q);
                double c = 1.0, sr = 0.0, si = 0.0, tg = 0.0;
                if (q >= 0) {
                    const double xr = A[(p * N + q) * 2], xi = A[(p * N + q) * 2 + 1];
                    const double g2 = __builtin_fma(xi, xi, xr * xr);
                    if (g2 > 0.0) {
                        const double g = sqrt(g2);
                        const double tau = (A[(q * N + q) * 2] - A[(p * N + p) * 2]) / (2.0 * g);
                        const double tt = __builtin_copysign(1.0, tau) / (fabs(tau) + sqrt(__builtin_fma(tau, tau, 1.0)));
                        c = 1.0 / sqrt(__builtin_fma(tt, tt, 1.0));
                        const double s = tt * c;
                        sr = s * (xr / g); si = s * (xi / g);
                        tg = tt * g;
                    }
                }
                rot[4 * tid] = c; rot[4 * tid + 1] = sr; rot[4 * tid + 2] = si; rot[4 * tid + 3] = tg;
            }
            __syncthreads();
#pragma unroll
            for (int m = 0; m < MBLK; ++m) {                         // X' = J1^H X J2 of block (r, c)
                if (tid + m * CT >= nblk) continue;
                const int r = br[m], cc = bc[m];
                int p, q, p2, q2;
                music_pair(k, r, NP, N, p, q);
                if (r == cc) {                                       // the pair's own block: the definition's closed form
                    if (q < 0) continue;
                    const double tg = rot[4 * r + 3];
                    A[(p * N + p) * 2] = A[(p * N + p) * 2] - tg; A[(p * N + p) * 2 + 1] = 0.0;
                    A[(q * N + q) * 2] = A[(q * N + q) * 2] + tg; A[(q * N + q) * 2 + 1] = 0.0;
                    A[(p * N + q) * 2] = 0.0; A[(p * N + q) * 2 + 1] = 0.0;
                    A[(q * N + p) * 2] = 0.0; A[(q * N + p) * 2 + 1] = 0.0;
                    continue;
                }
                music_pair(k, cc, NP, N, p2, q2);
                const double c1 = rot[4 * r], s1r = rot[4 * r + 1], s1i = rot[4 * r + 2];
                const double c2 = rot[4 * cc], s2r = rot[4 * cc + 1], s2i = rot[4 * cc + 2];
                // X = [[x00, x01], [x10, x11]] = A[{p, q}][{p2, q2}]; an absent row or column reads as 0 and is not stored
                double x00r = A[(p * N + p2) * 2], x00i = A[(p * N + p2) * 2 + 1];
                double x01r = 0.0, x01i = 0.0, x10r = 0.0, x10i = 0.0, x11r = 0.0, x11i = 0.0;
                if (q2 >= 0) { x01r = A[(p * N + q2) * 2]; x01i = A[(p * N + q2) * 2 + 1]; }
                if (q >= 0) { x10r = A[(q * N + p2) * 2]; x10i = A[(q * N + p2) * 2 + 1]; }
                if (q >= 0 && q2 >= 0) { x11r = A[(q * N + q2) * 2]; x11i = A[(q * N + q2) * 2 + 1]; }
                // T = X J2: T_:0 = c2 X_:0 - conj(s2) X_:1, T_:1 = s2 X_:0 + c2 X_:1
                const double t00r = __builtin_fma(-s2i, x01i, __builtin_fma(-s2r, x01r, c2 * x00r));
                const double t00i = __builtin_fma(s2i, x01r, __builtin_fma(-s2r, x01i, c2 * x00i));
                const double t01r = __builtin_fma(-s2i, x00i, __builtin_fma(s2r, x00r, c2 * x01r));
                const double t01i = __builtin_fma(s2i, x00r, __builtin_fma(s2r, x00i, c2 * x01i));
                const double t10r = __builtin_fma(-s2i, x11i, __builtin_fma(-s2r, x11r, c2 * x10r));
                const double t10i = __builtin_fma(s2i, x11r, __builtin_fma(-s2r, x11i, c2 * x10i));
                const double t11r = __builtin_fma(-s2i, x10i, __builtin_fma(s2r, x10r, c2 * x11r));
                const double t11i = __builtin_fma(s2i, x10r, __builtin_fma(s2r, x10i, c2 * x11i));
                // X' = J1^H T: X'_0: = c1 T_0: - s1 T_1:, X'_1: = conj(s1) T_0: + c1 T_1:
                x00r = __builtin_fma(s1i, t10i, __builtin_fma(-s1r, t10r, c1 * t00r));
                x00i = __builtin_fma(-s1i, t10r, __builtin_fma(-s1r, t10i, c1 * t00i));
                x01r = __builtin_fma(s1i, t11i, __builtin_fma(-s1r, t11r, c1 * t01r));
                x01i = __builtin_fma(-s1i, t11r, __builtin_fma(-s1r, t11i, c1 * t01i));
                x10r = __builtin_fma(s1i, t00i, __builtin_fma(s1r, t00r, c1 * t10r));
                x10i = __builtin_fma(-s1i, t00r, __builtin_fma(s1r, t00i, c1 * t10i));
                x11r = __builtin_fma(s1i, t01i, __builtin_fma(s1r, t01r, c1 * t11r));
                x11i = __builtin_fma(-s1i, t01r, __builtin_fma(s1r, t01i, c1 * t11i));
                A[(p * N + p2) * 2] = x00r; A[(p * N + p2) * 2 + 1] = x00i;
                A[(p2 * N + p) * 2] = x00r; A[(p2 * N + p) * 2 + 1] = -x00i;
                if (q2 >= 0) {
                    A[(p * N + q2) * 2] = x01r; A[(p * N + q2) * 2 + 1] = x01i;
                    A[(q2 * N + p) * 2] = x01r; A[(q2 * N + p) * 2 + 1] = -x01i;
                }
                if (q >= 0) {
                    A[(q * N + p2) * 2] = x10r; A[(q * N + p2) * 2 + 1] = x10i;
                    A[(p2 * N + q) * 2] = x10r; A[(p2 * N + q) * 2 + 1] = -x10i;
                }
                if (q >= 0 && q2 >= 0) {
                    A[(q * N + q2) * 2] = x11r; A[(q * N + q2) * 2 + 1] = x11i;
                    A[(q2 * N + q) * 2] = x11r; A[(q2 * N + q) * 2 + 1] = -x11i;
                }
            }
            for (int item = tid; item < N * M2; item += CT) {        // E J: row i, the columns of pair r
                const int i = item / M2, r = item - i * M2;
                int p, q;
                music_pair(k, r, NP, N, p, q);
                if (q < 0) continue;
                const double c = rot[4 * r], sr = rot[4 * r + 1], si = rot[4 * r + 2];
                const double ur = E[(i * N + p) * 2], ui = E[(i * N + p) * 2 + 1];
                const double vr = E[(i * N + q) * 2], vi = E[(i * N + q) * 2 + 1];
                // E_ip' = c E_ip - conj(s) E_iq, E_iq' = s E_ip + c E_iq
                E[(i * N + p) * 2] = __builtin_fma(-si, vi, __builtin_fma(-sr, vr, c * ur));
                E[(i * N + p) * 2 + 1] = __builtin_fma(si, vr, __builtin_fma(-sr, vi, c * ui));
                E[(i * N + q) * 2] = __builtin_fma(-si, ui, __builtin_fma(sr, ur, c * vr));
                E[(i * N + q) * 2 + 1] = __builtin_fma(si, ur, __builtin_fma(sr, ui, c * vi));
            }
            __syncthreads();
        }
        ++sweeps;
    }
    // the order: value descending, then the column's index ascending
    if (tid < N) {
        const double li = A[(tid * N + tid) * 2];
        int rank = 0;
        for (int j = 0; j < N; ++j) {
            const double lj = A[(j * N + j) * 2];
            rank += (lj > li || (lj == li && j < tid)) ? 1 : 0;
        }
        lam[rank] = li; ord[rank] = tid;
        a.eigenvalues[cell * N + rank] = li;
    }
    __syncthreads();
    int M = a.sources;                                               // (every thread: the same values)
    if (M == 0) {
        const double thr = a.eig_floor * lam[0];
        for (int k = 0; k < N; ++k) M += lam[k] >= thr ? 1 : 0;
        M = M < 1 ? 1 : (M > N - 1 ? N - 1 : M);
    }
    if (tid == 0) { a.nsrc[cell] = M; a.sweeps[cell] = sweeps; }
    if (a.vectors)
        for (int e = tid; e < N * N; e += CT) {                      // out[i][k] = E[i][ord[k]]
            const int i = e / N, k = e - i * N;
            const int src = i * N + ord[k];
            a.vectors[(cell * N * N + e) * 2] = E[src * 2];
            a.vectors[(cell * N * N + e) * 2 + 1] = E[src * 2 + 1];
        }
    // the grid: one lane per point, its steering vector in LDS column tid of Y
    const double2* steer = (const double2*)a.steer + (int64_t)band * N * G;
    const double2* E2 = (const double2*)E;
    double* const yr = Y + tid;                                      // a_i = (yr[i * 2 CT], yr[i * 2 CT + CT])
    const double dn = (double)N;
    double bp = 0.0;
    int bg = -1;
    double* mp = nullptr;                                            // with peaks: where the unit's map stays until it is picked
    if constexpr (PK) mp = a.map ? a.map + cell * G : a.slab + (int64_t)blockIdx.x * G;
    for (int g = tid; g < G; g += CT) {
        for (int i = 0; i < N; ++i) {
            const double2 v = steer[(int64_t)i * G + g];
            yr[i * 2 * CT] = v.x; yr[i * 2 * CT + CT] = v.y;
        }
        double d = 0.0;
        for (int k = M; k < N; ++k) {
            const int col = ord[k];                                  // (a wave-uniform LDS read)
            double zr = 0.0, zi = 0.0;                               // z = e_k^H a
            for (int i = 0; i < N; ++i) {
                const double2 e = E2[i * N + col];
                const double ar = yr[i * 2 * CT], ai = yr[i * 2 * CT + CT];
                zr = __builtin_fma(e.x, ar, zr);
                zr = __builtin_fma(e.y, ai, zr);
                zi = __builtin_fma(e.x, ai, zi);
                zi = __builtin_fma(-e.y, ar, zi);
            }
            d = __builtin_fma(zr, zr, d);
            d = __builtin_fma(zi, zi, d);
        }
        const double p = 1.0 / (d / dn);
        if (a.map) a.map[cell * G + g] = p;
        if (PK && !a.map) mp[g] = p;
        if (capon_better(p, g, bp, bg)) { bp = p; bg = g; }
    }
    capon_best(bp, bg, red_p, red_g, tid);
    if (tid == 0) { a.index[cell] = bg; a.power[cell] = bg < 0 ? nan_ : bp; }
    if constexpr (PK) {
        // the map is this workgroup's own writes to HBM: a fence and a barrier make them its reads
        __threadfence_block();
        __syncthreads();
        capon_peaks_of(a.pk, mp, cell, bg < 0 ? nan_ : bp, bg, red_p, red_g, tid);
    }
}

}  // namespace

// dynamic LDS bytes of capon_music_kernel for an array of nelem elements (see the kernel's head)
size_t nbls_capon_music_lds_bytes_of(int nelem) {
    const size_t n = (size_t)nelem;
    return (4 * n * n + 2 * (size_t)CT * n + 4 * n + 4) * sizeof(double);
}

hipError_t nbls_launch_capon_music(nbls_handle* h, int64_t u0, int64_t nu, hipStream_t st) {
    if (nu <= 0) return hipSuccess;
    if (h->nelem > CMAXN || h->nelem < 3 || h->derived.capon_n < 1 || !h->d_capon_csdm || h->req.music.sources < 0 || h->req.music.sources > h->nelem - 1)
        return hipErrorInvalidValue;                                 // (nbls_plan has refused such a plan)
    MUArgs a{};
    a.unit_band = h->d_unit_band; a.unit_win = h->d_unit_win;
    a.vector_len = h->vector_len; a.u0 = (int)u0; a.nunits = (int)nu;
    a.N = h->nelem; a.nseg = h->nbands / h->fbands; a.G = h->derived.capon_n;
    a.steer = h->d_capon_steer; a.csdm = h->d_capon_csdm.p;
    a.sources = h->req.music.sources; a.eig_floor = h->req.music.eig_floor;
    a.eigenvalues = h->d_music_eig; a.nsrc = h->d_music_int.p;
    const size_t cells = (size_t)h->nbands * h->vector_len;
    a.sweeps = h->d_music_int.p + cells; a.index = h->d_music_int.p + 2 * cells;
    a.power = h->d_music_power;
    a.map = (h->req.music.flags & NBLS_MUSIC_MAP) ? h->d_music_map.p : nullptr;
    a.vectors = (h->req.music.flags & NBLS_MUSIC_VECTORS) ? h->d_music_vec.p : nullptr;
    const bool peaks = (h->req.music.flags & NBLS_MUSIC_PEAKS) != 0;
    const void* fn = peaks ? (const void*)capon_music_kernel<true> : (const void*)capon_music_kernel<false>;
    if (!h->music_attr_set[peaks]) {                                 // once per handle (a streamed pass launches per unit batch)
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)nbls_capon_music_lds_bytes_of(CMAXN));
        if (e != hipSuccess) return e;
        h->music_attr_set[peaks] = true;
    }
    const size_t lds = nbls_capon_music_lds_bytes_of(h->nelem);
    void* params[] = {(void*)&a};
    if (!peaks) return hipLaunchKernel(fn, dim3((unsigned)nu), dim3(CT), params, lds, st);
    if (h->req.peaks.k < 1 || !h->d_capon_nbr || !h->d_music_peak_count) return hipErrorInvalidValue;      // (nbls_plan has refused such a plan)
    a.pk = PeakOut{h->d_capon_nbr, h->derived.capon_n, h->req.peaks.k, h->req.music.peak_floor, h->d_music_peak_count, h->d_music_peak_index,
                   h->d_music_peak_power, h->d_music_peak_offset};
    // the map of a unit lies in its own row of d_music_map where the plan keeps it; else in the slab of its workgroup: at
    // most capon_peak_slabs workgroups per launch.  On one stream its order hands the slabs on; the solves of a pass may be
    // on two, so a launch on the other stream than the last one waits for that one's event first (as nbls_launch_capon)
    a.slab = a.map ? nullptr : h->d_music_slab.p;
    if (a.slab) {
        if (!h->ev_music_slab) {
            const hipError_t e = hipEventCreateWithFlags(&h->ev_music_slab, hipEventDisableTiming);
            if (e != hipSuccess) { h->ev_music_slab = nullptr; return e; }
        }
        if (h->music_slab_stream && h->music_slab_stream != st) {
            const hipError_t e = hipStreamWaitEvent(st, h->ev_music_slab, 0);
            if (e != hipSuccess) return e;
        }
    }
    const int64_t step = a.map ? nu : h->derived.peak_slabs;
    if (step < 1) return hipErrorInvalidValue;
    for (int64_t o = 0; o < nu; o += step) {
        a.u0 = (int)(u0 + o);
        a.nunits = (int)(nu - o < step ? nu - o : step);
        const hipError_t e = hipLaunchKernel(fn, dim3((unsigned)a.nunits), dim3(CT), params, lds, st);
        if (e != hipSuccess) return e;
    }
    if (a.slab) {
        const hipError_t e = hipEventRecord(h->ev_music_slab, st);
        if (e != hipSuccess) return e;
        h->music_slab_stream = st;
    }
    return hipSuccess;
}
