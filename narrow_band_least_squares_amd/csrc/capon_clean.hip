// A window's arrivals and their powers by CLEAN-SC on the narrow band's cross-spectral matrix (nbls_set_capon_clean;
// DESIGN.md §24; the definition is in include/nbls.h and this kernel follows it literally).
//
// Per unit, from the R that capon_kernel has just written to the plan's csdm buffer on the same stream: up to I times, scan
// the Bartlett spectrum of R_i for its arg-max g_i, form v = R_i a[g_i] and q = Re(a^H v), and take (phi / q) v v^H out of R_i.
// Everything coherent with the beam at g_i leaves with it, sidelobes included, and R_{i+1} stays positive semidefinite.
//
// Mapping: one workgroup of CAPON_THREADS threads per unit, the unit range of nbls_launch_capon.
//   R        read from HBM into LDS once (KEPT: compacted through the unit's dropped mask on the way, row stride M)
//   scan     one lane per grid point, the lane's a in its column of Y [N][2][THREADS] (consecutive lanes on consecutive
//            banks), R read wave-uniformly; capon_bartlett_point is capon_kernel's own code (capon_point.h), so rank 0 is
//            bartlett_index / phi * bartlett_power bit for bit.  No register array is indexed by N
//   arg-max  capon_best; thread 0 publishes (g_i, p_i) in LDS, every thread reads the same two values: a stop is one
//            decision and the workgroup leaves the loop together
//   update   threads k < N put a[g_i] at the head of Y (free behind the scan), threads j < N form v_j, every thread forms
//            q from the same LDS values in the same order, and the triangle update goes by the (i, j) ownership of
//            capon_kernel's R phase; a barrier between the phases
//   LDS      dynamic, (2 N^2 + 2 N + 2 THREADS N) doubles (nbls_capon_clean_lds_bytes_of): R, v, Y; less than capon_kernel's
//            at every N
// No atomics, every order total, nothing depends on the launch's unit range.  Results leave by plain vector stores.
#include "nbls_internal.h"
#include "capon_point.h"

namespace {

using namespace nbls_capon;
constexpr int CMAXN = NBLS_CAPON_MAX_ELEMENTS;
constexpr int CTRI = (CMAXN * (CMAXN + 1) / 2 + CT - 1) / CT;     // lower-triangle entries per thread

struct CLArgs {
    const int32_t* unit_band; // [U]
    const int32_t* unit_win;  // [U]
    int vector_len, u0, nunits;
    int N, nseg, G;
    const double* steer;      // [fbands][N][G][2]
    const double* csdm;       // [B][VL][N][N][2]: R of every unit (capon_kernel)
    const uint32_t* dropped;  // [B][VL] (the KEPT instance alone)
    int iters;                // I
    double gain, floor;
    int32_t* count;           // [B][VL]
    int32_t* index;           // [B][VL][I]
    double* power;            // [B][VL][I]
    double* total;            // [B][VL]
    double* residual;         // [B][VL]
    double* rcsdm;            // [B][VL][N][N][2] or NULL
};

// R_count of the unit -> its [N][N][2] of rcsdm, every entry written once: through pos[] (the element's row of the compacted
// matrix, -1: dropped) where the unit has dropped elements, zeros for those
template <bool KEPT>
__device__ inline void clean_store_matrix(const CLArgs& a, const double* Rm, int SN, uint32_t bits, int64_t cell, int tid) {
    const int N = a.N;
    double2* out = (double2*)a.rcsdm + cell * N * N;
    const double2* R2 = (const double2*)Rm;
    for (int e = tid; e < N * N; e += CT) {
        const int i = e / N, j = e - i * N;
        double2 v = make_double2(0.0, 0.0);
        if (!KEPT || SN == N) {
            v = R2[e];
        } else if ((bits >> i & 1u) && (bits >> j & 1u)) {
            const int pi = __builtin_popcount(bits & ((1u << i) - 1u)), pj = __builtin_popcount(bits & ((1u << j) - 1u));
            v = R2[pi * SN + pj];
        }
        out[e] = v;
    }
}

template <bool KEPT>
__global__ __launch_bounds__(CT) void capon_clean_kernel(CLArgs a) {
    // dynamic LDS, sized by N (nbls_capon_clean_lds_bytes_of): Rm [N][N] complex, V [N] complex, Y [N][2][THREADS]
    extern __shared__ __attribute__((aligned(16))) double clean_lds[];
    __shared__ double red_p[CW];
    __shared__ int red_g[CW];
    __shared__ double pub_p;
    __shared__ int pub_g;
    __shared__ int kidx[KEPT ? CMAXN : 1];                           // e_i, the kept elements in ascending order
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= a.nunits) return;                         // (the same for every thread of the workgroup)
    const int u = a.u0 + blockIdx.x;
    const int row = a.unit_band[u], w = a.unit_win[u];
    const int band = row / a.nseg;
    const int N = a.N, G = a.G, I = a.iters;
    const int64_t cell = (int64_t)row * a.vector_len + w;
    double* const Rm = clean_lds;
    double* const V = Rm + N * N * 2;
    double* const Y = V + N * 2;
    int SN = N;                                                      // elements and row stride of Rm (KEPT: M)
    uint32_t bits = 0;
    if constexpr (KEPT) {
        bits = nbls_kept_bits_of(a.dropped[cell], N, SN);            // (the same in every thread)
        if (tid < SN) {                                              // the tid-th set bit
            uint32_t b = bits;
            for (int i = 0; i < tid; ++i) b &= b - 1;
            kidx[tid] = __builtin_ctz(b);
        }
        __syncthreads();
    }
    const double2* Rin = (const double2*)a.csdm + cell * N * N;
    int nan_here = 0;
    for (int e = tid; e < SN * SN; e += CT) {
        int src = e;
        if constexpr (KEPT) {
            const int i = e / SN, j = e - i * SN;
            src = kidx[i] * N + kidx[j];
        }
        const double2 r = Rin[src];
        nan_here |= (r.x != r.x) || (r.y != r.y);
        Rm[e * 2] = r.x; Rm[e * 2 + 1] = r.y;
    }
    const int bad_r = __syncthreads_or(nan_here);                    // (and the barrier behind the writes of Rm)
    double t = 0.0;
    for (int i = 0; i < SN; ++i) t += Rm[(i * SN + i) * 2];          // (every thread, the same order)
    const double nan_ = __builtin_nan("");
    int32_t* const oidx = a.index + cell * I;
    double* const opow = a.power + cell * I;
    if (bad_r || t == 0.0 || t != t) {
        if (tid == 0) { a.count[cell] = 0; a.total[cell] = nan_; a.residual[cell] = nan_; }
        if (tid < I) { oidx[tid] = -1; opow[tid] = nan_; }
        if (a.rcsdm) clean_store_matrix<KEPT>(a, Rm, SN, bits, cell, tid);
        return;
    }
    // this thread's entries of the lower triangle: e = i (i + 1) / 2 + j, j <= i
    const int ntri = SN * (SN + 1) / 2;
    int ei[CTRI], ej[CTRI];
#pragma unroll
    for (int m = 0; m < CTRI; ++m) {
        const int e = tid + m * CT;
        int i = 0;
        while ((i + 1) * (i + 2) / 2 <= e) ++i;
        ei[m] = i; ej[m] = e - i * (i + 1) / 2;
    }
    const double2* steer = (const double2*)a.steer + (int64_t)band * N * G;
    const double2* R2 = (const double2*)Rm;
    double* const yr = Y + tid;                                      // a_i = (yr[i * 2 CT], yr[i * 2 CT + CT])
    const double nn = (double)SN * (double)SN;
    double p0 = 0.0;
    int count = I;
    for (int it = 0; it < I; ++it) {
        double bb = 0.0;
        int gb = -1;
        for (int g = tid; g < G; g += CT) {
            for (int i = 0; i < SN; ++i) {
                int er = i;                                          // the element's row of the steering table
                if constexpr (KEPT) er = kidx[i];                    // (a wave-uniform LDS read)
                const double2 v = steer[(int64_t)er * G + g];
                yr[i * 2 * CT] = v.x; yr[i * 2 * CT + CT] = v.y;
            }
            const double pb = capon_bartlett_point(R2, yr, SN, nn);
            if (capon_better(pb, g, bb, gb)) { bb = pb; gb = g; }
        }
        capon_best(bb, gb, red_p, red_g, tid);
        if (tid == 0) { pub_p = bb; pub_g = gb; }
        __syncthreads();
        const double pi = pub_p;                                     // (every thread: the same two values)
        const int gi = pub_g;
        if (gi < 0 || !(pi > 0.0)) { count = it; break; }
        if (it == 0) p0 = pi;
        else if (pi < a.floor * p0) { count = it; break; }
        if (tid < SN) {                                              // a[g_i] to the head of Y: A_k = (Y[2 k], Y[2 k + 1])
            int er = tid;
            if constexpr (KEPT) er = kidx[tid];
            const double2 v = steer[(int64_t)er * G + gi];
            Y[2 * tid] = v.x; Y[2 * tid + 1] = v.y;
        }
        __syncthreads();
        if (tid < SN) {                                              // v_j = sum_k R[j][k] a_k
            double vr = 0.0, vi = 0.0;
            for (int k = 0; k < SN; ++k) {
                const double2 r = R2[tid * SN + k];
                const double ar = Y[2 * k], ai = Y[2 * k + 1];
                vr = __builtin_fma(r.x, ar, vr);
                vr = __builtin_fma(-r.y, ai, vr);
                vi = __builtin_fma(r.x, ai, vi);
                vi = __builtin_fma(r.y, ar, vi);
            }
            V[2 * tid] = vr; V[2 * tid + 1] = vi;
        }
        __syncthreads();
        double q = 0.0;
        for (int j = 0; j < SN; ++j) {                               // q = sum_j Re(conj(a_j) v_j)  (every thread)
            q = __builtin_fma(Y[2 * j], V[2 * j], q);
            q = __builtin_fma(Y[2 * j + 1], V[2 * j + 1], q);
        }
        if (!(q > 0.0) || !(q < __builtin_inf())) { count = it; break; }
        const double s = a.gain / q;
#pragma unroll
        for (int m = 0; m < CTRI; ++m) {
            if (tid + m * CT >= ntri) continue;
            const int j = ei[m], k = ej[m];                          // j >= k
            const double vjr = V[2 * j], vji = V[2 * j + 1], vkr = V[2 * k], vki = V[2 * k + 1];
            const double wr = __builtin_fma(vji, vki, vjr * vkr);
            const double wi = __builtin_fma(vji, vkr, -(vjr * vki));
            const double re = __builtin_fma(-wr, s, Rm[(j * SN + k) * 2]);
            const double im = j == k ? 0.0 : __builtin_fma(-wi, s, Rm[(j * SN + k) * 2 + 1]);
            Rm[(j * SN + k) * 2] = re; Rm[(j * SN + k) * 2 + 1] = im;
            Rm[(k * SN + j) * 2] = re; Rm[(k * SN + j) * 2 + 1] = -im;
        }
        if (tid == 0) { oidx[it] = gi; opow[it] = a.gain * pi; }
        __syncthreads();                                             // (R_{i+1} is there; Y and V are free)
    }
    double tr = 0.0;
    for (int i = 0; i < SN; ++i) tr += Rm[(i * SN + i) * 2];
    if (tid == 0) { a.count[cell] = count; a.total[cell] = t / (double)SN; a.residual[cell] = tr / (double)SN; }
    if (tid >= count && tid < I) { oidx[tid] = -1; opow[tid] = nan_; }
    if (a.rcsdm) clean_store_matrix<KEPT>(a, Rm, SN, bits, cell, tid);
}

}  // namespace

// dynamic LDS bytes of capon_clean_kernel for an array of nelem elements (see the kernel's head)
size_t nbls_capon_clean_lds_bytes_of(int nelem) {
    const size_t n = (size_t)nelem;
    return (2 * n * n + 2 * n + 2 * (size_t)CT * n) * sizeof(double);
}

hipError_t nbls_launch_capon_clean(nbls_handle* h, int64_t u0, int64_t nu, hipStream_t st) {
    if (nu <= 0) return hipSuccess;
    if (h->nelem > CMAXN || h->nelem < 1 || h->derived.capon_n < 1 || !h->d_capon_csdm) return hipErrorInvalidValue;   // (nbls_plan has refused such a plan)
    CLArgs a{};
    a.unit_band = h->d_unit_band; a.unit_win = h->d_unit_win;
    a.vector_len = h->vector_len; a.u0 = (int)u0; a.nunits = (int)nu;
    a.N = h->nelem; a.nseg = h->nbands / h->fbands; a.G = h->derived.capon_n;
    a.steer = h->d_capon_steer; a.csdm = h->d_capon_csdm.p;
    a.iters = h->req.clean.iterations; a.gain = h->req.clean.gain; a.floor = h->req.clean.floor;
    a.count = h->d_clean_count; a.index = h->d_clean_index; a.power = h->d_clean_power;
    a.total = h->d_clean_tr.p; a.residual = h->d_clean_tr.p + (size_t)h->nbands * h->vector_len;
    a.rcsdm = (h->req.clean.flags & NBLS_CLEAN_RESIDUAL) ? h->d_clean_csdm.p : nullptr;
    const bool kept = h->req.kept_capon();
    if (kept) {
        if (!h->d_kept_mask) return hipErrorInvalidValue;
        a.dropped = h->d_kept_mask;
    }
    const void* fn = kept ? (const void*)capon_clean_kernel<true> : (const void*)capon_clean_kernel<false>;
    if (!h->clean_attr_set[kept]) {                                  // once per handle (a streamed pass launches per unit batch)
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)nbls_capon_clean_lds_bytes_of(CMAXN));
        if (e != hipSuccess) return e;
        h->clean_attr_set[kept] = true;
    }
    void* params[] = {(void*)&a};
    return hipLaunchKernel(fn, dim3((unsigned)nu), dim3(CT), params, nbls_capon_clean_lds_bytes_of(h->nelem), st);
}
