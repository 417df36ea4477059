// What capon_kernel (capon.hip) and capon_clean_kernel (capon_clean.hip) share: the order of the arg-max, the workgroup's
// reduction under it, and the Bartlett value of one grid point.  Both kernels run these functions on the same values, so
// rank 0 of a CLEAN request is bartlett_index / bartlett_power bit for bit.  Device code; no contraction.
#pragma once
#include "nbls_internal.h"

namespace nbls_capon {

constexpr int CT = NBLS_CAPON_THREADS;
constexpr int CW = CT / 64;                  // waves

// "P descending, g ascending"; a NaN is no candidate, g < 0 is "none yet".
__device__ inline bool capon_better(double p, int g, double bp, int bg) {
    if (p != p || g < 0) return false;
    if (bg < 0) return true;
    return p > bp || (p == bp && g < bg);
}

// The workgroup's best of the threads' bests -> thread 0 (any tree: the order is total).
__device__ inline void capon_best(double& p, int& g, double* sp, int* sg, int tid) {
    for (int off = 32; off > 0; off >>= 1) {
        const double op = __shfl_xor(p, off, 64);
        const int og = __shfl_xor(g, off, 64);
        if (capon_better(op, og, p, g)) { p = op; g = og; }
    }
    if ((tid & 63) == 0) { sp[tid >> 6] = p; sg[tid >> 6] = g; }
    __syncthreads();
    if (tid == 0)
        for (int j = 1; j < CW; ++j)
            if (capon_better(sp[j], sg[j], p, g)) { p = sp[j]; g = sg[j]; }
    __syncthreads();
}

// Bartlett value of the lane's grid point: R2 [SN][SN] complex in LDS (read wave-uniformly), the lane's steering vector
// a_i = (yr[i * 2 CT], yr[i * 2 CT + CT]) in its LDS column, nn = SN^2.
//   sum_i R_ii |a_i|^2 + 2 Re(conj(a_i) sum_{j<i} R_ij a_j), over nn
__device__ inline double capon_bartlett_point(const double2* R2, const double* yr, int SN, double nn) {
    double pb = 0.0;
    for (int i = 0; i < SN; ++i) {
        double ur = 0.0, ui = 0.0;
        for (int j = 0; j < i; ++j) {
            const double2 r = R2[i * SN + j];
            const double vr = yr[j * 2 * CT], vi = yr[j * 2 * CT + CT];
            ur = __builtin_fma(r.x, vr, ur);
            ur = __builtin_fma(-r.y, vi, ur);
            ui = __builtin_fma(r.x, vi, ui);
            ui = __builtin_fma(r.y, vr, ui);
        }
        const double ar = yr[i * 2 * CT], ai = yr[i * 2 * CT + CT];
        pb += R2[i * SN + i].x * (ar * ar + ai * ai);
        pb += 2.0 * (ar * ur + ai * ui);
    }
    return pb / nn;
}

}  // namespace nbls_capon
