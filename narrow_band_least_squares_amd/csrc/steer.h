// Fractional-sample steering (nbls_set_beam_interpolation): the delay split and the Lagrange coefficients,
// one function for the beam kernel (device), the grid kernel's table (host) and nothing else.  Include it only from
// translation units built without contraction: the contract is this sequence of IEEE operations.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

// tau (|tau| < 2^30) -> n = floor(tau), mu = tau - n in [0, 1): the subtraction is exact.
__host__ __device__ inline void nbls_steer_split(double tau, int& n, double& mu) {
    const double fl = floor(tau);
    n = (int)fl;
    mu = tau - fl;
}

// c[k + K - 1] = c_k(mu), k = -K+1 .. K, K = TAPS / 2:
//   c_k = (((1.0 * (mu - j_1)) * (mu - j_2)) * ...) / D_k,  j ascending over -K+1 .. K without k,  D_k = prod_{j != k} (k - j)
// D_k is an exact integer (|D| <= 5040 at 8 taps); one division per coefficient.  mu = 0: c_0 = 1.0, the others +-0.
template <int TAPS>
__host__ __device__ inline void nbls_steer_coefficients(double mu, double* c) {
    constexpr int K = TAPS / 2;
#pragma unroll
    for (int k = -K + 1; k <= K; ++k) {
        double p = 1.0;
        int D = 1;
#pragma unroll
        for (int j = -K + 1; j <= K; ++j) {
            if (j == k) continue;
            p = p * (mu - (double)j);
            D *= k - j;
        }
        c[k + K - 1] = p / (double)D;
    }
}
