// The elements FAST-LTS dropped, per window (nbls_set_kept_elements; the definition is in include/nbls.h).
//
// Per unit (result row r, window w) of estimator 0, N elements with the full lexicographic pair list, k(a, b) the index of
// pair (a, b), a < b, and the unpacked weights w_k (one byte per pair, as the solve kernels leave them, before pack_weights):
//   c_m          = #{ pairs k that hold m : w_k == 0 }         integer
//   dropped_mask = bits m with c_m >= q                        uint32 [rows][VL]
//   kept_count   = M: N - popcount(mask), or N where fewer than 3 elements would remain (nbls_kept_bits_of)
//
// Mapping: a group of S lanes per unit, S the power of two >= N (8, 16 or 32), so a wave takes 64 / S consecutive units.
// Lane m of a group reads the N - 1 weights of its own element's pairs and counts the zeros: no reduction, no atomics, the
// count does not depend on the launch's unit range.  The mask is the group's field of the wave's ballot.  A unit's row is
// P <= 496 bytes: the group's byte loads stay inside a few cache lines.
#include "nbls_internal.h"

namespace {

constexpr int KEPT_WAVES = 4;
constexpr int KEPT_MAX_ELEMENTS = 32;        // one bit per element of a uint32; 33 elements are beyond the plan's pair limit
static_assert((KEPT_MAX_ELEMENTS + 1) * KEPT_MAX_ELEMENTS / 2 > NBLS_MAX_PAIRS,
              "kept_elements_kernel keeps one element per bit of a uint32 and per lane of half a wave: revisit both before lifting the pair limit");

struct KArgs {
    const uint8_t* wts;       // [B][VL][P]
    int N, P, q;
    const int32_t* unit_band; // [U]
    const int32_t* unit_win;  // [U]
    int vector_len, u0, nunits;
    uint32_t* mask;           // [B][VL]
    int32_t* count;           // [B][VL]
};

template <int S>
__global__ __launch_bounds__(KEPT_WAVES * 64) void kept_elements_kernel(KArgs a) {
    constexpr int UPW = 64 / S;                                  // units per wave
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int grp = lane / S, m = lane - grp * S;
    const int N = a.N;
    const int64_t ul = ((int64_t)blockIdx.x * KEPT_WAVES + wave) * UPW + grp;
    const bool live = ul < a.nunits;
    int64_t cell = 0;
    int c = 0;
    if (live) {
        const int u = a.u0 + (int)ul;
        cell = (int64_t)a.unit_band[u] * a.vector_len + a.unit_win[u];
        if (m < N) {
            const uint8_t* w = a.wts + cell * a.P;
            for (int o = 0; o < m; ++o) c += w[o * (2 * N - o - 1) / 2 + (m - o - 1)] == 0;      // pairs (o, m), o < m
            const int base = m * (2 * N - m - 1) / 2;                                           // pairs (m, o), o > m: consecutive
            for (int o = m + 1; o < N; ++o) c += w[base + (o - m - 1)] == 0;
        }
    }
    const unsigned long long bal = __ballot(live && m < N && c >= a.q);
    if (live && m == 0) {
        const uint32_t dropped = (uint32_t)(bal >> (grp * S)) & (S >= 32 ? 0xffffffffu : ((1u << S) - 1u));
        int M;
        nbls_kept_bits_of(dropped, N, M);
        a.mask[cell] = dropped;
        a.count[cell] = M;
    }
}

}  // namespace

hipError_t nbls_launch_kept_elements(nbls_handle* h, int64_t u0, int64_t nu, hipStream_t st) {
    if (nu <= 0) return hipSuccess;
    const nbls_estimator& s = h->est[0];
    KArgs a{};
    a.wts = s.d_wts;
    a.N = h->nelem; a.P = s.npairs; a.q = h->req.kept_q;
    if (a.N < 1 || a.N > KEPT_MAX_ELEMENTS || (int64_t)a.N * (a.N - 1) / 2 != a.P) return hipErrorInvalidValue;   // (nbls_plan has refused such a plan)
    a.unit_band = h->d_unit_band; a.unit_win = h->d_unit_win;
    a.vector_len = h->vector_len; a.u0 = (int)u0; a.nunits = (int)nu;
    a.mask = h->d_kept_mask; a.count = h->d_kept_count;
    const int S = a.N <= 8 ? 8 : (a.N <= 16 ? 16 : 32);
    const int64_t per_wg = (int64_t)KEPT_WAVES * (64 / S);
    const dim3 grid((unsigned)((nu + per_wg - 1) / per_wg)), block(KEPT_WAVES * 64);
    if (S == 8) hipLaunchKernelGGL(kept_elements_kernel<8>, grid, block, 0, st, a);
    else if (S == 16) hipLaunchKernelGGL(kept_elements_kernel<16>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(kept_elements_kernel<32>, grid, block, 0, st, a);
    return hipGetLastError();
}
