// The correlator route: every window-length decision of the correlation stage in one host function.
//
// A window group (consecutive bands of one window length W) goes through the int8 screening path (quantiser, screening
// kernel, FP64 verifier) where its channel images fit a CU's LDS, else through a general correlator (f64 MFMA where its
// N-channel window fits, else the VALU kernel with its two windows in LDS or read from global memory).  Inside each
// path W sets the tiling, the LDS layout and the kernel instance.  nbls_plan, launch_general_range (xcorr.hip) and
// nbls_launch_xcorr_screen_range (xcorr_screen.hip) all take their decisions from nbls_route_compute; it reads no
// handle and opens no device, so the tests scan it on the host (nbls_route_table).
#include "nbls_internal.h"

namespace {

constexpr size_t kLdsCU = 160 * 1024;       // LDS of a CU: what one workgroup may hold, static and dynamic together
constexpr size_t kLdsHalf = 80 * 1024;      // two workgroups per CU
constexpr size_t kLdsVerify = 158 * 1024;   // verify_lds_kernel's windows (+ zero slot), with room to spare

int round_up(int x, int m) { return (x + m - 1) / m * m; }

// Screening geometry for windows of W samples (the former nbls_screen_geometry).  G = partners per workgroup: all N-1
// (at most 16) when their images fit; else the largest group size whose images fit next to the sliding channel's eight
// shifted copies in a CU's 160 KB — the workgroups of a sliding channel then split its partners (the mechanism that
// serves 18..32 elements), e.g. 8 elements x 6000 samples: two groups of four; 16 elements x 4500 samples: two groups of
// eight.  Where not even two partners fit beside eight copies (~7900 samples) FOUR copies with dword-granular
// addressing (8 bytes per sample, four 4-byte reads per fragment, the C++ K loop): ~13 000 samples — example.py's
// WINLEN_1 = 60 s at 200 Hz.  Beyond, the caller falls back to the general correlator.
bool screen_geometry(int N, int W, int flags, nbls_route* r, size_t* lds) {
    if (N < 3 || N > 33 || W < 64) return false;
    const int NPc = (N - 1) < 16 ? (N - 1) : 16;     // partners per workgroup when everything fits (more than 16: partner groups)
    const int WP = round_up(W, 16);
    r->WP = WP;
    // (option screen_nc4: the four-copy layout also where eight fit — experiment)
    for (int nc = (flags & NBLS_ROUTE_OPT_NC4) ? 4 : 8; nc >= 4; nc -= 4) {
        r->ncopy = nc;
        for (int g = NPc; g >= 2; --g) {
            if (nc == 4 && g == 16) continue;            // (S == 1 selects the eight-tile instance, built for eight copies)
            const int S = 16 / g;
            if (S > 8) break;                            // (the column decode handles up to 8 lag blocks per tile)
            r->G = g;
            r->S = S;
            r->PFB = 16 * (S - 1);
            // partner image: PFB + window + read-ahead padding, a whole number of 256-B bank rows, plus one
            // row of room for the per-partner skew
            r->CSB = round_up(r->PFB + WP + 192, 256) + 256;
            // K round-up + read-ahead of the last tile of a group (sized for the eight-tile groups of the one-block instance
            // where it may be chosen: S == 1)
            int csa = WP + 144 + ((S == 1 ? 8 : NBLS_SCREEN_TB) - 1) * 16 * S;
            csa = round_up(csa, 32);
            while (csa % 64 != 32) csa += 32;            // copy stride == 32 B (mod 64): the 8 copies start 8 banks apart (mod 64), conflict-free ds_read_b64
            r->CSA = csa;
            // two sliding channels per workgroup (8 waves, all N images) when two such workgroups fit a CU's
            // LDS, else one sliding channel (4 waves, N-1 images)
            // + running maxima and merge scalars (6 x 32 ints) + the per-channel records (4 doubles each); the f32 energy
            // tables of the pruning test are added below when they still fit
            // (partner groups: a workgroup with two sliding channels stages the group's g + 1 channels, not all N)
            const size_t lds2 = (size_t)2 * (N - 1 <= 16 ? N : g + 1) * r->CSB + (size_t)4 * nc * csa + 6 * 128 + 16 + 32 * N + 64;
            const size_t lds1 = (size_t)2 * g * r->CSB + (size_t)2 * nc * csa + 6 * 128 + 16 + 32 * N + 64;
            const bool force1 = (flags & NBLS_ROUTE_OPT_NSL1) != 0;          // option: one sliding channel per workgroup
            if (nc == 8 && g == NPc && lds2 + (size_t)(2 + N) * (WP / 32 + 2) * 4 <= kLdsHalf && !force1) { r->nsl = 2; *lds = lds2; }
            else { r->nsl = 1; *lds = lds1; }
            if (*lds <= kLdsCU && *lds >= 1024) return true;
        }
    }
    return false;
}

// The quantiser of the screening path: one instance per group count (a lane holds 8 G samples in registers, and the
// registers set how many waves hide the HBM latency of this streaming kernel); beyond 64 groups per lane the LDS form,
// one slab per wave and as many waves per workgroup (<= 4) as fit a CU's LDS.
bool quantizer(int WP, nbls_route* r) {
    const int gpl = (WP / 8 + 63) / 64;              // 8-sample groups per lane
    if (gpl <= 8) {
        r->quant_inst = gpl <= 2 ? 2 : gpl == 3 ? 3 : gpl <= 4 ? 4 : gpl <= 6 ? 6 : 8;
        r->quant_waves = 4;
        r->lds_dyn[NBLS_ROUTE_QUANTIZE] = (int64_t)4 * (WP / 8 + 8) * sizeof(double);
        return true;
    }
    const size_t slab = (size_t)(WP + WP / 4 + 8) * sizeof(double);
    int nwq = (int)(kLdsCU / slab);
    nwq = nwq > 4 ? 4 : nwq;
    if (nwq < 1) return false;
    r->quant_inst = 1;
    r->quant_waves = nwq;
    r->lds_dyn[NBLS_ROUTE_QUANTIZE] = (int64_t)(slab * nwq);
    return true;
}

// The FP64 verifier of the screening path: the persistent double-buffered one (up to 8 elements, the unit's windows twice
// in LDS, its W / inc tables of `vrows` rows too; 8-byte loads of a row need an even padded trace length), else both
// windows of a unit in LDS, else from global memory.
void verifier(const nbls_route_query& q, nbls_route* r) {
    const size_t vlds = ((size_t)q.N * q.W + 2) * sizeof(double);                    // + the zero slot
    const int vwp = (q.W + 3) & ~1;                                                  // LDS row stride: even, >= W + 2
    const size_t dlds = ((size_t)2 * q.N * vwp + 2) * sizeof(double) + (size_t)2 * q.vrows * sizeof(int);
    if (q.N <= 8 && q.npairs <= 32 && dlds <= kLdsCU && (q.npts_pad & 1) == 0) {
        r->verifier = 1;
        r->verify_threads = 1024;
        r->lds_dyn[NBLS_ROUTE_VERIFY] = (int64_t)dlds;
    } else if (vlds <= kLdsVerify) {
        // (many pairs per unit: sixteen waves share them — the workgroup has the CU to itself when its windows fill the LDS)
        r->verifier = 2;
        r->verify_threads = q.npairs > 128 && vlds > kLdsHalf ? 1024 : 512;
        r->lds_dyn[NBLS_ROUTE_VERIFY] = (int64_t)vlds;
    } else {
        r->verifier = 3;
        r->verify_threads = 256;
        r->lds_static[NBLS_ROUTE_VERIFY] = NBLS_SLDS_VERIFY;
    }
}

}  // namespace

void nbls_route_compute(const nbls_route_query& q, nbls_route* r) {
    *r = nbls_route{};
    const int N = q.N, W = q.W;
    if (!q.no_screen && (q.impl == 0 || q.impl == 3)) {
        nbls_route s{};
        size_t lds = 0;
        if (screen_geometry(N, W, q.flags, &s, &lds) && quantizer(s.WP, &s)) {
            // energy tables in LDS when they do not cost occupancy (two workgroups per CU, or still one)
            const size_t tab = (size_t)(s.nsl + N) * (s.WP / 32 + 2) * 4;
            const size_t cap = lds <= kLdsHalf ? kLdsHalf : kLdsCU;
            s.tab_lds = lds + tab <= cap ? 1 : 0;
            if (s.tab_lds) lds += tab;
            lds += (size_t)q.pad_kb * 1024;                                          // developer: occupancy experiment
            // eight-tile instance: one lag block per tile step and a CU per workgroup (two waves per SIMD: 256 VGPRs)
            // (option screen_tb8: the eight-tile instance wherever S == 1, also for workgroups that would fit a CU twice)
            const bool tb8 = s.S == 1 && (lds > kLdsHalf || (q.flags & NBLS_ROUTE_OPT_TB8)) && !(q.flags & NBLS_ROUTE_OPT_TB4) && s.ncopy == 8;
            s.screen_inst = tb8 ? 3 : (s.ncopy == 4 ? 2 : 1);
            s.lds_dyn[NBLS_ROUTE_SCREEN_STAGE] = (int64_t)lds;
            verifier(q, &s);
            s.correlator = NBLS_ROUTE_SCREEN;
            s.impl = 3;
            *r = s;
            return;
        }
        if (q.impl == 3) return;                                                     // rejected
    }
    // f64-MFMA kernel: one wave per channel (N <= 16) and the N-channel window in LDS
    if (q.impl != 1 && N >= 3 && N <= 16 && q.npairs <= 64 * N) {
        const int S = 16 / (N - 1);
        const int PF = 16 * (S - 1);
        int cs = PF + W + 32;
        cs += ((2 - cs) % 32 + 32) % 32;            // CS == 2 (mod 32)
        const size_t shm = ((size_t)N * cs + N + N * 16) * sizeof(double) + (size_t)N * 16 * sizeof(int);
        if (shm <= kLdsCU) {
            r->correlator = NBLS_ROUTE_MFMA;
            r->impl = 2;
            r->S = S;
            r->PFB = PF;
            r->CSB = cs;
            r->lds_dyn[NBLS_ROUTE_GENERAL] = (int64_t)shm;
            return;
        }
    }
    if (q.impl == 2) return;                                                         // rejected
    // VALU kernel: both windows in LDS where they fit beside its static reduction slots, else read from global memory
    // (L2) — no window length is refused
    const size_t shm = (size_t)2 * W * sizeof(double);
    const bool in_lds = shm + NBLS_SLDS_XCORR_SIMPLE <= kLdsCU;
    r->correlator = in_lds ? NBLS_ROUTE_VALU_LDS : NBLS_ROUTE_VALU_GLOBAL;
    r->impl = 1;
    r->lds_dyn[NBLS_ROUTE_GENERAL] = in_lds ? (int64_t)shm : 0;
    r->lds_static[NBLS_ROUTE_GENERAL] = NBLS_SLDS_XCORR_SIMPLE;
}

nbls_route_query nbls_route_query_of(const nbls_handle* h, int W, int vrows, int impl, bool no_screen) {
    nbls_route_query q{};
    q.N = h->nelem;
    q.W = W;
    q.npairs = h->npairs;
    q.vrows = vrows;
    q.npts_pad = h->npts_pad;
    q.impl = impl;
    q.flags = (h->opt.screen_nc4 ? NBLS_ROUTE_OPT_NC4 : 0) | (h->opt.screen_nsl1 ? NBLS_ROUTE_OPT_NSL1 : 0) |
              (h->opt.screen_tb8 ? NBLS_ROUTE_OPT_TB8 : 0) | (h->opt.screen_tb4 ? NBLS_ROUTE_OPT_TB4 : 0);
    q.pad_kb = h->opt.screen_pad_kb;
    q.no_screen = no_screen;
    return q;
}

extern "C" int nbls_route_table(int32_t nelem, int32_t W0, int32_t W1, int32_t npairs, int32_t vrows, int64_t npts_pad,
                                int32_t xcorr_impl, int32_t flags, nbls_route* out) {
    if (!out || nelem < 2 || W0 < 2 || W1 < W0 || npairs < 1 || vrows < 1 || npts_pad < 1 || xcorr_impl < 0 ||
        xcorr_impl > 3 || (flags & ~15))
        return NBLS_ERR_ARG;
    nbls_route_query q{nelem, W0, npairs, vrows, npts_pad, xcorr_impl, flags, 0, false};
    for (int32_t W = W0; W <= W1; ++W) {
        q.W = W;
        nbls_route_compute(q, out + (W - W0));
    }
    return NBLS_OK;
}

extern "C" int nbls_route_xcorr(int32_t nelem, int32_t W, int32_t npairs, int32_t vrows, int64_t npts_pad,
                                int32_t xcorr_impl, int32_t flags, nbls_route* out) {
    return nbls_route_table(nelem, W, W, npairs, vrows, npts_pad, xcorr_impl, flags, out);
}
