// FAST-LTS for large arrays (9..32 elements, 36..496 pairs): ONE START PER LANE for the whole C-step, the h-th
// smallest residual by bucket refinement (lts_bucket.h).  Included by solve.hip inside its anonymous namespace.
//
// Why this form (round 3; the wave-cooperative kernel it replaces spent 2.6 M of its 2.8 M cycles per unit at 120
// pairs in ~600-instruction bitwise bisections, each a chain of compare -> ballot -> popcount -> scalar branch):
//   * a C-step of one start is lane-local: residuals (y_k - c0_k z0) - c1_k z1 are recomputed in every pass from
//     values that are the same for all 64 lanes — c0, c1 and their products come through the SCALAR cache into
//     SGPRs (plan constants, read-only), y and its products from LDS broadcast reads — so a pass is ~10 vector
//     instructions per pair for 64 starts at once, with no cross-lane traffic and no dependent scalar chain;
//   * the h-th smallest |r| is found by counting the keys into 64 bins of a bracket that shrinks 6 bits per pass
//     (per-lane histogram columns in LDS: 64 bins x 32 words, the two lanes l and l+32 share a word as two u16
//     halves, so ds_add_u32 is conflict-free and needs no per-key address arithmetic beyond bin << 7); two or three
//     passes from a guess (the start's previous threshold), three or four without;
//   * the sums of the fit (objective + 2x2 normal equations, ascending k, fma(t_k, w_k, sum) with w in {0,1}: the
//     arithmetic-order contract of the other kernels and the oracle) run in one more pass that also emits the
//     subset as a bit mask for the merging of identical subsets;
//   * live starts are kept in a compacted list: a wave takes 64 of them at a time, so that merged / converged
//     starts free whole wave-iterations (500 starts -> about 19 wave-iterations over the five selections instead
//     of 40).
// Same sequence of operations per start as solve_lts_kernel / the oracle; weights and z are bit-identical
// (tests: test_ltsva_large_arrays_bucket_kernel, tie grid, soak_large).

#ifdef NBLS_DEVELOPER     // thread 0's cycle accounts (second half of the stamp buffer: nbls_debug_lts_coop_breakdown)
#define BK_NOW() (acc ? __builtin_amdgcn_s_memtime() : 0ull)
#define BK_ACC(i, t0) do { if (acc) acc[i] += __builtin_amdgcn_s_memtime() - (t0); } while (0)
#define BK_ACC_ADD(i, v) do { if (acc) acc[i] += (unsigned long long)(v); } while (0)
#define BK_WACC_ARG , wacc
#else
#define BK_WACC_ARG
#define BK_NOW() 0ull
#define BK_ACC(i, t0) do { (void)(t0); } while (0)
#define BK_ACC_ADD(i, v) do { } while (0)
#endif

struct BkLds {
    double* y;                      // [P + 16] standardised lags (the pair loops read one block ahead)
    double* ys;                     // [ceil(P / 4) + 16] every 4th of them (sample pass)
    double *z0S, *z1S, *prevS;      // [S] entry state; prevS holds the final objective once an entry has finished
    unsigned short* thw;            // [S] top 16 bits of the entry's last threshold (centre of its next first pass)
    unsigned int* masks;            // [S][MWS] h-subset bit masks (bit order: k = 32 w + j at bit 31 - j)
    unsigned short *ordA, *ordB;    // [S] compacted list of live entries (double buffer)
    unsigned int* tab;              // [1024] one-probe hash of the subsets
    double* wred;                   // [8] doubles + [8] ints: per-wave partial results of the candidate peel
    int* misc;                      // [16]
    int* cand;                      // [NBLS_MAX_CAND]
    double* cres;                   // [4]
    unsigned char* stt;             // [S] 1 live, 2 finished, 0 dead (NaN), 3 not a candidate, 4 merged
    unsigned int* hist;             // [nwaves][65][32]; the prologue and the finish phase use this space as scratch
    int MW, MWS;
    int nsample;                    // selections of a start whose first pass is centred by the coarse sample histogram (the later ones: the start's previous threshold)
};

// Histogram of one wave: 65 rows (64 bins + the dump row) of 64 / LPW words; LPW lanes share a word (LPW = 2: two
// u16 counters, any pair count; LPW = 4: four u8 counters, up to 255 pairs — half the LDS, twice the resident waves).
__host__ __device__ constexpr int bk_hist_words(int lpw) { return 65 * (64 / lpw); }

__host__ __device__ inline size_t bk_align16(size_t b) { return (b + 15) & ~(size_t)15; }

// Byte offsets of the carve-up (host: LDS size; device: pointers).
struct BkLayout {
    size_t y, ys, z, thw, masks, ord, tab, wred, misc, cand, cres, stt, hist, total;
    int MW, MWS;
};
__host__ __device__ inline BkLayout bk_layout(int P, int S, int nwaves, int lpw, bool dedupe) {
    BkLayout o;
    o.MW = (P + 31) / 32;
    o.MWS = o.MW | 1;                                   // odd row stride: lanes writing their own rows do not collide
    size_t b = 0;
    o.y = b;      b = bk_align16(b + (size_t)(P + 16) * sizeof(double));
    o.ys = b;     b = bk_align16(b + (size_t)((P + 3) / 4 + 16) * sizeof(double));
    o.z = b;      b = bk_align16(b + (size_t)3 * S * sizeof(double));
    o.thw = b;    b = bk_align16(b + (size_t)S * sizeof(unsigned short));
    o.masks = b;  b = bk_align16(b + (dedupe ? (size_t)S * o.MWS * sizeof(unsigned int) : 0));
    o.ord = b;    b = bk_align16(b + (size_t)2 * S * sizeof(unsigned short));
    o.tab = b;    b = bk_align16(b + (dedupe ? (size_t)1024 * sizeof(unsigned int) : 0));
    o.wred = b;   b = bk_align16(b + (size_t)8 * (sizeof(double) + sizeof(int)));
    o.misc = b;   b = bk_align16(b + (size_t)16 * sizeof(int));
    o.cand = b;   b = bk_align16(b + (size_t)NBLS_MAX_CAND * sizeof(int));
    o.cres = b;   b = bk_align16(b + (size_t)4 * sizeof(double));
    o.stt = b;    b = bk_align16(b + (size_t)S);
    o.hist = b;
    // scratch of the prologue (2 P doubles) and of the finish phase (4 P doubles + P bytes) lives in the histograms
    size_t hb = (size_t)nwaves * bk_hist_words(lpw) * sizeof(unsigned int);
    const size_t scratch = bk_align16((size_t)4 * P * sizeof(double)) + bk_align16((size_t)P);
    if (hb < scratch) hb = scratch;
    b = bk_align16(b + hb);
    o.total = b;
    return o;
}

__device__ inline BkLds bk_carve(unsigned char* sm, int P, int S, int nwaves, int lpw, bool dedupe) {
    const BkLayout o = bk_layout(P, S, nwaves, lpw, dedupe);
    BkLds L;
    L.y = (double*)(sm + o.y);
    L.ys = (double*)(sm + o.ys);
    L.z0S = (double*)(sm + o.z);  L.z1S = L.z0S + S;  L.prevS = L.z1S + S;
    L.thw = (unsigned short*)(sm + o.thw);
    L.masks = (unsigned int*)(sm + o.masks);
    L.ordA = (unsigned short*)(sm + o.ord);  L.ordB = L.ordA + S;
    L.tab = (unsigned int*)(sm + o.tab);
    L.wred = (double*)(sm + o.wred);
    L.misc = (int*)(sm + o.misc);
    L.cand = (int*)(sm + o.cand);
    L.cres = (double*)(sm + o.cres);
    L.stt = sm + o.stt;
    L.hist = (unsigned int*)(sm + o.hist);
    L.MW = o.MW;
    L.MWS = o.MWS;
    return L;
}

size_t lts_bucket_lds_bytes(int P, int S, int nwaves, int lpw, bool dedupe) { return bk_layout(P, S, nwaves, lpw, dedupe).total; }

// Scan of the lane's histogram column for absolute rank `target`, two levels: totals of 8 groups of 8 bins (all
// lanes that share a word in one packed add), then the bins of the group that holds the rank; the column is zeroed.
template <int LPW>
__device__ __forceinline__ void bk_scan(unsigned int* col, int hs, int target, int& bsel, int& cbelow, int& cincl) {
    constexpr int RS = 64 / LPW, FBITS = 32 / LPW;
    constexpr unsigned int FMASK = (1u << FBITS) - 1u;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    unsigned int gs[8];
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        unsigned int t = 0u;
#pragma unroll
        for (int j = 0; j < 8; ++j) t += col[(g * 8 + j) * RS];
        gs[g] = t;
    }
    int cum = 0, gsel = 0, cb = 0;
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        const int ci = cum + (int)((gs[g] >> hs) & FMASK);
        const bool below = ci < target;
        gsel += below;
        cb = below ? ci : cb;
        cum = ci;
    }
    gsel = gsel > 7 ? 7 : gsel;
    bsel = gsel * 8;
    cbelow = cb;
    cincl = 0x7fffffff;
    cum = cb;
    const unsigned int* grp = col + gsel * (8 * RS);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int ci = cum + (int)((grp[j * RS] >> hs) & FMASK);
        const bool below = ci < target;
        bsel += below;
        cbelow = below ? ci : cbelow;
        cincl = below ? cincl : (ci < cincl ? ci : cincl);
        cum = ci;
    }
    bsel = bsel > 63 ? 63 : bsel;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
    for (int b = 0; b < 64; ++b) col[b * RS] = 0u;
}

// Tables of the sample pass: every 4th pair (plan: d_xss; LDS: L.ys), ns = ceil(P / 4) pairs.
struct BkSample { const double* xss; const double* ys; int ns; int hs; };
constexpr int BK_SAMPLE_E0 = 1023 - 48;          // coarse bins: one binade each from 2^-48 up (below: bin 0, above 2^15: bin 63)

// One wave, one start per lane: (T, m) of the h-subset of the fit (z0, z1).  hist: this wave's histogram (zero on
// entry and on exit; a gather pass keeps its key lists there).  xs: standardised co-array [P][2] (global, read
// through the scalar cache); y: LDS.  sample != nullptr: the centre of the first pass comes from a coarse histogram
// of every 4th pair (a quarter of a pass) instead of centre_hw.
template <int LPW>
__device__ __forceinline__ void bk_select(const double* __restrict__ xs, const double* y, int P, int h, double z0, double z1,
                                          unsigned int centre_hw, int shift0, const BkSample* sample, bool active, unsigned int* hist,
                                          int lane, unsigned long long& T_out, int& m_out, unsigned long long* acc = nullptr) {
    constexpr int ROW = 64 / LPW, FBITS = 32 / LPW;             // words per histogram row, bits per counter
    constexpr int RS = ROW;                                     // row stride (an odd stride, ROW + 1, is conflict-free in tools/lds_atomic_rate — 5.8 against 7.2 cycles per update — but costs a second address instruction per pair: the kernel got 4 % slower)
    const int lp = lane & (ROW - 1);
    const int hs = (lane / ROW) * FBITS;
    unsigned int* col = hist + lp;
    unsigned int inc = active ? (1u << hs) : 0u;                // a lane without work adds nothing
    if (sample) {
        const unsigned int lo_hw = (unsigned int)BK_SAMPLE_E0 << 20;
        const int sh = 20;
        const double* __restrict__ xss = sample->xss;
        BK_HIST_PASS(sample->ns, xss, sample->ys, nbls_bucket::bin_of_hw(lo_hw, sh, hw));
        int bsel, cbelow, cincl;
        bk_scan<LPW>(col, hs, sample->hs, bsel, cbelow, cincl);
        centre_hw = nbls_bucket::centre_from_sample(BK_SAMPLE_E0, bsel, cbelow, cincl, sample->hs);
        BK_ACC_ADD(4, 1);
    }
    nbls_bucket::Lane s;
    nbls_bucket::init(s, centre_hw, shift0, h, active);
    for (;;) {
        inc = s.done ? 0u : (1u << hs);
        if (__ballot(!s.done && !nbls_bucket::fast_ok(s)) == 0ull) {
            const unsigned int lo_hw = (unsigned int)(s.lo >> 32);
            const int sh = s.shift >= 32 ? s.shift - 32 : 0;
            BK_HIST_PASS(P, xs, y, nbls_bucket::bin_of_hw(lo_hw, sh, hw));
        } else {
            // ---- some lane needs the low word (keys that agree in their first 26 bits): full 64-bit keys ----
            for (int k = 0; k < P; ++k) {
                const double r = (y[k] - xs[2 * k] * z0) - xs[2 * k + 1] * z1;
                const int b = nbls_bucket::bin_of(s, bk_key(r));
                __hip_atomic_fetch_add(col + b * RS, inc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        int bsel, cbelow, cincl;
        bk_scan<LPW>(col, hs, h, bsel, cbelow, cincl);
        nbls_bucket::update(s, bsel, cbelow, cincl);
        BK_ACC_ADD(4, 1);
        if (__ballot(!s.done) == 0ull) break;
        if (__ballot(!s.done && !s.gather_ok) == 0ull) {
            // ---- every unfinished lane's bin holds at most kCap keys: collect them and pick the threshold ----
            unsigned long long* lst = (unsigned long long*)hist + lane;      // slot j of this lane: lst[64 j]
            const unsigned long long glo = s.glo, gw = s.done ? 0ull : s.ghi - s.glo;
            int cnt = 0;
            BK_FOR_PAIRS8(P, xs, y, {
                const double r = (yk - c0 * z0) - c1 * z1;
                const unsigned long long key = bk_key(r);
                if (key - glo < gw && cnt < nbls_bucket::kCap) { lst[64 * cnt] = key; ++cnt; }
            });
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            uint64_t g[nbls_bucket::kCap];
#pragma unroll
            for (int j = 0; j < nbls_bucket::kCap; ++j) { g[j] = lst[64 * j]; }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
            for (int j = 0; j < nbls_bucket::kCap; ++j) lst[64 * j] = 0ull;
            nbls_bucket::finish_gather(s, g, cnt);
            BK_ACC_ADD(4, 1);
            break;
        }
    }
    T_out = s.T;
    m_out = s.m;
}

// One wave: a C-step's selection + sums for the 64 entries ord[g*64 ..] (entry state in LDS), then the entry's
// state transition.  it = index of the selection (0: the start's own fit), maxsteps = C-steps allowed.
template <int LPW, bool MASKS>
__device__ __forceinline__ void bk_group(const BkLds& L, const double* __restrict__ xs, const double* __restrict__ xc, int P, int h,
                                         int it, int maxsteps, int shift0, const BkSample* sample, const unsigned short* ord, int nlive, int g,
                                         unsigned int* hist, int lane, unsigned long long* acc = nullptr) {
    const int idx = g * 64 + lane;
    const bool valid = idx < nlive;
    const int s = ord[valid ? idx : nlive - 1];
    const double z0 = L.z0S[s], z1 = L.z1S[s];
    unsigned long long T;
    int m;
    unsigned long long t0 = BK_NOW();
    // the centre of the first fine pass: from the coarse sample histogram (a quarter of a pass) for the first `L.nsample`
    // selections of a start — the thresholds of random elemental starts span ten binades — and from the start's own
    // previous threshold afterwards (a C-step moves it by far less than the two binades either side that the bins cover)
    bk_select<LPW>(xs, L.y, P, h, z0, z1, (unsigned int)L.thw[s] << 16, shift0, it < L.nsample ? sample : nullptr, valid, hist, lane, T, m, acc);
    BK_ACC(5, t0);
    t0 = BK_NOW();
    // ---- sums over the subset, ascending k ----
    double obj = 0.0, sxx = 0.0, sxy = 0.0, syy = 0.0, bx = 0.0, by = 0.0;
    unsigned int mw = 0u;
    unsigned int* mrow = L.masks + (size_t)s * L.MWS;
    if (__ballot(valid && m > 0) == 0ull) {
        BK_FOR_PAIRS_SUMS(P, xs, xc, L, {
            const double r = (yk - c0 * z0) - c1 * z1;
            const bool in = bk_key(r) < T;
            const double w = in ? 1.0 : 0.0;
            obj = __builtin_fma(r * r, w, obj);
            sxx = __builtin_fma(c0 * c0, w, sxx);
            sxy = __builtin_fma(c01, w, sxy);
            syy = __builtin_fma(c1 * c1, w, syy);
            bx = __builtin_fma(c0 * yk, w, bx);
            by = __builtin_fma(c1 * yk, w, by);
            if (MASKS) mw = (mw << 1) | (unsigned int)in;
            if (MASKS && (k & 31) == 31) { if (valid) mrow[k >> 5] = mw; mw = 0u; }
        });
    } else {
        int taken = 0;
        BK_FOR_PAIRS_SUMS(P, xs, xc, L, {
            const double r = (yk - c0 * z0) - c1 * z1;
            const unsigned long long key = bk_key(r);
            bool in = key < T;
            if (key == T && taken < m) { in = true; ++taken; }
            const double w = in ? 1.0 : 0.0;
            obj = __builtin_fma(r * r, w, obj);
            sxx = __builtin_fma(c0 * c0, w, sxx);
            sxy = __builtin_fma(c01, w, sxy);
            syy = __builtin_fma(c1 * c1, w, syy);
            bx = __builtin_fma(c0 * yk, w, bx);
            by = __builtin_fma(c1 * yk, w, by);
            if (MASKS) mw = (mw << 1) | (unsigned int)in;
            if (MASKS && (k & 31) == 31) { if (valid) mrow[k >> 5] = mw; mw = 0u; }
        });
    }
    BK_ACC(6, t0);
    BK_ACC_ADD(7, 1);
    if (!valid) return;
    if (MASKS && (P & 31)) mrow[P >> 5] = mw << (32 - (P & 31));
    L.thw[s] = (unsigned short)(T >> 48);
    const double det = sxx * syy - sxy * sxy;
    const double n0 = (bx * syy - by * sxy) / det;
    const double n1 = (by * sxx - bx * sxy) / det;
    const int kk = it - 1;                        // index of the C-step whose objective this is
    if (!(obj == obj)) { L.stt[s] = 0; return; }
    if (it >= 1 && ((kk >= 1 && obj == L.prevS[s]) || kk == maxsteps - 1)) {
        L.prevS[s] = obj;                         // finished (converged, or the last allowed C-step): its objective; z stays
        L.stt[s] = 2;
        return;
    }
    if (it >= 1) L.prevS[s] = obj;
    L.z0S[s] = n0;
    L.z1S[s] = n1;
}

// C-steps in lock step for the entries of the list ord[0..nlive): on exit finished entries (stt == 2) hold their
// objective in prevS and their z in z0S/z1S.  Returns nothing; the list buffers are swapped as entries leave.
template <int LPW, bool DEDUPE>
__device__ inline void bk_csteps(const BkLds& L, const double* __restrict__ xs, const double* __restrict__ xc, int P, int h,
                                 int maxsteps, int shift0, const BkSample* sample, int nlive, int tid, int nthr,
                                 unsigned long long* acc = nullptr, unsigned long long* wacc = nullptr) {
    const int lane = tid & 63, wv = tid >> 6, nwv = nthr >> 6;
    unsigned short* ord = L.ordA;
    unsigned short* ord2 = L.ordB;
    unsigned int* hist = L.hist + (size_t)wv * bk_hist_words(LPW);
    for (int it = 0; it <= maxsteps && nlive > 0; ++it) {
        const int ngroups = (nlive + 63) >> 6;
        unsigned long long t0 = BK_NOW();
        BK_ACC_ADD(3, nlive);
#ifdef NBLS_DEVELOPER
        const unsigned long long tw0 = wacc ? __builtin_amdgcn_s_memtime() : 0ull;
#endif
        for (int g = wv; g < ngroups; g += nwv)
            bk_group<LPW, DEDUPE>(L, xs, xc, P, h, it, maxsteps, shift0, sample, ord, nlive, g, hist, lane, acc);
#ifdef NBLS_DEVELOPER
        if (wacc) *wacc += __builtin_amdgcn_s_memtime() - tw0;
#endif
        __syncthreads();
        BK_ACC(0, t0);
        t0 = BK_NOW();
        if (DEDUPE && it < maxsteps) {
            // Entries that landed on the SAME h-subset continue identically from here (a C-step depends on the subset
            // only): the lowest start index of each group is carried on, the others are dropped — whatever this
            // iteration made of them (they would end with the same (objective, z) and be discarded as duplicate
            // candidates anyway).  One-probe hash: a collision merely leaves a mergeable entry alive.
            for (int q = tid; q < 1024; q += nthr) L.tab[q] = 0xffffffffu;
            __syncthreads();
            for (int i = tid; i < nlive; i += nthr) {
                const int s = ord[i];
                const unsigned int* row = L.masks + (size_t)s * L.MWS;
                unsigned long long hv = 0x9E3779B97F4A7C15ull;
                for (int q = 0; q < L.MW; ++q) hv = (hv ^ row[q]) * 0xD6E8FEB86659FD93ull + (hv >> 29);
                atomicMin(&L.tab[(unsigned int)(hv >> 40) & 1023u], (unsigned int)s);
            }
            __syncthreads();
            for (int i = tid; i < nlive; i += nthr) {
                const int s = ord[i];
                const unsigned int* row = L.masks + (size_t)s * L.MWS;
                unsigned long long hv = 0x9E3779B97F4A7C15ull;
                for (int q = 0; q < L.MW; ++q) hv = (hv ^ row[q]) * 0xD6E8FEB86659FD93ull + (hv >> 29);
                const unsigned int w = L.tab[(unsigned int)(hv >> 40) & 1023u];
                if (w != (unsigned int)s) {
                    const unsigned int* wr = L.masks + (size_t)w * L.MWS;
                    bool same = true;
                    for (int q = 0; q < L.MW; ++q) same = same && (wr[q] == row[q]);
                    if (same) L.stt[s] = 4;             // merged into entry w
                }
            }
            __syncthreads();
        }
        BK_ACC(1, t0);
        t0 = BK_NOW();
        // ---- compact the entries that are still live (order kept) ----
        if (tid == 0) L.misc[4] = 0;
        __syncthreads();
        for (int base = 0; base < nlive; base += nthr) {
            const int i = base + tid;
            const int s = i < nlive ? ord[i] : 0;
            const bool keep = i < nlive && L.stt[s] == 1;
            const unsigned long long bal = __ballot(keep);
            if (lane == 0) L.misc[8 + wv] = __popcll(bal);     // nthr <= 512: 8 waves
            __syncthreads();
            int off = L.misc[4];
            for (int q = 0; q < wv; ++q) off += L.misc[8 + q];
            if (keep) ord2[off + __popcll(bal & ((1ull << lane) - 1ull))] = (unsigned short)s;
            __syncthreads();
            if (tid == 0) { int t = L.misc[4]; for (int q = 0; q < nwv; ++q) t += L.misc[8 + q]; L.misc[4] = t; }
            __syncthreads();
        }
        nlive = L.misc[4];
        unsigned short* t = ord; ord = ord2; ord2 = t;
        __syncthreads();
        BK_ACC(2, t0);
    }
}

template <int LPW, bool DEDUPE>
__global__ __launch_bounds__(512, 3) void solve_lts_bucket_kernel(SArgs a, const double* __restrict__ xs, const double* __restrict__ xc, const double* __restrict__ xss,
                                                               int nunits) {
    extern __shared__ double sm[];
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int lane = tid & 63, wv = tid >> 6;
    const int u = a.u0 + blockIdx.x;
    const int band = a.unit_band[u];
    const int w = u - a.unit_off[band] + a.win_off[band];   // window index inside the band (global)
    const int P = a.npairs, S = a.nstarts, h = a.h;
    const int64_t o = (int64_t)band * a.vector_len + w;
    BkLds L = bk_carve((unsigned char*)sm, P, S, nthr >> 6, LPW, DEDUPE);
    L.nsample = a.nsample;
#ifdef NBLS_DEVELOPER      // phase stamps (same slots as the wave-per-unit kernel: nbls_debug_lts_stamps)
    unsigned long long* stp = (a.stamps && tid == 0 && (int)blockIdx.x < a.stamp_waves) ? a.stamps + (size_t)blockIdx.x * 8 : nullptr;
#define BK_STAMP(i) do { if (stp) stp[i] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define BK_STAMP(i) do { } while (0)
#endif
    BK_STAMP(0);
    // ---- prologue: tau, its MAD, MdCCM; scratch in the histogram space ----
    double* tmp = (double*)L.hist;
    double* srt = tmp + P;
    for (int k = tid; k < P; k += nthr) tmp[k] = fabs(tau_of(a, o * P + k));
    if (tid == 0) L.misc[0] = 0;
    __syncthreads();
    for (int k = tid; k < P; k += nthr) {
        const double vk = tmp[k];
        if (vk == vk) {
            int rank = 0;
            for (int j = 0; j < P; ++j) { const double vj = tmp[j]; rank += (vj < vk) || (vj == vk && j < k); }
            srt[rank] = vk;
            atomicAdd(&L.misc[0], 1);
        }
    }
    __syncthreads();
    int m = L.misc[0];
    const double med = (m & 1) ? srt[(m - 1) / 2] : (srt[m / 2 - 1] + srt[m / 2]) * 0.5;
    const double tmad = 1.4826 * med;
    __syncthreads();
    for (int k = tid; k < P; k += nthr) tmp[k] = a.cmax[o * P + k];
    if (tid == 0) L.misc[0] = 0;
    __syncthreads();
    for (int k = tid; k < P; k += nthr) {
        const double vk = tmp[k];
        if (vk == vk) {
            int rank = 0;
            for (int j = 0; j < P; ++j) { const double vj = tmp[j]; rank += (vj < vk) || (vj == vk && j < k); }
            srt[rank] = vk;
            atomicAdd(&L.misc[0], 1);
        }
    }
    __syncthreads();
    m = L.misc[0];
    if (tid == 0) a.mdccm[o] = m == 0 ? dnan() : ((m & 1) ? srt[(m - 1) / 2] : (srt[m / 2 - 1] + srt[m / 2]) * 0.5);
    __syncthreads();
    if (tmad == 0.0) {     // "data spike" [R]: not processed
        if (tid == 0) {
            a.vel[o] = dnan(); a.baz[o] = dnan(); a.sig[o] = dnan();
            a.z[2 * o] = dnan(); a.z[2 * o + 1] = dnan();
        }
        for (int k = tid; k < P; k += nthr) a.wts[o * P + k] = 1;
        return;
    }
    for (int k = tid; k < P; k += nthr) {
        const double yk = tau_of(a, o * P + k) / tmad;
        L.y[k] = yk;
        if ((k & 3) == 0) L.ys[k >> 2] = yk;
    }
    for (int q = tid; q < (nthr >> 6) * bk_hist_words(LPW); q += nthr) L.hist[q] = 0u;     // (behind the barrier below: tmp/srt are dead)
    __syncthreads();
    BK_STAMP(1);
    // ---- elemental starts: exact fit on the (up to four) points of the start, ascending index ----
    for (int s = tid; s < S; s += nthr) {
        int idx[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) idx[q] = a.starts[4 * s + q];
        double sxx = 0.0, sxy = 0.0, syy = 0.0, bx = 0.0, by = 0.0;
        int last = -1;
        for (int rep = 0; rep < 4; ++rep) {
            int best = 0x7fffffff;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (idx[q] > last && idx[q] < best) best = idx[q];
            if (best == 0x7fffffff) break;
            last = best;
            const double c0 = xs[2 * best], c1 = xs[2 * best + 1];
            sxx = sxx + c0 * c0;
            sxy = sxy + xc[best];
            syy = syy + c1 * c1;
            bx = bx + c0 * L.y[best];
            by = by + c1 * L.y[best];
        }
        const double det = sxx * syy - sxy * sxy;
        L.z0S[s] = (bx * syy - by * sxy) / det;
        L.z1S[s] = (by * sxx - bx * sxy) / det;
        L.prevS[s] = 0.0;
        L.thw[s] = 0x3ff0;                      // residuals are in units of the lags' MAD: 1.0 centres the first pass
        L.stt[s] = 1;
        L.ordA[s] = (unsigned short)s;
    }
    __syncthreads();
    BK_STAMP(2);
#ifdef NBLS_DEVELOPER
    unsigned long long* acc = stp ? a.stamps + (size_t)(a.stamp_waves + blockIdx.x) * 8 : nullptr;
    if (acc) for (int i = 0; i < 8; ++i) acc[i] = 0;
    if (a.stamp_mode == 2) acc = nullptr;       // per-wave busy cycles instead (bk_csteps)
    unsigned long long* wacc = (a.stamp_mode == 2 && a.stamps && lane == 0 && wv < 8 && (int)blockIdx.x < a.stamp_waves)
                                   ? a.stamps + (size_t)(a.stamp_waves + blockIdx.x) * 8 + wv : nullptr;
    __syncthreads();
    if (wacc) *wacc = 0;
#else
    unsigned long long* acc = nullptr;
#endif
    const BkSample smp{xss, L.ys, (P + 3) / 4, max(1, (h * ((P + 3) / 4) + P - 1) / P)};
    bk_csteps<LPW, DEDUPE>(L, xs, xc, P, h, a.csteps, P <= 255 ? 48 : 47, &smp, S, tid, nthr, acc BK_WACC_ARG);
    __syncthreads();
    BK_STAMP(3);

    // ---- the ncand best distinct finished starts by (objective, start index): repeated workgroup arg-min with
    //      duplicate knock-out (a rank count over all starts, 500 x 500 compares, was a fifth of the kernel) ----
    {
        double* wbest = L.wred;                         // [8] per-wave minima
        int* wbidx = (int*)(wbest + 8);                 // [8]
        if (tid == 0) L.misc[1] = 0;
        // a thread owns the entries s = tid, tid + nthr, ...; taken entries are struck off in stt (2 -> 3)
        for (int round = 0; round < S; ++round) {
            double bo = __builtin_inf();
            int bs = 0x7fffffff;
            for (int s = tid; s < S; s += nthr) {
                if (L.stt[s] != 2) continue;
                const double os = L.prevS[s];
                if (!(os < __builtin_inf())) continue;          // NaN / inf objectives never become candidates
                if (os < bo) { bo = os; bs = s; }               // ascending s: the lowest index wins ties inside a thread
            }
            // wave arg-min of (bo, bs)
            const double wm = nbls_wave::min_f64(bo);
            const unsigned long long mine = __ballot(bo == wm && bs != 0x7fffffff);
            int ws = 0x7fffffff;
            if (mine) {
                // the lowest start index among the lanes that hold the minimum
                int cand_s = (bo == wm && bs != 0x7fffffff) ? bs : 0x7fffffff;
                for (int off = 32; off > 0; off >>= 1) cand_s = min(cand_s, __shfl_xor(cand_s, off, 64));
                ws = cand_s;
            }
            if (lane == 0) { wbest[wv] = wm; wbidx[wv] = ws; }
            __syncthreads();
            if (tid == 0) {
                double gb = __builtin_inf();
                int gs_ = 0x7fffffff;
                for (int q = 0; q < (nthr >> 6); ++q) {
                    const int qs = wbidx[q];
                    if (qs == 0x7fffffff) continue;
                    const double qo = wbest[q];
                    if (qo < gb || (qo == gb && qs < gs_)) { gb = qo; gs_ = qs; }
                }
                int stop = 1;
                if (gs_ != 0x7fffffff) {
                    stop = 0;
                    int nc = L.misc[1];
                    bool dup = false;
                    for (int c = 0; c < nc; ++c) {
                        const int cs = L.cand[c];
                        if (L.prevS[cs] == gb && L.z0S[cs] == L.z0S[gs_] && L.z1S[cs] == L.z1S[gs_]) { dup = true; break; }
                    }
                    if (!dup) { L.cand[nc++] = gs_; L.misc[1] = nc; }
                    L.stt[gs_] = dup ? 3 : 5;           // struck off; 5 = accepted candidate (its objective stays in prevS)
                    if (nc >= a.ncand) stop = 1;
                }
                L.misc[3] = stop;
            }
            __syncthreads();
            if (L.misc[3]) break;
        }
    }
    __syncthreads();
    const int nc = L.misc[1];
    // ---- refine the candidates to convergence: only they are live ----
    if (tid < nc) {
        const int s = L.cand[tid];
        L.stt[s] = 1;
        L.prevS[s] = 0.0;
        L.ordA[tid] = (unsigned short)s;
    }
    __syncthreads();
    BK_STAMP(4);
    bk_csteps<LPW, false>(L, xs, xc, P, h, a.csteps2, P <= 255 ? 48 : 47, nullptr, nc, tid, nthr, acc);
    __syncthreads();
    BK_STAMP(5);
    // ---- best candidate -> de-standardise ----
    double zr0 = dnan(), zr1 = dnan();
    {
        double best = __builtin_inf();
        for (int c = 0; c < nc; ++c) {
            const int s = L.cand[c];
            const double ob = L.stt[s] == 2 ? L.prevS[s] : dnan();
            if (ob < best) { best = ob; zr0 = L.z0S[s]; zr1 = L.z1S[s]; }
        }
        zr0 = zr0 * tmad / a.xmad0;
        zr1 = zr1 * tmad / a.xmad1;
    }
    const bool finite_z = (zr0 - zr0 == 0.0) && (zr1 - zr1 == 0.0);
    if (!finite_z) {
        if (tid == 0) {
            a.vel[o] = dnan(); a.baz[o] = dnan(); a.sig[o] = dnan();
            a.z[2 * o] = dnan(); a.z[2 * o + 1] = dnan();
        }
        for (int k = tid; k < P; k += nthr) a.wts[o * P + k] = 1;
        return;
    }
    // ---- finish in original units; scratch in the histogram space: tauv, x0, x1, res [P], wsh [P] ----
    double* tauv = (double*)L.hist;
    double* x0 = tauv + P;
    double* x1 = x0 + P;
    double* res = x1 + P;
    uint8_t* wsh = (uint8_t*)L.hist + bk_align16((size_t)4 * P * sizeof(double));
    __syncthreads();
    for (int k = tid; k < P; k += nthr) {
        const double tk = tau_of(a, o * P + k);
        const double c0 = a.xij[2 * k], c1 = a.xij[2 * k + 1];
        tauv[k] = tk;
        x0[k] = c0;
        x1[k] = c1;
        res[k] = (tk - c0 * zr0) - c1 * zr1;         // residual of the raw fit
    }
    __syncthreads();
    // raw scale from the h smallest residuals: stable rank of every |res_k| (keys compared as integers: the order
    // of the selections above), thread 0 sums
    for (int k = tid; k < P; k += nthr) {
        const unsigned long long kk = bk_key(res[k]);
        int rank = 0;
        for (int j = 0; j < P; ++j) {
            const unsigned long long kj = bk_key(res[j]);
            rank += (kj < kk) || (kj == kk && j < k);
        }
        wsh[k] = rank < h;
    }
    __syncthreads();
    if (tid == 0) {
        double ssq = 0.0;
        for (int k = 0; k < P; ++k) ssq = __builtin_fma(res[k] * res[k], (double)wsh[k], ssq);
        L.cres[0] = sqrt(ssq / (double)h) * a.raw_factor;
    }
    __syncthreads();
    const double s0 = L.cres[0];
    const bool tiny = fabs(s0) < a.zero_scale;
    for (int k = tid; k < P; k += nthr)
        wsh[k] = tiny ? (fabs(res[k]) < a.zero_scale) : (fabs(res[k] / s0) <= a.quantile);
    __syncthreads();
    if (tid == 0) {
        double zf0 = zr0, zf1 = zr1;
        if (!tiny) {
            int nw = 0;
            double sxx = 0.0, sxy = 0.0, syy = 0.0, bx = 0.0, by = 0.0;
            for (int k = 0; k < P; ++k) {
                const double wk = (double)wsh[k];
                const double c0 = x0[k], c1 = x1[k], tk = tauv[k];
                nw += wsh[k];
                sxx = __builtin_fma(c0 * c0, wk, sxx);
                sxy = __builtin_fma(c0 * c1, wk, sxy);
                syy = __builtin_fma(c1 * c1, wk, syy);
                bx = __builtin_fma(c0 * tk, wk, bx);
                by = __builtin_fma(c1 * tk, wk, by);
            }
            const double det = sxx * syy - sxy * sxy;
            zf0 = (bx * syy - by * sxy) / det;
            zf1 = (by * sxx - bx * sxy) / det;
            L.misc[2] = nw;
        }
        L.cres[1] = zf0;
        L.cres[2] = zf1;
    }
    __syncthreads();
    const double zf0 = L.cres[1], zf1 = L.cres[2];
    for (int k = tid; k < P; k += nthr) res[k] = (tauv[k] - x0[k] * zf0) - x1[k] * zf1;
    __syncthreads();
    if (!tiny) {
        if (tid == 0) {
            const int nw = L.misc[2];
            double ssw = 0.0;
            for (int k = 0; k < P; ++k) ssw = __builtin_fma(res[k] * res[k], (double)wsh[k], ssw);
            L.cres[3] = nw > 1 ? sqrt(ssw / (double)(nw - 1)) * a.rew[nw] : 0.0;
        }
        __syncthreads();
        const double scale = L.cres[3];
        if (scale > 0.0)
            for (int k = tid; k < P; k += nthr) wsh[k] = fabs(res[k] / scale) <= a.quantile;
        __syncthreads();
    }
    if (tid == 0) {
        int nw = 0;
        double acc = 0.0;
        for (int k = 0; k < P; ++k) {
            nw += wsh[k];
            acc = __builtin_fma(tauv[k] * res[k], (double)wsh[k], acc);
        }
        double vel, baz;
        vel_baz(zf0, zf1, &vel, &baz);
        a.vel[o] = vel;
        a.baz[o] = baz;
        a.sig[o] = nw > 2 ? sqrt(acc / (double)(nw - 2)) : dnan();
        a.z[2 * o] = zf0;
        a.z[2 * o + 1] = zf1;
    }
    __syncthreads();
    for (int k = tid; k < P; k += nthr) a.wts[o * P + k] = wsh[k];
    BK_STAMP(6);
#ifdef NBLS_DEVELOPER
    if (stp) stp[7] = (unsigned long long)nc;
#endif
}
