// A pass's windows grouped into detections: connected components ("families", after PMCC) of the eligible cells of the
// result lattice under a link of neighbouring bands, nearby window centres and agreeing back-azimuth and velocity
// (nbls_set_families / nbls_label_families; the definition is in include/nbls.h and is followed literally).
//
// Mapping: one thread per cell, eight kernels on one stream, a kernel boundary between any two phases.
//   family_init_kernel     eligibility; parent[cell] = cell, or -1 for a cell that is not eligible; the root statistics reset
//   family_union_kernel    every eligible cell enumerates its linked neighbours of SMALLER cell index (bands b' <= b in reach;
//                          the closed window range of condition 3 by integer division, clipped to the row's windows) and
//                          unites itself with each: lock-free union-find, path halving, and one compare-and-swap that hooks
//                          the larger root under the smaller.  A parent only ever decreases, so every chain is strictly
//                          descending (bounded by the cell count), and the final root is the component's smallest cell.
//                          Every access to parent[] in this kernel is an agent-scope relaxed atomic load or CAS: a plain load
//                          could be served from an L1 line another compute unit has since overwritten.  No wave waits for
//                          another: a failed CAS means another wave hooked that root, and the loop finds the new root itself.
//   family_flatten_kernel  parent[cell] = its root; count, band_hi, sample_first, sample_end and the order-preserving image of
//                          the largest MdCCM accumulated on the root's record with integer add / min / max (vector atomics)
//   family_peak_kernel     the smallest cell among those whose MdCCM image equals the root's maximum
//   family_sums_kernel, family_scan_kernel, family_ids_kernel    a device-wide exclusive scan over "root with count >=
//                          min_pixels": block sums, a scan of the sums by one workgroup that walks them in chunks (any cell
//                          count), and the ids with the table rows; ascending root = ascending smallest cell
//   family_label_kernel    family[cell] = the root's id, -2 (component too small) or -1 (not eligible)
// Integer atomics commute, the value links are plain compares: the results are a function of the inputs alone.
// No LDS beyond the scan's 256 counters, no scratch; results leave by plain vector stores.
#include "nbls_internal.h"

namespace {

constexpr int FAM_THREADS = 256;
#define FAM_RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

struct FArgs {
    nbls_family_params p;
    int gate;                   // 1: the sigma_tau gate is on (sigma_tau_max is not NaN)
    int rows, nseg, vector_len;
    int64_t ncells;
    const int32_t* Wb;          // [rows]
    const int32_t* incb;        // [rows]
    const int32_t* nwin;        // [rows]
    const double *vel, *baz, *mdccm, *sig;      // [rows][vector_len]
    nbls_family_work::ptrs w;
    int32_t* family;            // [rows][vector_len]
    int64_t* table;             // [table_rows][8]
    int64_t table_rows;
    int32_t* nfam;
    int64_t nblocks;            // blocks of FAM_THREADS cells
};

__device__ inline bool fam_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }      // (false for NaN and +-inf)

// order-preserving integer image of a finite double; -0.0 and +0.0 compare equal, so both take +0.0's image
__device__ inline unsigned long long fam_key(double m) {
    if (m == 0.0) m = 0.0;
    const unsigned long long b = (unsigned long long)__double_as_longlong(m);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ inline int64_t fam_floor_div(int64_t a, int64_t d) {        // d > 0
    const int64_t q = a / d;
    return (a % d != 0 && a < 0) ? q - 1 : q;
}

__device__ inline int32_t fam_load(int32_t* parent, int64_t i) { return __hip_atomic_load(parent + i, FAM_RLX); }

// the root of x, halving the path on the way; the chain descends strictly, `bound` steps are never needed
__device__ inline int32_t fam_find(int32_t* parent, int32_t x, int64_t bound) {
    for (int64_t it = 0; it < bound; ++it) {
        const int32_t p = fam_load(parent, x);
        if (p == x) return x;
        const int32_t gp = fam_load(parent, p);
        if (gp == p) return p;
        int32_t expect = p;
        __hip_atomic_compare_exchange_strong(parent + x, &expect, gp, __ATOMIC_RELAXED, FAM_RLX);     // (lost: another wave shortened it)
        x = gp;
    }
    return x;
}

// one component of a and b: the larger root is hooked under the smaller by one CAS; a lost CAS means that root has a parent
// now, and the next round starts from it.  Successful hooks number fewer than the cells, which bounds the rounds.
__device__ inline void fam_unite(int32_t* parent, int32_t a, int32_t b, int64_t bound) {
    for (int64_t it = 0; it <= bound; ++it) {
        a = fam_find(parent, a, bound);
        b = fam_find(parent, b, bound);
        if (a == b) return;
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        int32_t expect = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &expect, lo, __ATOMIC_RELAXED, FAM_RLX)) return;
        a = hi; b = lo;
    }
}

__global__ __launch_bounds__(FAM_THREADS) void family_init_kernel(FArgs a) {
    const int64_t cell = (int64_t)blockIdx.x * FAM_THREADS + threadIdx.x;
    if (cell >= a.ncells) return;
    const int r = (int)(cell / a.vector_len), w = (int)(cell - (int64_t)r * a.vector_len);
    bool ok = w < a.nwin[r];
    if (ok) {
        const double v = a.vel[cell], z = a.baz[cell], m = a.mdccm[cell];
        ok = fam_finite(v) && fam_finite(z) && fam_finite(m) && m >= a.p.mdccm_min && a.p.vel_min <= v && v <= a.p.vel_max;
        if (ok && a.gate) ok = a.sig[cell] <= a.p.sigma_tau_max;              // (a NaN fails the gate)
    }
    a.w.parent[cell] = ok ? (int32_t)cell : -1;
    a.w.count[cell] = 0;
    a.w.band_hi[cell] = -1;
    a.w.peak[cell] = 0x7fffffff;
    a.w.fid[cell] = -1;
    a.w.smin[cell] = ~0ull;
    a.w.smax[cell] = 0ull;
    a.w.key[cell] = 0ull;
}

__global__ __launch_bounds__(FAM_THREADS) void family_union_kernel(FArgs a) {
    const int64_t cell = (int64_t)blockIdx.x * FAM_THREADS + threadIdx.x;
    if (cell >= a.ncells) return;
    int32_t* parent = a.w.parent;
    if (fam_load(parent, cell) < 0) return;                                  // (-1 never changes)
    const int r = (int)(cell / a.vector_len), w = (int)(cell - (int64_t)r * a.vector_len);
    const int b = r / a.nseg, s = r - b * a.nseg;
    const int64_t inc = a.incb[r], c2 = 2 * (int64_t)w * inc + a.Wb[r];
    const double v = a.vel[cell], z = a.baz[cell];
    const int blo = b - a.p.band_reach > 0 ? b - a.p.band_reach : 0;
    for (int bb = blo; bb <= b; ++bb) {
        const int rr = bb * a.nseg + s;
        const int64_t inc2 = a.incb[rr], W2 = a.Wb[rr];
        const int64_t T = 2 * (int64_t)a.p.time_reach * (inc > inc2 ? inc : inc2);
        // |c2 - (2 w' inc' + W')| <= T   <=>   ceil((c2 - T - W') / (2 inc')) <= w' <= floor((c2 + T - W') / (2 inc'))
        int64_t lo = -fam_floor_div(-(c2 - T - W2), 2 * inc2), hi = fam_floor_div(c2 + T - W2, 2 * inc2);
        if (lo < 0) lo = 0;
        if (hi > (int64_t)a.nwin[rr] - 1) hi = (int64_t)a.nwin[rr] - 1;
        if (bb == b && hi > (int64_t)w - 1) hi = (int64_t)w - 1;             // smaller cell index only
        const int64_t base = (int64_t)rr * a.vector_len;
        for (int64_t ww = lo; ww <= hi; ++ww) {
            const int64_t other = base + ww;
            if (fam_load(parent, other) < 0) continue;
            double d = fabs(z - a.baz[other]);
            if (d > 180.0) d = 360.0 - d;
            if (!(d <= a.p.baz_tol) || !(fabs(v - a.vel[other]) <= a.p.vel_tol)) continue;
            fam_unite(parent, (int32_t)cell, (int32_t)other, a.ncells);
        }
    }
}

__global__ __launch_bounds__(FAM_THREADS) void family_flatten_kernel(FArgs a) {
    const int64_t cell = (int64_t)blockIdx.x * FAM_THREADS + threadIdx.x;
    if (cell >= a.ncells) return;
    int32_t* parent = a.w.parent;
    int32_t root = fam_load(parent, cell);
    if (root < 0) return;
    // read-only walk (others flatten their own cell meanwhile: whatever a load returns is an ancestor)
    for (int64_t it = 0; it < a.ncells; ++it) {
        const int32_t p = fam_load(parent, root);
        if (p == root) break;
        root = p;
    }
    __hip_atomic_store(parent + cell, root, FAM_RLX);
    const int r = (int)(cell / a.vector_len), w = (int)(cell - (int64_t)r * a.vector_len);
    const unsigned long long s0 = (unsigned long long)((int64_t)w * a.incb[r]);
    atomicAdd(a.w.count + root, 1);
    atomicMax(a.w.band_hi + root, r / a.nseg);
    atomicMin(a.w.smin + root, s0);
    atomicMax(a.w.smax + root, s0 + (unsigned long long)a.Wb[r]);
    atomicMax(a.w.key + root, fam_key(a.mdccm[cell]));
}

__global__ __launch_bounds__(FAM_THREADS) void family_peak_kernel(FArgs a) {
    const int64_t cell = (int64_t)blockIdx.x * FAM_THREADS + threadIdx.x;
    if (cell >= a.ncells) return;
    const int32_t root = a.w.parent[cell];
    if (root < 0) return;
    if (fam_key(a.mdccm[cell]) == a.w.key[root]) atomicMin(a.w.peak + root, (int32_t)cell);
}

__device__ inline int fam_flag(const FArgs& a, int64_t cell) {
    return cell < a.ncells && a.w.parent[cell] == (int32_t)cell && a.w.count[cell] >= a.p.min_pixels ? 1 : 0;
}

// inclusive scan of one value per thread over the workgroup; -> the thread's inclusive sum, total in *total
__device__ inline int fam_block_scan(int v, int* lds, int* total) {
    const int tid = threadIdx.x;
    lds[tid] = v;
    __syncthreads();
    for (int o = 1; o < FAM_THREADS; o <<= 1) {
        const int t = tid >= o ? lds[tid - o] : 0;
        __syncthreads();
        lds[tid] += t;
        __syncthreads();
    }
    const int inc = lds[tid];
    *total = lds[FAM_THREADS - 1];
    __syncthreads();
    return inc;
}

__global__ __launch_bounds__(FAM_THREADS) void family_sums_kernel(FArgs a) {
    __shared__ int lds[FAM_THREADS];
    int total;
    fam_block_scan(fam_flag(a, (int64_t)blockIdx.x * FAM_THREADS + threadIdx.x), lds, &total);
    if (threadIdx.x == 0) a.w.sums[blockIdx.x] = total;
}

// one workgroup: sums[] -> its exclusive scan, chunk after chunk with a running carry; the total is the family count
__global__ __launch_bounds__(FAM_THREADS) void family_scan_kernel(FArgs a) {
    __shared__ int lds[FAM_THREADS];
    int carry = 0;
    for (int64_t k0 = 0; k0 < a.nblocks; k0 += FAM_THREADS) {
        const int64_t k = k0 + threadIdx.x;
        const int v = k < a.nblocks ? a.w.sums[k] : 0;
        int total;
        const int inc = fam_block_scan(v, lds, &total);
        if (k < a.nblocks) a.w.sums[k] = carry + inc - v;
        carry += total;
    }
    if (threadIdx.x == 0) *a.nfam = carry;
}

__global__ __launch_bounds__(FAM_THREADS) void family_ids_kernel(FArgs a) {
    __shared__ int lds[FAM_THREADS];
    const int64_t cell = (int64_t)blockIdx.x * FAM_THREADS + threadIdx.x;
    const int f = fam_flag(a, cell);
    int total;
    const int inc = fam_block_scan(f, lds, &total);
    if (!f) return;
    const int32_t id = a.w.sums[blockIdx.x] + inc - 1;
    a.w.fid[cell] = id;
    if (id >= a.table_rows) return;
    const int r = (int)(cell / a.vector_len);
    int64_t* t = a.table + 8 * (int64_t)id;
    t[0] = a.w.count[cell];
    t[1] = cell;
    t[2] = a.w.peak[cell];
    t[3] = r / a.nseg;                           // the smallest cell lies in the component's lowest band
    t[4] = a.w.band_hi[cell];
    t[5] = r % a.nseg;
    t[6] = (int64_t)a.w.smin[cell];
    t[7] = (int64_t)a.w.smax[cell];
}

__global__ __launch_bounds__(FAM_THREADS) void family_label_kernel(FArgs a) {
    const int64_t cell = (int64_t)blockIdx.x * FAM_THREADS + threadIdx.x;
    if (cell >= a.ncells) return;
    const int32_t root = a.w.parent[cell];
    int32_t out = -1;
    if (root >= 0) {
        const int32_t id = a.w.fid[root];
        out = id >= 0 ? id : -2;
    }
    a.family[cell] = out;
}

}  // namespace

size_t nbls_family_table_rows_of(int64_t ncells, int min_pixels) {
    const int64_t f = ncells / (min_pixels > 0 ? min_pixels : 1);
    return (size_t)(f > 0 ? f : 1);
}

hipError_t nbls_family_work::grow(int64_t ncells, int min_pixels) {
    const size_t n = (size_t)(ncells > 0 ? ncells : 1), nb = (n + FAM_THREADS - 1) / FAM_THREADS;
    hipError_t e;
    if ((e = parent.grow(n * sizeof(int32_t))) != hipSuccess) return e;
    if ((e = count.grow(n * sizeof(int32_t))) != hipSuccess) return e;
    if ((e = band_hi.grow(n * sizeof(int32_t))) != hipSuccess) return e;
    if ((e = peak.grow(n * sizeof(int32_t))) != hipSuccess) return e;
    if ((e = fid.grow(n * sizeof(int32_t))) != hipSuccess) return e;
    if ((e = smin.grow(n * sizeof(unsigned long long))) != hipSuccess) return e;
    if ((e = smax.grow(n * sizeof(unsigned long long))) != hipSuccess) return e;
    if ((e = key.grow(n * sizeof(unsigned long long))) != hipSuccess) return e;
    if ((e = sums.grow(nb * sizeof(int32_t))) != hipSuccess) return e;
    if ((e = family.grow(n * sizeof(int32_t))) != hipSuccess) return e;
    if ((e = table.grow(nbls_family_table_rows_of(ncells, min_pixels) * 8 * sizeof(int64_t))) != hipSuccess) return e;
    return nfam.grow(sizeof(int32_t));
}

hipError_t nbls_launch_families(const nbls_family_params& p, nbls_family_work& wk, int rows, int nseg, int vector_len,
                                const int32_t* d_W, const int32_t* d_inc, const int32_t* d_nwin, const double* vel, const double* baz,
                                const double* mdccm, const double* sig, hipStream_t st) {
    FArgs a{};
    a.p = p;
    a.gate = p.sigma_tau_max == p.sigma_tau_max ? 1 : 0;                     // (off iff sigma_tau_max is NaN)
    a.rows = rows; a.nseg = nseg; a.vector_len = vector_len;
    a.ncells = (int64_t)rows * vector_len;
    a.Wb = d_W; a.incb = d_inc; a.nwin = d_nwin;
    a.vel = vel; a.baz = baz; a.mdccm = mdccm; a.sig = sig;
    a.w = {wk.parent, wk.count, wk.band_hi, wk.peak, wk.fid, wk.smin, wk.smax, wk.key, wk.sums};
    a.family = wk.family; a.table = wk.table; a.nfam = wk.nfam;
    a.table_rows = (int64_t)nbls_family_table_rows_of(a.ncells, p.min_pixels);
    a.nblocks = (a.ncells + FAM_THREADS - 1) / FAM_THREADS;
    // (the callers have refused all of this)
    if (rows < 1 || nseg < 1 || rows % nseg || vector_len < 1 || a.ncells >= ((int64_t)1 << 31) || !d_W || !d_inc || !d_nwin || !vel ||
        !baz || !mdccm || (a.gate && !sig) || !wk.parent || !wk.table || !wk.nfam || !wk.family || p.min_pixels < 1 || p.time_reach < 1 ||
        p.band_reach < 0)
        return hipErrorInvalidValue;
    if (wk.parent.cap < (size_t)a.ncells * sizeof(int32_t) || wk.table.cap < (size_t)a.table_rows * 8 * sizeof(int64_t) ||
        wk.sums.cap < (size_t)a.nblocks * sizeof(int32_t))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)a.nblocks), block(FAM_THREADS);
    hipLaunchKernelGGL(family_init_kernel, grid, block, 0, st, a);
    hipLaunchKernelGGL(family_union_kernel, grid, block, 0, st, a);
    hipLaunchKernelGGL(family_flatten_kernel, grid, block, 0, st, a);
    hipLaunchKernelGGL(family_peak_kernel, grid, block, 0, st, a);
    hipLaunchKernelGGL(family_sums_kernel, grid, block, 0, st, a);
    hipLaunchKernelGGL(family_scan_kernel, dim3(1), block, 0, st, a);
    hipLaunchKernelGGL(family_ids_kernel, grid, block, 0, st, a);
    hipLaunchKernelGGL(family_label_kernel, grid, block, 0, st, a);
    return hipGetLastError();
}
