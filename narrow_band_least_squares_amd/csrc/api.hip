// C ABI of libnbls_hip.so (see include/nbls.h): handle, HBM buffers, plan, launch order.
#include "nbls_internal.h"
#include <algorithm>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <unistd.h>

namespace {

std::mutex g_err_mu;
std::string g_err;   // error of a failed nbls_create

int fail(nbls_handle* h, int code, const std::string& msg) {
    if (h) { std::lock_guard<std::mutex> l(h->err_mu); h->err = msg; }
    else { std::lock_guard<std::mutex> l(g_err_mu); g_err = msg; }
    return code;
}

#define HIPCHK(h, call)                                                                        \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(h, e_ == hipErrorOutOfMemory ? NBLS_ERR_NOMEM : NBLS_ERR_HIP,          \
                        std::string(#call) + ": " + hipGetErrorString(e_));                    \
    } while (0)

// Blocking copy ON THE HANDLE'S STREAM.  The streams are non-blocking (hipStreamNonBlocking) and nothing in
// the library touches the NULL stream: a plain hipMemcpy would wait for every other handle of the process
// that is busy on this GPU (the band groups of a pipelined call run on several handles at once).
hipError_t copy_sync(nbls_handle* h, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, h->stream);
    if (e != hipSuccess) return e;
    e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess) h->work_queued = false;       // (the solve stream is joined into this one at the end of a pass)
    return e;
}

// A buffer's grow as the API's result: `what` is the allocator call the error text names.
int grown(nbls_handle* h, hipError_t e, const char* what) {
    if (e == hipSuccess) return 0;
    return fail(h, e == hipErrorOutOfMemory ? NBLS_ERR_NOMEM : NBLS_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// A work or result buffer of at least need_bytes; contents are not kept.
template <typename T>
int ensure(nbls_handle* h, dev_buf<T>& b, size_t need_bytes) {
    const hipError_t e = b.grow(need_bytes);
    if (e != hipSuccess)
        return fail(h, NBLS_ERR_NOMEM, std::string("hipMalloc(") + std::to_string(need_bytes ? need_bytes : 8) + "): " + hipGetErrorString(e));
    return 0;
}

// Upload a small plan table.  The allocation is kept and reused while it is big enough (hipFree
// synchronises the device and hipMalloc is slow: a plan uploads ~15 of these).
template <typename T>
int alloc_copy(nbls_handle* h, dev_buf<T>& p, const T* src, size_t n) {
    const size_t need = (n ? n : 1) * sizeof(T);
    {
        const size_t slot = (need + 63) & ~(size_t)63;
        if (h->arena_mode && h->stage && h->d_parena && h->stage_used + slot <= h->stage.cap) {
            // a table of nbls_plan: a place in the arena, no copy of its own (StreamGuard sends the arena in one piece)
            if (n) memcpy(h->stage + h->stage_used, src, n * sizeof(T));
            p.place((T*)(h->d_parena + h->stage_used));
            h->stage_used += slot;
            return 0;
        }
    }
    p.leave_arena();                                                 // back to an allocation of its own
    if (int rc = grown(h, p.grow(need), "hipMalloc((void**)p, need)")) return rc;
    // queued on the handle's UPLOAD stream (highest priority: a plan made while other handles' passes fill the GPU
    // must not wait behind them — on a low-priority compute stream the ~15 small copies of a plan took 5 ms instead
    // of 0.3); nbls_plan / nbls_set_geometry wait for that stream before they return (StreamGuard), i.e. before the
    // host buffers go away and before any kernel that reads the tables can be launched
    if (n) {
        const size_t bytes = n * sizeof(T), slot = (bytes + 63) & ~(size_t)63;
        const void* from = src;
        if (h->stage && h->stage_used + slot <= h->stage.cap) {      // through the pinned arena (reset by StreamGuard)
            memcpy(h->stage + h->stage_used, src, bytes);
            from = h->stage + h->stage_used;
            h->stage_used += slot;
        } else {
            h->stage_bypass = true;                                  // the caller's buffer is read: the guard has to wait
        }
        HIPCHK(h, hipMemcpyAsync(p, from, bytes, hipMemcpyHostToDevice, h->up));
    }
    return 0;
}

// Host-side linear algebra of the DF2T cascade (state order [s1_0, s2_0, s1_1, s2_1, ...]), in long
// double: one step is s' = A s + g x.  Returns, for a chunk of C samples and carry groups of G chunks,
//   fw[t][d]    = (A^(C-1-t) g)[d]         zero-state end state  e = sum_t fw[t] x_t
//   mpow[j]     = (A^C)^j, j = 0..G        chunk / group transitions
// Waits for the handle's upload stream when the enclosing API call returns, on every exit path: host tables that
// alloc_copy queued must have been read by then.
// On entry the upload stream is made to wait (GPU-side, on this handle's own streams only: other handles' passes
// are not touched) for whatever pass of THIS handle is still queued: nbls_execute is asynchronous, and the tables a
// plan overwrites (d_sos, d_fw, d_M, d_unit_*, d_W, d_starts, d_xs, ...) may be under running kernels.
struct StreamGuard {
    nbls_handle* h;
    explicit StreamGuard(nbls_handle* hh) : h(hh) {
        // the staging arena of alloc_copy: everything queued from it has been read when the previous guard left
        if (!h->stage && h->stage.grow((size_t)8 << 20) != hipSuccess) (void)hipGetLastError();
        if (h->up_pending) { (void)hipStreamSynchronize(h->up); h->up_pending = false; }     // the arena is free again
        h->stage_used = 0;
        h->stage_bypass = false;
        if (h->stage && !h->d_parena && h->d_parena.grow(h->stage.cap) != hipSuccess) (void)hipGetLastError();
        if (!h->ev_up && hipEventCreateWithFlags(&h->ev_up, hipEventDisableTiming) != hipSuccess) { h->ev_up = nullptr; (void)hipGetLastError(); }
        if (h->work_queued && h->up != h->stream && h->ev_plan) {
            for (hipStream_t s : {h->stream, h->stream2}) {
                if (!s) continue;
                if (hipEventRecord(h->ev_plan, s) == hipSuccess) (void)hipStreamWaitEvent(h->up, h->ev_plan, 0);
            }
        }
    }
    ~StreamGuard() {
        h->arena_mode = false;                           // (a plan that failed half-way: its tables are never used)
        // everything came from the arena: nothing of the caller's is still being read, and the kernels that need the
        // tables are ordered behind ev_up on the GPU (wait_uploads) — the host does not wait for the copies
        if (!h->stage_bypass && h->stage && h->ev_up && hipEventRecord(h->ev_up, h->up) == hipSuccess) { h->up_pending = true; return; }
        (void)hipStreamSynchronize(h->up);
    }
};

// GPU-side: the handle's compute streams wait for the plan / geometry tables still on their way (see ev_up).
void wait_uploads(nbls_handle* h) {
    if (!h->up_pending || !h->ev_up) return;
    for (hipStream_t s : {h->stream, h->stream2})
        if (s && s != h->up) (void)hipStreamWaitEvent(s, h->ev_up, 0);
}

// A few host threads kept asleep between plans (filter tables: long-double arithmetic, 30-100 us per band, on the critical
// path of every call — the GPU has nothing to do until the plan is through).  Starting a thread costs ~15 us, one after
// the other on the planning thread: eleven of them were a third of the 0.5 ms the tables of 48 bands took.  One job at a
// time; a second planner (the launch threads of a multi-GPU call plan side by side) computes its bands inline instead of
// waiting.  The pool is never destroyed (threads asleep at exit are simply gone with the process) and is rebuilt in a
// forked child, which inherits none of them.
struct TablePool {
    std::mutex m;
    std::condition_variable go, done;
    std::mutex busy;                       // held for the length of one job
    const std::function<void(int)>* job = nullptr;
    int njob = 0, left = 0;
    unsigned long gen = 0;
    int nthreads = 0;
    pid_t pid = 0;
    void worker(int t) {
        unsigned long seen = 0;
        for (;;) {
            const std::function<void(int)>* f;
            {
                std::unique_lock<std::mutex> l(m);
                go.wait(l, [&] { return gen != seen; });
                seen = gen;
                if (t >= njob) continue;
                f = job;
            }
            (*f)(t);
            std::lock_guard<std::mutex> l(m);
            if (--left == 0) done.notify_one();
        }
    }
};
TablePool* g_pool = nullptr;
std::mutex g_pool_mu;

// f(0) .. f(n-1), f(0) on the calling thread; returns false when the pool is taken (the caller then runs everything itself)
bool pool_run(int n, const std::function<void(int)>& f) {
    constexpr int kThreads = 12;
    TablePool* p;
    {
        std::lock_guard<std::mutex> l(g_pool_mu);
        if (!g_pool || g_pool->pid != getpid()) {
            p = new TablePool;                       // (an inherited pool of the parent process is left alone)
            p->pid = getpid();
            p->nthreads = kThreads;
            for (int t = 1; t < kThreads; ++t) std::thread(&TablePool::worker, p, t).detach();
            g_pool = p;
        }
        p = g_pool;
    }
    if (n > p->nthreads) return false;
    std::unique_lock<std::mutex> use(p->busy, std::try_to_lock);
    if (!use.owns_lock()) return false;
    if (n > 1) {
        std::lock_guard<std::mutex> l(p->m);
        p->job = &f;
        p->njob = n;
        p->left = n - 1;
        ++p->gen;
        p->go.notify_all();
    }
    f(0);
    if (n > 1) {
        std::unique_lock<std::mutex> l(p->m);
        p->done.wait(l, [&] { return p->left == 0; });
        p->job = nullptr;
    }
    return true;
}

void filter_tables(const double* sos, int S, int C, int G, double* fw, double* mpow) {
    constexpr int DM = 2 * NBLS_MAX_SECTIONS;
    const int D = 2 * S;
    typedef long double ld;
    // fixed-size stack matrices (D <= 16): this runs for every band of every plan
    auto step = [&](ld* st, ld x) {
        ld v = x;
        for (int s = 0; s < S; ++s) {
            const ld b0 = sos[s * 6 + 0], b1 = sos[s * 6 + 1], b2 = sos[s * 6 + 2];
            const ld a1 = sos[s * 6 + 4], a2 = sos[s * 6 + 5];
            const ld y = b0 * v + st[2 * s];
            const ld n1 = (b1 * v - a1 * y) + st[2 * s + 1];
            const ld n2 = b2 * v - a2 * y;
            st[2 * s] = n1;
            st[2 * s + 1] = n2;
            v = y;
        }
    };
    ld A[DM * DM], g[DM];
    for (int col = 0; col < D; ++col) {
        ld st[DM];
        for (int r = 0; r < D; ++r) st[r] = 0.0L;
        st[col] = 1.0L;
        step(st, 0.0L);
        for (int r = 0; r < D; ++r) A[r * D + col] = st[r];
    }
    for (int r = 0; r < D; ++r) g[r] = 0.0L;
    step(g, 1.0L);
    auto matmul = [&](const ld* X, const ld* Y, ld* o) {          // o = X Y (o distinct from X, Y)
        for (int i = 0; i < D; ++i)
            for (int j = 0; j < D; ++j) {
                ld acc = 0.0L;
                for (int k = 0; k < D; ++k) acc += X[i * D + k] * Y[k * D + j];
                o[i * D + j] = acc;
            }
    };
    // v = A^k g is the weight of sample t = C-1-k.  One DF2T step with input 0 IS the product A v
    // (A's columns were made by that same step), at O(S) instead of O(D^2) operations.
    ld v[DM];
    for (int d = 0; d < D; ++d) v[d] = g[d];
    for (int k = 0; k < C; ++k) {
        for (int d = 0; d < D; ++d) fw[(size_t)(C - 1 - k) * D + d] = (double)v[d];
        ld nv[DM];
        for (int i = 0; i < D; ++i) {
            ld acc = 0.0L;
            for (int q = 0; q < D; ++q) acc += A[i * D + q] * v[q];
            nv[i] = acc;
        }
        for (int d = 0; d < D; ++d) v[d] = nv[d];
    }
    ld M[DM * DM], Bm[DM * DM], T[DM * DM];                       // M = A^C by squaring
    for (int i = 0; i < D * D; ++i) { M[i] = 0.0L; Bm[i] = A[i]; }
    for (int i = 0; i < D; ++i) M[i * D + i] = 1.0L;
    for (int e = C; e > 0; e >>= 1) {
        if (e & 1) { matmul(M, Bm, T); for (int i = 0; i < D * D; ++i) M[i] = T[i]; }
        matmul(Bm, Bm, T);
        for (int i = 0; i < D * D; ++i) Bm[i] = T[i];
    }
    ld Pw[DM * DM];
    for (int i = 0; i < D * D; ++i) Pw[i] = 0.0L;
    for (int i = 0; i < D; ++i) Pw[i * D + i] = 1.0L;
    for (int j = 0; j <= G; ++j) {
        for (int i = 0; i < D * D; ++i) mpow[(size_t)j * D * D + i] = (double)Pw[i];
        matmul(Pw, M, T);
        for (int i = 0; i < D * D; ++i) Pw[i] = T[i];
    }
}

// Rank of a co-array [npairs][2] (2 unknowns): false for a collinear array.
bool coarray_full_rank(const double* xij, int npairs) {
    double sxx = 0, sxy = 0, syy = 0;
    for (int k = 0; k < npairs; ++k) { sxx += xij[2*k]*xij[2*k]; sxy += xij[2*k]*xij[2*k+1]; syy += xij[2*k+1]*xij[2*k+1]; }
    const double det = sxx * syy - sxy * sxy;
    return det > 1e-12 * (sxx + syy) * (sxx + syy);
}

// The LTS description of an array of P pairs; `who` is the caller's message prefix.
int check_lts(nbls_handle* h, const nbls_lts_params* l, int P, const std::string& who) {
    if (l->nstarts < 1 || l->nstarts > NBLS_MAX_STARTS || !l->starts || !l->rew_table) return fail(h, NBLS_ERR_ARG, who + "bad LTS starts");
    if (l->h < 2 || l->h > P) return fail(h, NBLS_ERR_ARG, who + "LTS h out of range");
    if (l->ncand < 1 || l->ncand > NBLS_MAX_CAND) return fail(h, NBLS_ERR_ARG, who + "ncand out of range");
    for (int i = 0; i < l->nstarts * 4; ++i)
        if (l->starts[i] >= P) return fail(h, NBLS_ERR_ARG, who + "start index out of range");
    return 0;
}

// The LTS tables of a record on the device: starts, reweighting table and the standardised co-array xs / xc / xss.
int upload_lts_tables(nbls_handle* h, nbls_estimator& x) {
    int rc;
    const int P = x.npairs;
    if ((rc = alloc_copy(h, x.d_starts, x.h_starts.data(), x.h_starts.size()))) return rc;
    if ((rc = alloc_copy(h, x.d_rew, x.h_rew.data(), x.h_rew.size()))) return rc;
    const int PP = P + 16;                           // padding: the large-array LTS kernel fetches one block of pairs ahead
    std::vector<double> xs((size_t)PP * 2, 0.0), xc((size_t)PP, 0.0);
    for (int k = 0; k < P; ++k) {
        xs[2 * k] = x.h_xij[2 * k] / x.ltsp.xij_mad[0];
        xs[2 * k + 1] = x.h_xij[2 * k + 1] / x.ltsp.xij_mad[1];
        xc[k] = xs[2 * k] * xs[2 * k + 1];
    }
    if ((rc = alloc_copy(h, x.d_xs, xs.data(), xs.size()))) return rc;
    if ((rc = alloc_copy(h, x.d_xc, xc.data(), xc.size()))) return rc;
    const int NS4 = (P + 3) / 4;                     // every 4th pair: the sample pass of the large-array LTS kernel
    std::vector<double> xss((size_t)(NS4 + 16) * 2, 0.0);
    for (int i = 0; i < NS4; ++i) { xss[2 * i] = xs[2 * (4 * i)]; xss[2 * i + 1] = xs[2 * (4 * i) + 1]; }
    return alloc_copy(h, x.d_xss, xss.data(), xss.size());
}

// Size a record's result buffers for `cells` result cells: every buffer has its own capacity (a smaller plan after a
// bigger one keeps the allocations).  The lag / cmax rows are the pass's own unless the record is a sub-array's
// (nbls_view_of); min_res: the least allocation of the result block (nbls_reserve_results).
int size_result_buffers(nbls_handle* h, nbls_estimator& x, size_t cells, size_t min_res) {
    int rc;
    const size_t P = x.d_xij ? (size_t)x.npairs : 1;     // (geometry is optional for a filter-only plan)
    const bool own = x.kept_pair.empty();
    x.mask_bytes = (int)((P + 7) / 8);
    x.res_bytes = cells * (4 * sizeof(double) + (size_t)x.mask_bytes);
    if ((rc = ensure(h, x.d_res, x.res_bytes > min_res ? x.res_bytes : min_res))) return rc;
    if ((rc = ensure(h, own ? h->d_lag : x.d_lag, cells * P * sizeof(int32_t)))) return rc;
    if ((rc = ensure(h, own ? h->d_cmax : x.d_cmax, cells * P * sizeof(double)))) return rc;
    if (h->req.refine && (rc = ensure(h, own ? h->d_lagfrac : x.d_lagfrac, cells * P * sizeof(double)))) return rc;
    if ((rc = ensure(h, x.d_z, 2 * cells * sizeof(double)))) return rc;
    if ((rc = ensure(h, x.d_wts, cells * P))) return rc;
    if (x.want_unc && (rc = ensure(h, x.d_unc, 2 * cells * sizeof(double)))) return rc;
    if (h->req.beam && (rc = ensure(h, x.d_beam, 2 * cells * sizeof(double)))) return rc;
    if (h->req.closure) {
        const size_t N = own ? (size_t)h->nelem : x.kept.size();
        if ((rc = ensure(h, x.d_closure, 2 * cells * sizeof(double)))) return rc;
        if ((rc = ensure(h, x.d_closure_el, cells * (N ? N : 1) * sizeof(double)))) return rc;
    }
    return 0;
}

// A streamed pass: the pinned mirror of a record's result block, large enough for the plan's block.
int ensure_mirror(nbls_handle* h, nbls_estimator& x) {
    if (x.h_res.cap >= x.res_bytes) return 0;
    HIPCHK(h, hipStreamSynchronize(h->cstream));             // (copies of the last pass may still write the old one)
    return grown(h, x.h_res.grow(x.res_bytes), "hipHostMalloc((void**)&x.h_res, x.res_bytes ? x.res_bytes : 8, hipHostMallocDefault)");
}

// The first window band b of the plan computed (0 unless window-sharded); it computed nwin[b] from there on.
int64_t first_window(const nbls_handle* h, int b) { return (int)h->woff.size() == h->nbands ? h->woff[b] : 0; }

// Rows of windows the plan did not compute (beyond a band's count, outside a window slice) are zeros in what a fetch
// returns: `out` is [B][VL] rows of row_bytes.
void zero_uncomputed(const nbls_handle* h, void* out, size_t row_bytes) {
    unsigned char* o = (unsigned char*)out;
    for (int b = 0; b < h->nbands; ++b) {
        const int64_t first = first_window(h, b), n = h->nwin[b];
        unsigned char* band = o + (size_t)b * h->vector_len * row_bytes;
        if (first > 0) memset(band, 0, (size_t)first * row_bytes);
        if (first + n < h->vector_len) memset(band + (size_t)(first + n) * row_bytes, 0, (size_t)(h->vector_len - first - n) * row_bytes);
    }
}

// One result plane of a fetch, [B][VL] rows of row_bytes, into `out` (NULL: the caller does not want it).  No pass clears
// these buffers: zeros until `valid` (a pass of this plan has run the stage that writes the plane; a later pass without
// that stage leaves it as it is), then the plane, with zeros where no window was computed.
int fetch_plane(nbls_handle* h, bool valid, void* out, const void* src, size_t row_bytes) {
    const size_t cells = (size_t)h->nbands * h->vector_len;
    if (!out) return NBLS_OK;
    if (!valid) { memset(out, 0, cells * row_bytes); return NBLS_OK; }
    HIPCHK(h, copy_sync(h, out, src, cells * row_bytes, hipMemcpyDeviceToHost));
    zero_uncomputed(h, out, row_bytes);
    return NBLS_OK;
}

}  // namespace

extern "C" {

int nbls_version(void) { return 200; }

const char* nbls_last_error(const nbls_handle* h) {
    if (h) return h->err.c_str();
    std::lock_guard<std::mutex> l(g_err_mu);
    return g_err.c_str();
}

int nbls_device_count(void) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) return 0;
    return ndev;
}

int nbls_create(int device_id, nbls_handle** out) {
    if (!out) return fail(nullptr, NBLS_ERR_ARG, "nbls_create: out is NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, NBLS_ERR_HIP, std::string("no HIP device available: ") + hipGetErrorString(e));
    if (device_id < 0 || device_id >= ndev)
        return fail(nullptr, NBLS_ERR_ARG, "nbls_create: device_id out of range");
    nbls_handle* h = new nbls_handle();
    h->device = device_id;
    if ((e = hipSetDevice(device_id)) != hipSuccess || (e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)) != hipSuccess) {
        delete h;
        return fail(nullptr, NBLS_ERR_HIP, std::string("device init: ") + hipGetErrorString(e));
    }
    (void)hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking);
    {
        int least = 0, greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) greatest = 0;
        if (hipStreamCreateWithPriority(&h->up, hipStreamNonBlocking, greatest) != hipSuccess) {
            h->up = h->stream;             // no priorities on this device: uploads share the compute stream
            (void)hipGetLastError();
        }
    }
    if (hipDeviceGetAttribute(&h->num_cus, hipDeviceAttributeMultiprocessorCount, device_id) != hipSuccess) h->num_cus = 0;
    for (int i = 0; i < 4; ++i) (void)hipEventCreate(&h->ev[i]);
    if (hipEventCreateWithFlags(&h->ev_xd, hipEventDisableTiming) != hipSuccess) { h->ev_xd = nullptr; (void)hipGetLastError(); }
    if (hipEventCreateWithFlags(&h->ev_plan, hipEventDisableTiming) != hipSuccess) { h->ev_plan = nullptr; (void)hipGetLastError(); }
    *out = h;
    return NBLS_OK;
}

void nbls_destroy(nbls_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    // nothing is freed or destroyed under queued work (the solve stream is joined into `stream` at the end of a pass)
    for (hipStream_t s : {h->stream, h->stream2, h->up, h->cstream, h->ustream})
        if (s) (void)hipStreamSynchronize(s);
    (void)nbls_comm_destroy(h);
    for (int i = 0; i < 4; ++i) if (h->ev[i]) (void)hipEventDestroy(h->ev[i]);
    for (hipEvent_t e : h->bev) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->pev) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->rev) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->uev) (void)hipEventDestroy(e);
    for (hipEvent_t e : {h->ev_uprev, h->ev_xd, h->ev_plan, h->ev_up, h->ev_capon_slab, h->ev_music_slab})
        if (e) (void)hipEventDestroy(e);
    if (h->cstream) (void)hipStreamDestroy(h->cstream);
    if (h->ustream) (void)hipStreamDestroy(h->ustream);
    if (h->up && h->up != h->stream) (void)hipStreamDestroy(h->up);
    if (h->stream2) (void)hipStreamDestroy(h->stream2);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;                                // the buffers free themselves (dev_buf.h), on the handle's device
}

// Array elements of a trace of `nchans` rows under the handle's segment count (nbls_set_segments; rows that do not
// divide into the segments: nbls_plan refuses them).  A geometry of another array size is stale.
static void set_elements(nbls_handle* h, int32_t nchans) {
    const int E = h->nseg > 1 && nchans % h->nseg == 0 ? nchans / h->nseg : nchans;
    nbls_estimator& x = h->est[0];
    if (h->nelem != E && x.d_xij) {
        x.d_xij.release();
        h->npairs = x.npairs = 0;
    }
    h->nelem = E;
}

// Declare the trace: allocation and shape, no samples yet (h->trace_loaded = false).
static int trace_shape_impl(nbls_handle* h, int32_t nchans, int64_t npts, double fs) {
    HIPCHK(h, hipSetDevice(h->device));
    const int64_t pad = (npts + 63) / 64 * 64;
    const size_t need = (size_t)nchans * pad * sizeof(double);
    if (int rc = grown(h, h->d_trace.grow(need), "hipMalloc((void**)&h->d_trace, need)")) return rc;
    set_elements(h, nchans);
    h->nchans = nchans;
    h->npts = npts;
    h->npts_pad = pad;
    h->fs = fs;
    h->planned = false;
    h->trace_loaded = false;
    h->rows_landed.store(0, std::memory_order_release);
    h->upload_state.store(2, std::memory_order_release);
    return NBLS_OK;
}

// Copy the samples of a declared trace, row by row on the handle's upload stream, an event behind every row (a pass
// queued meanwhile on another thread filters the rows as they land, see wait_rows).  Touches only d_trace, the upload
// stream and (on failure) the error text: nbls_upload_rows may therefore run beside nbls_set_geometry / nbls_plan /
// nbls_execute of the same handle on another thread.
static int trace_copy_impl(nbls_handle* h, const double* const* rows, const double* flat) {
    struct Guard {
        nbls_handle* h; bool ok = false;
        ~Guard() { h->upload_state.store(ok ? 0 : -1, std::memory_order_release); }
    } guard{h};
    h->rows_landed.store(0, std::memory_order_release);
    h->upload_state.store(1, std::memory_order_release);
    HIPCHK(h, hipSetDevice(h->device));
    const int32_t nchans = h->nchans;
    const int64_t npts = h->npts, pad = h->npts_pad;
    if (!h->ustream) HIPCHK(h, hipStreamCreateWithFlags(&h->ustream, hipStreamNonBlocking));
    if (!h->ev_uprev) HIPCHK(h, hipEventCreateWithFlags(&h->ev_uprev, hipEventDisableTiming));
    while ((int)h->uev.size() < nchans) {
        hipEvent_t e;
        HIPCHK(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        h->uev.push_back(e);
    }
    // behind whatever is still queued on the compute streams: an earlier pass may be reading the trace this one replaces
    for (hipStream_t s : {h->stream, h->stream2}) {
        if (!s) continue;
        HIPCHK(h, hipEventRecord(h->ev_uprev, s));
        HIPCHK(h, hipStreamWaitEvent(h->ustream, h->ev_uprev, 0));
    }
    if (pad > npts)
        HIPCHK(h, hipMemset2DAsync(h->d_trace + npts, pad * sizeof(double), 0, (pad - npts) * sizeof(double), nchans, h->ustream));
    if (flat) {
        HIPCHK(h, hipMemcpy2DAsync(h->d_trace, pad * sizeof(double), flat, npts * sizeof(double),
                                   npts * sizeof(double), nchans, hipMemcpyHostToDevice, h->ustream));
        for (int c = 0; c < nchans; ++c) HIPCHK(h, hipEventRecord(h->uev[c], h->ustream));
        h->rows_landed.store(nchans, std::memory_order_release);
    } else {
        for (int c = 0; c < nchans; ++c) {
            HIPCHK(h, hipMemcpyAsync(h->d_trace + (size_t)c * pad, rows[c], npts * sizeof(double), hipMemcpyHostToDevice, h->ustream));
            HIPCHK(h, hipEventRecord(h->uev[c], h->ustream));
            h->rows_landed.store(c + 1, std::memory_order_release);
        }
    }
    // the caller's buffers may be reused as soon as this returns (pageable sources are staged before
    // hipMemcpyAsync returns; pinned ones are still being read): wait for the copies
    HIPCHK(h, hipStreamSynchronize(h->ustream));
    h->trace_loaded = true;
    guard.ok = true;
    return NBLS_OK;
}

// Host side of the row pipeline: wait until more than `done` channels of the trace are in flight behind their events
// (-> how many), the upload has failed (-> -1), nothing arrives (-> -2) or the shape was declared but no upload announced
// (nbls_expect_upload) or started (-> -3).  With no upload under way every channel is there.
static int wait_rows(nbls_handle* h, int done) {
    const auto t0 = std::chrono::steady_clock::now();
    for (long spin = 0;; ++spin) {
        const int st = h->upload_state.load(std::memory_order_acquire);
        const int landed = h->rows_landed.load(std::memory_order_acquire);
        if (st < 0) return -1;
        if (st == 0) return h->trace_loaded ? h->nchans : -1;
        if (st == 2) return -3;                  // declared, and nobody has announced the samples
        if (landed > done) return landed;
        if ((spin & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(120)) return -2;
        std::this_thread::yield();
    }
}

static int set_trace_impl(nbls_handle* h, const double* const* rows, const double* flat, int32_t nchans, int64_t npts,
                          double fs) {
    const int rc = trace_shape_impl(h, nchans, npts, fs);
    return rc ? rc : trace_copy_impl(h, rows, flat);
}

int nbls_set_trace_shape(nbls_handle* h, int32_t nchans, int64_t npts, double fs) {
    if (!h) return NBLS_ERR_ARG;
    if (nchans < 1 || npts < 1 || !(fs > 0.0)) return fail(h, NBLS_ERR_ARG, "nbls_set_trace_shape: bad argument");
    return trace_shape_impl(h, nchans, npts, fs);
}

int nbls_upload_rows(nbls_handle* h, const double* const* rows, int32_t nchans, int64_t npts) {
    if (!h) return NBLS_ERR_ARG;
    if (!rows || nchans != h->nchans || npts != h->npts || !h->d_trace)
        return fail(h, NBLS_ERR_ARG, "nbls_upload_rows: rows do not match the shape declared with nbls_set_trace_shape");
    for (int c = 0; c < nchans; ++c)
        if (!rows[c]) return fail(h, NBLS_ERR_ARG, "nbls_upload_rows: null row");
    return trace_copy_impl(h, rows, nullptr);
}

int nbls_expect_upload(nbls_handle* h) {
    if (!h) return NBLS_ERR_ARG;
    int declared = 2;
    if (!h->upload_state.compare_exchange_strong(declared, 3, std::memory_order_acq_rel))
        return fail(h, NBLS_ERR_STATE, "nbls_expect_upload: no trace shape declared (nbls_set_trace_shape) or its samples are there already");
    return NBLS_OK;
}

int nbls_abort_upload(nbls_handle* h) {
    if (!h) return NBLS_ERR_ARG;
    int st = h->upload_state.load(std::memory_order_acquire);
    while ((st == 2 || st == 3) && !h->upload_state.compare_exchange_weak(st, -1, std::memory_order_acq_rel)) {}
    return NBLS_OK;
}

int nbls_set_trace(nbls_handle* h, const double* trace, int32_t nchans, int64_t npts, double fs) {
    if (!h) return NBLS_ERR_ARG;
    if (!trace || nchans < 1 || npts < 1 || !(fs > 0.0)) return fail(h, NBLS_ERR_ARG, "nbls_set_trace: bad argument");
    return set_trace_impl(h, nullptr, trace, nchans, npts, fs);
}

int nbls_set_trace_from(nbls_handle* h, const nbls_handle* src) {
    if (!h || !src) return NBLS_ERR_ARG;
    if (!src->d_trace) return fail(h, NBLS_ERR_STATE, "nbls_set_trace_from: the source handle has no trace");
    if (h == src) return NBLS_OK;
    if (h->device != src->device) return fail(h, NBLS_ERR_ARG, "nbls_set_trace_from: handles are on different devices");
    HIPCHK(h, hipSetDevice(h->device));
    const size_t need = (size_t)src->nchans * src->npts_pad * sizeof(double);
    if (int rc = grown(h, h->d_trace.grow(need), "hipMalloc((void**)&h->d_trace, need)")) return rc;
    // the source's upload has completed (nbls_set_trace* return after it) or is still running on another thread
    // (nbls_upload_rows): wait for its last row; the copy is ordered on THIS handle's stream
    {
        nbls_handle* s_ = const_cast<nbls_handle*>(src);
        int landed = 0;
        while (landed >= 0 && landed < src->nchans) landed = wait_rows(s_, landed);
        if (landed < 0) return fail(h, NBLS_ERR_STATE, "nbls_set_trace_from: the source handle's trace did not arrive");
        if (!src->uev.empty() && (int)src->uev.size() >= src->nchans) HIPCHK(h, hipStreamWaitEvent(h->stream, src->uev[src->nchans - 1], 0));
    }
    HIPCHK(h, hipMemcpyAsync(h->d_trace, src->d_trace, need, hipMemcpyDeviceToDevice, h->stream));
    set_elements(h, src->nchans);
    h->nchans = src->nchans;
    h->npts = src->npts;
    h->npts_pad = src->npts_pad;
    h->fs = src->fs;
    h->planned = false;
    h->trace_loaded = true;               // (ordered on this handle's stream before its next pass)
    h->rows_landed.store(h->nchans, std::memory_order_release);
    h->upload_state.store(0, std::memory_order_release);
    return NBLS_OK;
}

int nbls_set_trace_rows(nbls_handle* h, const double* const* rows, int32_t nchans, int64_t npts, double fs) {
    if (!h) return NBLS_ERR_ARG;
    if (!rows || nchans < 1 || npts < 1 || !(fs > 0.0)) return fail(h, NBLS_ERR_ARG, "nbls_set_trace_rows: bad argument");
    for (int c = 0; c < nchans; ++c)
        if (!rows[c]) return fail(h, NBLS_ERR_ARG, "nbls_set_trace_rows: NULL row pointer");
    return set_trace_impl(h, rows, nullptr, nchans, npts, fs);
}

int nbls_set_geometry(nbls_handle* h, const double* xij, const int32_t* pair_idx, const double* xpinv,
                      int32_t npairs) {
    if (!h) return NBLS_ERR_ARG;
    if (!xij || !pair_idx || !xpinv) return fail(h, NBLS_ERR_ARG, "nbls_set_geometry: NULL pointer");
    if (npairs < 3) return fail(h, NBLS_ERR_GEOMETRY, "need at least 3 array elements (3 pairs)");
    if (npairs > NBLS_MAX_PAIRS) return fail(h, NBLS_ERR_UNSUPPORTED, "more than 512 pairs (32 elements) not supported");
    if (!coarray_full_rank(xij, npairs)) return fail(h, NBLS_ERR_GEOMETRY, "co-array is rank deficient (collinear array)");
    // the same geometry as the handle already holds (every band group of every call of one array): nothing to upload
    nbls_estimator& x = h->est[0];
    const size_t n2 = (size_t)npairs * 2;
    if (x.d_xij && h->d_pair && x.d_xpinv && h->npairs == npairs && x.h_xij.size() == n2 && h->h_pair.size() == n2 &&
        x.h_xpinv.size() == n2 && memcmp(x.h_xij.data(), xij, n2 * sizeof(double)) == 0 &&
        memcmp(h->h_pair.data(), pair_idx, n2 * sizeof(int32_t)) == 0 && memcmp(x.h_xpinv.data(), xpinv, n2 * sizeof(double)) == 0) {
        h->planned = false;
        return NBLS_OK;
    }
    HIPCHK(h, hipSetDevice(h->device));
    StreamGuard guard(h);
    int rc;
    x.h_xij.clear();                         // (a failed upload leaves no stale "already there" record)
    if ((rc = alloc_copy(h, x.d_xij, xij, n2))) return rc;
    if ((rc = alloc_copy(h, h->d_pair, pair_idx, n2))) return rc;
    if ((rc = alloc_copy(h, x.d_xpinv, xpinv, n2))) return rc;
    x.h_xij.assign(xij, xij + n2);
    h->h_pair.assign(pair_idx, pair_idx + n2);
    x.h_xpinv.assign(xpinv, xpinv + n2);
    h->npairs = x.npairs = npairs;
    h->planned = false;
    return NBLS_OK;
}

int nbls_set_segments(nbls_handle* h, int32_t nseg) {
    if (!h) return NBLS_ERR_ARG;
    if (nseg < 1) return fail(h, NBLS_ERR_ARG, "nbls_set_segments: nseg must be at least 1");
    h->nseg = nseg;
    if (h->d_trace) set_elements(h, h->nchans);
    h->planned = false;                      // (consumed by the next nbls_plan)
    return NBLS_OK;
}

int nbls_set_window_ranges(nbls_handle* h, int32_t nbands, const int32_t* first, const int32_t* count) {
    if (!h) return NBLS_ERR_ARG;
    // consumed by the NEXT nbls_plan; an existing plan keeps the ranges it was made with
    if (nbands <= 0 || !first || !count) {       // reset: every band processes all its windows
        h->win_first.clear();
        h->win_count.clear();
        return NBLS_OK;
    }
    for (int b = 0; b < nbands; ++b)
        if (first[b] < 0) return fail(h, NBLS_ERR_ARG, "nbls_set_window_ranges: negative first window");
    h->win_first.assign(first, first + nbands);
    h->win_count.assign(count, count + nbands);
    return NBLS_OK;
}

int nbls_set_estimators(nbls_handle* h, int32_t n, const nbls_estimator_desc* desc) {
    if (!h) return NBLS_ERR_ARG;
    if (n <= 0) {                                // reset: the next plan is the plain pass (the buffers stay for a later use)
        h->nest = 0;
        h->planned = false;
        return NBLS_OK;
    }
    // everything is checked, and the new estimators are built beside the handle's, before the handle changes
    if (!desc) return fail(h, NBLS_ERR_ARG, "nbls_set_estimators: NULL pointer");
    if (n > NBLS_MAX_ESTIMATORS) return fail(h, NBLS_ERR_UNSUPPORTED, "nbls_set_estimators: at most 8 further estimators");
    if (h->nseg > 1) return fail(h, NBLS_ERR_UNSUPPORTED, "nbls_set_estimators: not supported with several segments (nbls_set_segments)");
    if (!h->win_first.empty()) return fail(h, NBLS_ERR_UNSUPPORTED, "nbls_set_estimators: not supported with window ranges (nbls_set_window_ranges)");
    if (h->comm) return fail(h, NBLS_ERR_UNSUPPORTED, "nbls_set_estimators: not supported with an RCCL communicator (nbls_comm_*)");
    if (!h->d_trace) return fail(h, NBLS_ERR_STATE, "nbls_set_estimators: no trace set (the element count is not known)");
    const int E = h->nelem;
    struct Built { std::vector<int32_t> kept, kept_pair, starts; std::vector<double> xij, xpinv, rew; };
    std::vector<Built> built((size_t)n);
    for (int e = 0; e < n; ++e) {
        const nbls_estimator_desc& d = desc[e];
        const std::string who = "nbls_set_estimators: estimator " + std::to_string(e + 1) + ": ";
        if (!d.kept || !d.xij || !d.pair_idx || !d.xpinv) return fail(h, NBLS_ERR_ARG, who + "NULL pointer");
        if (d.nkept < 0 || d.nkept > E) return fail(h, NBLS_ERR_ARG, who + "more kept elements than the trace has");
        for (int i = 0; i < d.nkept; ++i) {
            if (d.kept[i] < 0 || d.kept[i] >= E) return fail(h, NBLS_ERR_ARG, who + "element index out of range");
            if (i > 0 && d.kept[i] <= d.kept[i - 1]) return fail(h, NBLS_ERR_ARG, who + "element indices must ascend without repeats");
        }
        if (d.nkept < 3) return fail(h, NBLS_ERR_GEOMETRY, who + "need at least 3 array elements");
        if (d.lts && d.nkept < 4) return fail(h, NBLS_ERR_GEOMETRY, who + "LTS needs at least 4 array elements");
        const int K = d.nkept, P = K * (K - 1) / 2;
        for (int i = 0, k = 0; i < K - 1; ++i)
            for (int j = i + 1; j < K; ++j, ++k)
                if (d.pair_idx[2 * k] != i || d.pair_idx[2 * k + 1] != j)
                    return fail(h, NBLS_ERR_ARG, who + "pair_idx is not the lexicographic pair list of the kept elements");
        if (!coarray_full_rank(d.xij, P)) return fail(h, NBLS_ERR_GEOMETRY, who + "co-array is rank deficient (collinear array)");
        if (d.lts) { const int rc = check_lts(h, d.lts, P, who); if (rc) return rc; }
        if (d.eig6 && (!(d.eig6[0] > 0.0) || !(d.eig6[1] > 0.0))) return fail(h, NBLS_ERR_ARG, who + "the eigenvalues of X^T X must be positive");
        Built& b = built[(size_t)e];
        b.kept.assign(d.kept, d.kept + K);
        if (K < E) {                             // pair (i, j) of the sub-array = pair (kept[i], kept[j]) of the full one
            for (int i = 0; i < K - 1; ++i)
                for (int j = i + 1; j < K; ++j) {
                    const int a = d.kept[i], c = d.kept[j];
                    b.kept_pair.push_back(a * (2 * E - a - 1) / 2 + (c - a - 1));
                }
        }
        b.xij.assign(d.xij, d.xij + 2 * (size_t)P);
        b.xpinv.assign(d.xpinv, d.xpinv + 2 * (size_t)P);
        if (d.lts) {
            b.starts.assign(d.lts->starts, d.lts->starts + (size_t)d.lts->nstarts * 4);
            b.rew.assign(d.lts->rew_table, d.lts->rew_table + (size_t)P + 1);
        }
    }
    for (int e = 0; e < n; ++e) {                // est[0] is the plan's own: not touched here
        nbls_estimator& x = h->est[1 + e];
        Built& b = built[(size_t)e];
        x.kept.swap(b.kept); x.kept_pair.swap(b.kept_pair);
        x.h_xij.swap(b.xij); x.h_xpinv.swap(b.xpinv); x.h_starts.swap(b.starts); x.h_rew.swap(b.rew);
        x.npairs = (int)(x.h_xij.size() / 2);
        x.lts = desc[e].lts != nullptr;
        x.ltsp = nbls_lts_params{};
        if (x.lts) { x.ltsp = *desc[e].lts; x.ltsp.starts = nullptr; x.ltsp.rew_table = nullptr; }
        x.want_unc = desc[e].eig6 != nullptr;
        for (int i = 0; i < 6; ++i) x.unc_par[i] = x.want_unc ? desc[e].eig6[i] : 0.0;
    }
    h->nest = n;
    h->planned = false;
    return NBLS_OK;
}

// nbls_plan's arguments and what its argument checks derive from them, handed from step to step.
struct plan_args {
    int32_t nbands;
    const double* sos;
    int32_t nsections, zero_phase;
    const double *taper_left, *taper_right;
    int32_t taper_len;
    const int32_t *winlen, *wininc;
    int32_t vector_len;
    const nbls_lts_params* lts;
    int32_t xcorr_impl;
    int NS, E, P, R, D;            // segments, elements, pairs (1 without geometry), result rows, filter state size
};

// Step 1: the arguments against the handle's trace, geometry and estimators; records the LTS plan of est[0].
static int plan_check_args(nbls_handle* h, plan_args& a) {
    if (!h->d_trace) return fail(h, NBLS_ERR_STATE, "nbls_plan: no trace set");
    if (a.nbands < 1 || (!a.sos && a.nsections != 0) || !a.winlen || !a.wininc || a.vector_len < 1)
        return fail(h, NBLS_ERR_ARG, "nbls_plan: bad argument");
    if (a.nsections < 0 || a.nsections > NBLS_MAX_SECTIONS)
        return fail(h, NBLS_ERR_UNSUPPORTED, "nbls_plan: 0..8 second-order sections supported");
    if (a.taper_len < 0 || 2 * (int64_t)a.taper_len > h->npts || (a.taper_len > 0 && (!a.taper_left || !a.taper_right)))
        return fail(h, NBLS_ERR_ARG, "nbls_plan: bad taper");
    // several recordings of one array (nbls_set_segments): nseg blocks of E rows, result row r = b * nseg + s
    const int NS = h->nseg;
    if (NS > 1) {
        if (h->nchans % NS != 0)
            return fail(h, NBLS_ERR_ARG, "nbls_plan: " + std::to_string(h->nchans) + " trace rows do not divide into " + std::to_string(NS) + " segments");
        if (!h->win_first.empty())
            return fail(h, NBLS_ERR_UNSUPPORTED, "nbls_plan: window ranges (nbls_set_window_ranges) are not supported with several segments");
        if (h->comm)
            return fail(h, NBLS_ERR_UNSUPPORTED, "nbls_plan: the RCCL gather (nbls_comm_*) is not supported with several segments");
    }
    if (h->nest > 0 && (NS > 1 || !h->win_first.empty() || h->comm))
        return fail(h, NBLS_ERR_UNSUPPORTED, "nbls_plan: further estimators (nbls_set_estimators) are not supported with several segments, window ranges or the RCCL gather");
    const nbls_requests& w = h->want;
    // what several requests need of the geometry (nbls_set_geometry): that it is the one of the trace's array of En elements,
    // and of its pair list every pair in lexicographic order, or the pairs (0, m) in its first rows
    const int En = h->nchans / NS;
    const bool own_geometry = h->est[0].d_xij && (int64_t)En * (En - 1) / 2 == h->npairs;
    const bool pair_list = own_geometry && h->h_pair.size() == 2 * (size_t)h->npairs;
    const auto lexicographic = [&] {
        for (int i = 0, k = 0; pair_list && i < En; ++i)
            for (int j = i + 1; j < En; ++j, ++k)
                if (h->h_pair[2 * k] != i || h->h_pair[2 * k + 1] != j) return false;
        return pair_list;
    };
    const auto first_rows_from_0 = [&] {
        for (int m = 1; pair_list && m < En; ++m)
            if (h->h_pair[2 * (m - 1)] != 0 || h->h_pair[2 * (m - 1) + 1] != m) return false;
        return pair_list;
    };
    if (w.beam && h->comm)
        return fail(h, NBLS_ERR_UNSUPPORTED, "nbls_plan: beam results (nbls_set_beam) are not supported with an RCCL communicator (the gathered block does not carry them)");
    if (w.closure) {                 // closure of the picked lags (nbls_set_closure): every pair of the trace's array, in list order
        if (h->comm)
            return fail(h, NBLS_ERR_UNSUPPORTED, "nbls_plan: closure results (nbls_set_closure) are not supported with an RCCL communicator (the gathered block does not carry them)");
        if (!lexicographic())
            return fail(h, NBLS_ERR_STATE, "nbls_plan: closure results (nbls_set_closure) need the geometry of the trace's array, every pair in lexicographic order");
    }
    std::vector<int32_t> gdel;       // the slowness grid (nbls_set_beam_grid): its delay table for this trace's array
    std::vector<double> gcoef;       // ... and, steered at fractional delays (nbls_set_beam_interpolation), its coefficient table
    int ghalo = 0;
    if (w.steer_taps && !w.beam && w.grid.empty())
        return fail(h, NBLS_ERR_STATE, "nbls_plan: fractional-sample steering (nbls_set_beam_interpolation) needs beam results (nbls_set_beam) or a slowness grid (nbls_set_beam_grid)");
    if (!w.grid.empty()) {
        if (h->comm)
            return fail(h, NBLS_ERR_UNSUPPORTED, "nbls_plan: the slowness-grid search (nbls_set_beam_grid) is not supported with an RCCL communicator (the gathered block does not carry its grids)");
        if (!own_geometry)
            return fail(h, NBLS_ERR_STATE, "nbls_plan: the slowness-grid search (nbls_set_beam_grid) needs the geometry of the trace's array");
        const int G = (int)(w.grid.size() / 2);
        gdel.resize((size_t)G * En);
        bool made;
        if (w.steer_taps) {          // floor(tau) and the Lagrange coefficients instead of rint(tau)
            gcoef.resize((size_t)G * En * w.steer_taps);
            made = nbls_beam_grid_steer_of(h->est[0].h_xij.data(), En, h->fs, w.grid.data(), G, w.steer_taps, gdel.data(), gcoef.data(), &ghalo);
        } else {
            made = nbls_beam_grid_delays_of(h->est[0].h_xij.data(), En, h->fs, w.grid.data(), G, gdel.data(), &ghalo);
        }
        if (!made)
            return fail(h, NBLS_ERR_ARG, "nbls_plan: a delay of the slowness grid (nbls_set_beam_grid) reaches 2^30 samples");
    }
    int64_t rhalo = 0;               // the refinement of the grid maximum (nbls_set_beam_grid_refinement): its halo H_r
    if (w.grid_refined()) {
        if (w.grid.empty() || !w.steer_taps)
            return fail(h, NBLS_ERR_STATE, "nbls_plan: the refinement of the grid maximum (nbls_set_beam_grid_refinement) needs a slowness grid (nbls_set_beam_grid) steered at fractional-sample delays (nbls_set_beam_interpolation): whole-sample F is piecewise constant");
        if (!w.seed.empty())
            return fail(h, NBLS_ERR_UNSUPPORTED, "nbls_plan: the refinement of the grid maximum (nbls_set_beam_grid_refinement) is not supported with a lag seed (nbls_set_lag_seed): the seed keeps the unrefined maximum");
        rhalo = nbls_beam_grid_refine_halo_of(h->est[0].h_xij.data(), En, h->fs, ghalo, w.grid_refine.step);
        if (rhalo < 0)
            return fail(h, NBLS_ERR_ARG, "nbls_plan: the delay bound of the refined grid maximum (nbls_set_beam_grid_refinement) reaches 2^30 samples");
    }
    if (!w.capon.grid.empty()) {     // Capon spectra (nbls_set_capon): the tables are made once the windows are known (plan_estimators)
        const nbls_requests::capon_request& c = w.capon;
        if (h->comm)
            return fail(h, NBLS_ERR_UNSUPPORTED, "nbls_plan: Capon spectra (nbls_set_capon) are not supported with an RCCL communicator (the gathered block does not carry them)");
        if (!own_geometry)
            return fail(h, NBLS_ERR_STATE, "nbls_plan: Capon spectra (nbls_set_capon) need the geometry of the trace's array");
        if (En > NBLS_CAPON_MAX_ELEMENTS)
            return fail(h, NBLS_ERR_UNSUPPORTED, "nbls_plan: Capon spectra (nbls_set_capon) support up to " + std::to_string(NBLS_CAPON_MAX_ELEMENTS) + " elements");
        if ((int)c.freq.size() != a.nbands)
            return fail(h, NBLS_ERR_ARG, "nbls_plan: Capon tables (nbls_set_capon) of " + std::to_string(c.freq.size()) + " bands for a plan of " +
                                             std::to_string(a.nbands) + " bands");
        for (int b = 0; b < a.nbands; ++b) {
            if (c.ls[b] > a.winlen[b])
                return fail(h, NBLS_ERR_ARG, "nbls_plan: the Capon snapshot of band " + std::to_string(b) + " (" + std::to_string(c.ls[b]) +
                                                 " samples) is longer than its window (" + std::to_string(a.winlen[b]) + ")");
            if (c.loading == 0.0 && 1 + (a.winlen[b] - c.ls[b]) / c.hs[b] < En)
                return fail(h, NBLS_ERR_ARG, "nbls_plan: band " + std::to_string(b) + " has fewer Capon snapshots than elements and no loading: its matrix is singular by construction");
        }
        if ((size_t)a.nbands * (c.grid.size() / 2) * (size_t)En * 16 > ((size_t)1 << 30))
            return fail(h, NBLS_ERR_UNSUPPORTED, "nbls_plan: the Capon steering table (nbands * G * N * 16 bytes) exceeds 1 GiB");
    }
    if (w.clean.iterations > 0 && w.capon.grid.empty())      // the CLEAN-SC request (nbls_set_capon_clean) works on the spectra's R and tables
        return fail(h, NBLS_ERR_STATE, "nbls_plan: a CLEAN request (nbls_set_capon_clean) needs Capon spectra (nbls_set_capon)");
    if (w.music.sources >= 0) {      // the MUSIC request (nbls_set_capon_music): the spectra's R and tables, the full array, estimator 0 alone
        if (w.capon.grid.empty())
            return fail(h, NBLS_ERR_STATE, "nbls_plan: a MUSIC request (nbls_set_capon_music) needs Capon spectra (nbls_set_capon)");
        if (h->nest > 0)
            return fail(h, NBLS_ERR_UNSUPPORTED, "nbls_plan: a MUSIC request (nbls_set_capon_music) is not supported with further estimators (nbls_set_estimators)");
        if (w.kept_capon())
            return fail(h, NBLS_ERR_UNSUPPORTED, "nbls_plan: a MUSIC request (nbls_set_capon_music) is not supported with NBLS_KEPT_CAPON (nbls_set_kept_elements): it works on the full array");
        if (En < 3)
            return fail(h, NBLS_ERR_UNSUPPORTED, "nbls_plan: a MUSIC request (nbls_set_capon_music) needs at least 3 elements");
        if (w.music.sources > En - 1)
            return fail(h, NBLS_ERR_ARG, "nbls_plan: " + std::to_string(w.music.sources) + " sources (nbls_set_capon_music) for an array of " +
                                             std::to_string(En) + " elements (1.." + std::to_string(En - 1) + ")");
        if ((w.music.flags & NBLS_MUSIC_PEAKS) && w.peaks.nbr.empty())
            return fail(h, NBLS_ERR_STATE, "nbls_plan: NBLS_MUSIC_PEAKS (nbls_set_capon_music) needs K and the cells of a peak request (nbls_set_capon_peaks)");
    }
    int peak_route = 0;              // the peaks of the spectra (nbls_set_capon_peaks): Capon spectra of the same G, and a route
    if (!w.peaks.nbr.empty()) {
        const size_t G = w.capon.grid.size() / 2;
        if (!G)
            return fail(h, NBLS_ERR_ARG, "nbls_plan: a peak request (nbls_set_capon_peaks) needs Capon spectra (nbls_set_capon)");
        if (w.peaks.nbr.size() != 8 * G)
            return fail(h, NBLS_ERR_ARG, "nbls_plan: the peak request (nbls_set_capon_peaks) has " + std::to_string(w.peaks.nbr.size() / 8) +
                                             " cells for Capon spectra of " + std::to_string(G) + " points");
        // the unit's two maps wait in LDS or in HBM (capon.hip: nbls_capon_peak_route_of has the automatic choice)
        const bool fits = nbls_capon_peak_lds_bytes_of(En, (int)G) != 0;
        peak_route = h->opt.capon_peak_route ? h->opt.capon_peak_route : nbls_capon_peak_route_of(En, (int)G);
        if (peak_route == 1 && !fits)
            return fail(h, NBLS_ERR_UNSUPPORTED, "nbls_plan: option capon_peak_route 1: the two maps of " + std::to_string(G) + " points do not fit the LDS of a workgroup beside the kernel's " +
                                                     std::to_string(nbls_capon_lds_bytes_of(En)) + " bytes");
    }
    if (w.kept_q > 0) {              // the elements LTS kept (nbls_set_kept_elements): the full pair list, estimator 0 alone
        if (h->nest > 0)
            return fail(h, NBLS_ERR_UNSUPPORTED, "nbls_plan: the kept elements (nbls_set_kept_elements) are not supported with further estimators (nbls_set_estimators)");
        if (h->comm)
            return fail(h, NBLS_ERR_UNSUPPORTED, "nbls_plan: the kept elements (nbls_set_kept_elements) are not supported with an RCCL communicator (the gathered block does not carry them)");
        if (!lexicographic())
            return fail(h, NBLS_ERR_STATE, "nbls_plan: the kept elements (nbls_set_kept_elements) need the geometry of the trace's array, every pair in lexicographic order");
        if (En > 32 || w.kept_q > En - 1)
            return fail(h, NBLS_ERR_ARG, "nbls_plan: min_pairs (nbls_set_kept_elements) is " + std::to_string(w.kept_q) + " for an array of " +
                                             std::to_string(En) + " elements (1.." + std::to_string(En - 1) + ", at most 32 elements)");
        if ((w.kept_flags & NBLS_KEPT_BEAM) && !w.beam)
            return fail(h, NBLS_ERR_STATE, "nbls_plan: NBLS_KEPT_BEAM (nbls_set_kept_elements) needs beam results (nbls_set_beam)");
        if ((w.kept_flags & NBLS_KEPT_CAPON) && w.capon.grid.empty())
            return fail(h, NBLS_ERR_STATE, "nbls_plan: NBLS_KEPT_CAPON (nbls_set_kept_elements) needs Capon spectra (nbls_set_capon)");
    }
    if (w.bt) {                      // the beam trace (nbls_set_beam_trace): estimator 0, every window of every band, one synthesis window per band
        if (!h->win_first.empty())
            return fail(h, NBLS_ERR_UNSUPPORTED, "nbls_plan: the beam trace (nbls_set_beam_trace) is not supported with window ranges (nbls_set_window_ranges): a slice of the windows does not cover the trace");
        if (h->nest > 0)
            return fail(h, NBLS_ERR_UNSUPPORTED, "nbls_plan: the beam trace (nbls_set_beam_trace) is not supported with further estimators (nbls_set_estimators)");
        if (h->comm)
            return fail(h, NBLS_ERR_UNSUPPORTED, "nbls_plan: the beam trace (nbls_set_beam_trace) is not supported with an RCCL communicator (the gathered block does not carry it)");
        if (!first_rows_from_0())
            return fail(h, NBLS_ERR_STATE, "nbls_plan: the beam trace (nbls_set_beam_trace) needs the geometry of the trace's array, its first rows the pairs (0, m)");
        if ((w.bt_flags & NBLS_BEAM_TRACE_KEPT) && w.kept_q < 1)
            return fail(h, NBLS_ERR_STATE, "nbls_plan: NBLS_BEAM_TRACE_KEPT (nbls_set_beam_trace) needs the kept elements (nbls_set_kept_elements)");
        int64_t sumw = 0;
        for (int b = 0; b < a.nbands; ++b) sumw += a.winlen[b] > 0 ? a.winlen[b] : 0;
        if ((int64_t)w.bt_win.size() != sumw)
            return fail(h, NBLS_ERR_ARG, "nbls_plan: a synthesis window table (nbls_set_beam_trace) of " + std::to_string(w.bt_win.size()) +
                                             " entries for bands whose window lengths add up to " + std::to_string(sumw));
        int64_t o = 0;
        for (int b = 0; b < a.nbands; ++b) {
            bool any = false;
            for (int t = 0; t < a.winlen[b]; ++t) {
                const double g = w.bt_win[(size_t)(o + t)];
                if (!(g >= 0.0) || std::isinf(g))
                    return fail(h, NBLS_ERR_ARG, "nbls_plan: the synthesis window (nbls_set_beam_trace) of band " + std::to_string(b) + " has a negative or non-finite entry");
                any = any || g > 0.0;
            }
            if (!any)
                return fail(h, NBLS_ERR_ARG, "nbls_plan: the synthesis window (nbls_set_beam_trace) of band " + std::to_string(b) + " is all zero");
            o += a.winlen[b] > 0 ? a.winlen[b] : 0;
        }
    }
    if (w.fam) {                     // the families (nbls_set_families): estimator 0's rows, every window of every band
        if (!h->win_first.empty())
            return fail(h, NBLS_ERR_UNSUPPORTED, "nbls_plan: the families (nbls_set_families) are not supported with window ranges (nbls_set_window_ranges): a slice of the windows does not cover the lattice");
        if (h->nest > 0)
            return fail(h, NBLS_ERR_UNSUPPORTED, "nbls_plan: the families (nbls_set_families) are not supported with further estimators (nbls_set_estimators)");
        if (h->comm)
            return fail(h, NBLS_ERR_UNSUPPORTED, "nbls_plan: the families (nbls_set_families) are not supported with an RCCL communicator (the gathered block does not carry them)");
        if ((int64_t)a.nbands * NS * (int64_t)a.vector_len >= ((int64_t)1 << 31))
            return fail(h, NBLS_ERR_ARG, "nbls_plan: the families (nbls_set_families) take fewer than 2^31 cells");
    }
    size_t ed_lds = 0;
    if (w.ed) {                      // the element delays (nbls_set_element_delays): estimator 0, one max_shift per band
        if ((int)w.ed_K.size() != a.nbands)
            return fail(h, NBLS_ERR_ARG, "nbls_plan: " + std::to_string(w.ed_K.size()) + " shift ranges (nbls_set_element_delays) for a plan of " +
                                             std::to_string(a.nbands) + " bands");
        if (En > 32)
            return fail(h, NBLS_ERR_ARG, "nbls_plan: the element delays (nbls_set_element_delays) take at most 32 elements, not " + std::to_string(En));
        if (h->nest > 0)
            return fail(h, NBLS_ERR_UNSUPPORTED, "nbls_plan: the element delays (nbls_set_element_delays) are not supported with further estimators (nbls_set_estimators)");
        if (h->comm)
            return fail(h, NBLS_ERR_UNSUPPORTED, "nbls_plan: the element delays (nbls_set_element_delays) are not supported with an RCCL communicator (the gathered block does not carry them)");
        if (!first_rows_from_0())
            return fail(h, NBLS_ERR_STATE, "nbls_plan: the element delays (nbls_set_element_delays) need the geometry of the trace's array, its first rows the pairs (0, m)");
        if ((w.ed_flags & NBLS_ELEMENT_DELAY_KEPT) && w.kept_q < 1)
            return fail(h, NBLS_ERR_STATE, "nbls_plan: NBLS_ELEMENT_DELAY_KEPT (nbls_set_element_delays) needs the kept elements (nbls_set_kept_elements)");
        // the form: staged where the block of every band fits the LDS of a workgroup (element_delay.hip), else global
        bool fits = true;
        for (int b = 0; b < a.nbands; ++b) {
            const size_t lds = a.winlen[b] > 0 ? nbls_element_delay_lds_bytes_of(En, a.winlen[b], w.ed_K[(size_t)b]) : 0;
            if (!lds) fits = false;
            if (lds > ed_lds) ed_lds = lds;
        }
        if (h->opt.element_delay_form == 1 && !fits)
            return fail(h, NBLS_ERR_UNSUPPORTED, "nbls_plan: option element_delay_form 1: the rows of a band's windows do not fit the LDS of a workgroup");
        if (!fits || h->opt.element_delay_form == 2) ed_lds = 0;
    }
    if (!w.lim.empty()) {            // lag limits (nbls_set_lag_limits): one per pair of the geometry, the auto route only
        if (!h->est[0].d_xij || (int)w.lim.size() != h->npairs)
            return fail(h, NBLS_ERR_ARG, "nbls_plan: " + std::to_string(w.lim.size()) + " lag limits (nbls_set_lag_limits) for a geometry of " +
                                             std::to_string(h->est[0].d_xij ? h->npairs : 0) + " pairs");
        if (a.xcorr_impl != 0)
            return fail(h, NBLS_ERR_UNSUPPORTED, "nbls_plan: lag limits (nbls_set_lag_limits) need xcorr_impl 0: the forced correlators search every lag");
    }
    if (!w.seed.empty()) {           // the lag seed (nbls_set_lag_seed): one half-width per band, a plan with a slowness grid, the auto route only
        if ((int)w.seed.size() != a.nbands)
            return fail(h, NBLS_ERR_ARG, "nbls_plan: " + std::to_string(w.seed.size()) + " seed half-widths (nbls_set_lag_seed) for a plan of " +
                                             std::to_string(a.nbands) + " bands");
        if (w.grid.empty())
            return fail(h, NBLS_ERR_STATE, "nbls_plan: the lag seed (nbls_set_lag_seed) needs a slowness grid (nbls_set_beam_grid)");
        if (!w.lim.empty())
            return fail(h, NBLS_ERR_UNSUPPORTED, "nbls_plan: the lag seed (nbls_set_lag_seed) is not supported together with lag limits (nbls_set_lag_limits): the grid's extent bounds the slowness, one restriction at a time");
        if (a.xcorr_impl != 0)
            return fail(h, NBLS_ERR_UNSUPPORTED, "nbls_plan: the lag seed (nbls_set_lag_seed) needs xcorr_impl 0: the forced correlators search every lag");
    }
    const int E = En;
    nbls_estimator& x0 = h->est[0];
    for (int e = 1; e <= h->nest; ++e)
        if (!x0.d_xij || h->est[e].kept.empty() || h->est[e].kept.back() >= E || ((int)h->est[e].kept.size() == E) != h->est[e].kept_pair.empty())
            return fail(h, NBLS_ERR_ARG, "nbls_plan: the further estimators (nbls_set_estimators) do not fit this trace's elements and geometry");
    if (NS > 1 && (E < 3 || E > 32))
        return fail(h, NBLS_ERR_GEOMETRY, "nbls_plan: " + std::to_string(E) + " elements per segment (3..32 supported)");
    // geometry is optional for a filter-only plan (filter_data()); execute checks it
    const int P = x0.d_xij ? h->npairs : 1;
    if (x0.d_xij && (int64_t)E * (E - 1) / 2 != P)
        return fail(h, NBLS_ERR_ARG, "nbls_plan: geometry pair count does not match the array's element count");
    if (a.lts) {
        if (!x0.d_xij) return fail(h, NBLS_ERR_STATE, "nbls_plan: LTS needs the geometry");
        if (E < 4) return fail(h, NBLS_ERR_GEOMETRY, "LTS needs at least 4 array elements");
        const int rc = check_lts(h, a.lts, P, "nbls_plan: ");
        if (rc) return rc;
    }
    // nothing was refused: the handle takes the plan's requests (a refused plan has left `req` as it was) and what derives
    // from them; no pass of this plan has run yet
    h->req = w;
    if (w.capon.grid.empty()) {      // the CLEAN-SC and MUSIC requests belong to the spectra: a plan without them has neither
        h->req.clean = nbls_requests::capon_clean_request();
        h->req.music = nbls_requests::capon_music_request();
    }
    nbls_plan_derived& d = h->derived;
    d.grid_n = (int)(w.grid.size() / 2);
    d.grid_halo = ghalo;
    d.grid_delay.swap(gdel);
    d.grid_coef.swap(gcoef);
    d.grid_refine_halo = (int)rhalo;
    d.capon_n = (int)(w.capon.grid.size() / 2);
    d.peak_route = peak_route;
    // the slabs of the HBM route: what the option says, else as many as 256 MiB hold, 256 at least (which is 256 MiB at the
    // largest grid) and 4096 at most: a launch of 256 workgroups is one per CU
    d.peak_slabs = h->opt.capon_peak_slabs;
    if (peak_route && d.peak_slabs < 1) {
        const size_t fit = ((size_t)256 << 20) / (2 * (size_t)d.capon_n * sizeof(double));
        d.peak_slabs = (int)std::min<size_t>(4096, std::max<size_t>(256, fit));
    }
    d.ed_lds = ed_lds;
    h->solve_ran = h->xcorr_ran = false;
    h->nelem = E;
    if (a.lts) {
        x0.ltsp = *a.lts;
        x0.ltsp.starts = nullptr;
        x0.ltsp.rew_table = nullptr;
        x0.h_starts.assign(a.lts->starts, a.lts->starts + (size_t)a.lts->nstarts * 4);
        x0.h_rew.assign(a.lts->rew_table, a.lts->rew_table + (size_t)P + 1);
    }
    x0.lts = a.lts != nullptr;
    a.NS = NS; a.E = E; a.P = P;
    a.R = a.nbands * NS;
    a.D = 2 * a.nsections;
    return 0;
}

// Step 2: the filter tables, pure host arithmetic.  Every HIP call of the plan comes AFTER them — while the trace of a
// pipelined call is still going up on another thread (nbls_upload_rows) each HIP call waits for the runtime's lock
// behind a row copy (~0.15 ms apiece), and the first launch of the call waits for this plan.
static void plan_filter_tables(nbls_handle* h, const plan_args& a) {
    const int nbands = a.nbands, nsections = a.nsections, D = a.D;
    const int GG = NBLS_FILTER_GROUP;
    // (host tables kept in the handle between plans: a fresh 1.2 MB per plan is 300 page faults on the table threads, on the
    //  critical path of every call — and trimmed back to the OS when it is freed)
    h->hp_M.resize((size_t)nbands * (GG + 1) * D * D);
    h->hp_FW.resize((size_t)nbands * NBLS_FILTER_CHUNK * D);
    // long-double table arithmetic, 30-100 us per band: the bands are dealt to a few host threads (the
    // plan sits on the critical path of a call: the GPU has nothing to do until it is through)
    double* const fwp = h->hp_FW.data();
    double* const mp = h->hp_M.data();
    int nt = nsections > 0 ? std::max(1, std::min(12, nbands / 2)) : 0;     // 2+ bands per thread of the pool (TablePool)
    const std::function<void(int)> work = [&](int t) {
        for (int b = t; b < nbands; b += nt)
            filter_tables(a.sos + (size_t)b * nsections * 6, nsections, NBLS_FILTER_CHUNK, GG,
                          fwp + (size_t)b * NBLS_FILTER_CHUNK * D, mp + (size_t)b * (GG + 1) * D * D);
    };
    if (nt > 0 && !pool_run(nt, work)) {       // the pool is busy with another handle's plan: all bands here
        nt = 1;
        work(0);
    }
}

// Step 3: the windows of every result row (R = nbands * nseg, rows of one band consecutive; the filter tables stay per
// band) and the units they make, on the host.
static int plan_windows(nbls_handle* h, const plan_args& a) {
    const int R = a.R, NS = a.NS;
    h->W.resize(R);
    h->inc.resize(R);
    for (int r = 0; r < R; ++r) { h->W[r] = a.winlen[r / NS]; h->inc[r] = a.wininc[r / NS]; }
    h->nwin.resize(R);
    h->unit_off.resize(R + 1);
    h->woff.assign(R, 0);
    int64_t U = 0;
    int maxW = 0, uniW = a.nbands > 0 ? a.winlen[0] : 0;
    for (int b = 0; b < R; ++b) {
        const int W = h->W[b], inc = h->inc[b];
        if (W != uniW) uniW = 0;
        if (W < 2 || inc < 1)
            return fail(h, NBLS_ERR_ARG, "nbls_plan: window length must be at least 2 samples, the hop at least 1");
        // len(arange(0, npts - W, inc))
        const int64_t span = h->npts - W;
        int64_t n = span > 0 ? (span + inc - 1) / inc : 0;
        if (n > a.vector_len) return fail(h, NBLS_ERR_ARG, "nbls_plan: vector_len smaller than a band's window count");
        int64_t first = 0;
        if ((int)h->win_first.size() == R) {               // window sharding: this handle's slice of the band
            first = h->win_first[b] < n ? h->win_first[b] : n;
            int64_t cnt = h->win_count[b] < 0 ? n - first : h->win_count[b];
            if (cnt > n - first) cnt = n - first;
            n = cnt;
        }
        h->woff[b] = (int32_t)first;
        h->nwin[b] = (int32_t)n;
        h->unit_off[b] = (int32_t)U;
        U += n;
        if (W > maxW) maxW = W;
    }
    h->unit_off[R] = (int32_t)U;
    if (U > 0x7fffffffLL / (a.P > 0 ? a.P : 1)) return fail(h, NBLS_ERR_UNSUPPORTED, "nbls_plan: too many (unit, pair) items for one launch");
    h->nunits = U;
    h->maxW = maxW;
    h->uniW = uniW;
    h->fbands = a.nbands;
    h->nbands = R;
    h->nsections = a.nsections;
    h->zero_phase = a.zero_phase ? 1 : 0;
    h->taper_len = a.taper_len;
    h->vector_len = a.vector_len;
    h->xcorr_impl = a.xcorr_impl;
    h->nchunks = (h->npts + NBLS_FILTER_CHUNK - 1) / NBLS_FILTER_CHUNK;
    return 0;
}

// Step 4: the filter, taper, window and unit tables go to the device (places in the arena; the ramps apart).
static int plan_upload_tables(nbls_handle* h, const plan_args& a) {
    const int R = a.R;
    const int64_t U = h->nunits;
    int rc;
    if ((rc = alloc_copy(h, h->d_fw, h->hp_FW.data(), h->hp_FW.size()))) return rc;
    if ((rc = alloc_copy(h, h->d_sos, a.sos, (size_t)a.nbands * a.nsections * 6))) return rc;
    if (a.nsections == 0 && a.nbands != 1)
        return fail(h, NBLS_ERR_ARG, "nbls_plan: an unfiltered plan has exactly one band");
    if ((rc = alloc_copy(h, h->d_M, h->hp_M.data(), h->hp_M.size()))) return rc;
    {   // the ramps (1 % of the trace each: 0.14 MB at cfg-3, a quarter of a plan's upload) only when they differ from what is there
        const size_t tn = (size_t)a.taper_len;
        const bool same = h->d_tl && h->d_tr && h->h_tl.size() == tn && h->h_tr.size() == tn &&
                          (tn == 0 || (memcmp(h->h_tl.data(), a.taper_left, tn * sizeof(double)) == 0 &&
                                       memcmp(h->h_tr.data(), a.taper_right, tn * sizeof(double)) == 0));
        if (!same) {
            h->h_tl.clear();
            h->h_tr.clear();
            h->arena_mode = false;                       // allocations of their own: they outlive the plan
            rc = alloc_copy(h, h->d_tl, a.taper_left, tn);
            if (!rc) rc = alloc_copy(h, h->d_tr, a.taper_right, tn);
            h->arena_mode = true;
            if (rc) return rc;
            if (tn) { h->h_tl.assign(a.taper_left, a.taper_left + tn); h->h_tr.assign(a.taper_right, a.taper_right + tn); }
        }
    }
    if ((rc = alloc_copy(h, h->d_W, h->W.data(), (size_t)R))) return rc;
    if ((rc = alloc_copy(h, h->d_inc, h->inc.data(), (size_t)R))) return rc;
    if ((rc = alloc_copy(h, h->d_nwin, h->nwin.data(), (size_t)R))) return rc;
    if ((rc = alloc_copy(h, h->d_unit_off, h->unit_off.data(), (size_t)R + 1))) return rc;
    if ((rc = alloc_copy(h, h->d_win_off, h->woff.data(), (size_t)R))) return rc;
    std::vector<int32_t>& ub = h->hp_ub;
    ub.resize((size_t)U);
    for (int b = 0; b < R; ++b)
        for (int64_t u = h->unit_off[b]; u < h->unit_off[b + 1]; ++u) ub[(size_t)u] = b;
    if ((rc = alloc_copy(h, h->d_unit_band, ub.data(), (size_t)U))) return rc;
    std::vector<int32_t>& uw = h->hp_uw;
    uw.resize((size_t)(U > 0 ? U : 1));
    for (int b = 0; b < R; ++b)
        for (int64_t u = h->unit_off[b]; u < h->unit_off[b + 1]; ++u) uw[(size_t)u] = (int32_t)(u - h->unit_off[b]) + h->woff[b];
    return alloc_copy(h, h->d_unit_win, uw.data(), (size_t)U);
}

// Step 5: the work buffers of the filter, and the pass's lag / cmax rows with the result buffers of est[0].
static int plan_work_buffers(nbls_handle* h, const plan_args& a) {
    const int D = a.D, nsections = a.nsections;
    int rc;
    const size_t nseries = (size_t)a.nbands * h->nchans;      // (= R * E)
    // + 64 bytes: the verifier's 16-byte copies of a window that starts on an odd sample read one sample past its end
    if ((rc = ensure(h, h->d_filt, nseries * h->npts_pad * sizeof(double) + 64))) return rc;
    if ((rc = ensure(h, h->d_cstate, nseries * h->nchunks * D * sizeof(double)))) return rc;
    if ((rc = ensure(h, h->d_cstate2, nseries * h->nchunks * D * sizeof(double)))) return rc;
    if (!(h->zero_phase && nsections > 0 && nsections <= 4)) {
        h->d_tstate.release();               // this plan filters in the stored form
    } else {
        // tile-boundary states of the recompute form (2S doubles per 16 samples: a quarter of the filtered buffer at
        // two sections; beyond four sections they would be as large as the samples they replace, and the stored form
        // is used).  Without room for them the filter writes and re-reads the forward output instead: same results.
        const size_t need = nseries * h->nchunks * (NBLS_FILTER_CHUNK / NBLS_FILTER_TILE) * D * sizeof(double);
        if (h->d_tstate.grow(need) != hipSuccess) (void)hipGetLastError();
    }
    const size_t ngroups = (size_t)((h->nchunks + NBLS_FILTER_GROUP - 1) / NBLS_FILTER_GROUP);
    if ((rc = ensure(h, h->d_gend, nseries * ngroups * D * sizeof(double)))) return rc;
    if ((rc = ensure(h, h->d_gin, nseries * ngroups * D * sizeof(double)))) return rc;
    return size_result_buffers(h, h->est[0], (size_t)a.R * a.vector_len, h->reserve_res);
}

// Step 6: window groups (consecutive bands of one window length) and, per group, whether the int8 screening correlator
// applies; "auto" = screening wherever it applies, the faster general correlator elsewhere.
static int plan_window_groups(nbls_handle* h, const plan_args& a) {
    const int R = a.R;
    int xcorr_impl = a.xcorr_impl;
    h->wgroups.clear();
    int maxWP = 0;
    bool all_ok = true, any_ok = false;
    const int32_t min_lim = h->req.lim.empty() ? 0 : *std::min_element(h->req.lim.begin(), h->req.lim.end());
    if (!h->req.lim.empty()) {
        const int E = h->nelem;
        std::vector<int32_t> sq((size_t)E * E, 0);
        for (int k = 0; k < h->npairs; ++k) {
            const int i = h->h_pair[2 * k], j = h->h_pair[2 * k + 1];
            if (i < 0 || j < 0 || i >= E || j >= E) return fail(h, NBLS_ERR_ARG, "nbls_plan: a pair of the geometry names an element the trace does not have");
            sq[(size_t)i * E + j] = sq[(size_t)j * E + i] = h->req.lim[(size_t)k];
        }
        if (int rc = alloc_copy(h, h->d_limsq, sq.data(), sq.size())) return rc;
    }
    if (!h->req.seed.empty()) {          // the half-width of every result row: row r is band r / nseg
        std::vector<int32_t> rows((size_t)R);
        for (int r = 0; r < R; ++r) rows[(size_t)r] = h->req.seed[(size_t)(r / h->nseg)];
        for (size_t k = 0; k < h->h_pair.size(); ++k)
            if (h->h_pair[k] < 0 || h->h_pair[k] >= h->nelem) return fail(h, NBLS_ERR_ARG, "nbls_plan: a pair of the geometry names an element the trace does not have");
        if (int rc = alloc_copy(h, h->d_seed, rows.data(), rows.size())) return rc;
    }
    for (int b = 0; b < R; ) {
        int e = b + 1;
        while (e < R && h->W[e] == h->W[b]) ++e;
        nbls_wgroup g{b, e, h->W[b], h->unit_off[b], h->unit_off[e], false};
        // a plan with a lag seed: every group takes the seeded correlator in the general correlators' slot
        if (!h->req.seed.empty()) {
            g.sform = nbls_lag_seed_form_of(h->nelem, g.W);
            h->wgroups.push_back(g);
            b = e;
            continue;
        }
        nbls_route r;                               // (xcorr_route.hip: the launchers take the same route)
        nbls_route_compute(nbls_route_query_of(h, g.W, R, 3, false), &r);
        g.screen = h->est[0].d_xij && r.correlator == NBLS_ROUTE_SCREEN;
        // a plan with lag limits: a group whose windows are longer than the smallest limit takes the bounded-lag correlator
        // in the general correlators' slot; where every limit reaches W-1 the full search is the bounded one
        if (!h->req.lim.empty()) g.bform = nbls_lag_limit_form_of(h->nelem, g.W, std::min(min_lim, g.W - 1));
        if (g.bform) { g.screen = false; h->wgroups.push_back(g); b = e; continue; }
        if (g.screen) { any_ok = true; if (r.WP > maxWP) maxWP = r.WP; }
        else if (g.u1 > g.u0) all_ok = false;
        h->wgroups.push_back(g);
        b = e;
    }
    if (xcorr_impl == 3 && !all_ok)
        return fail(h, NBLS_ERR_UNSUPPORTED, "nbls_plan: the int8 screening correlator needs 3..33 channels and channel images that fit a CU's LDS");
    if (xcorr_impl == 0 && any_ok) xcorr_impl = 3;
    h->xcorr_impl = xcorr_impl;
    if (xcorr_impl != 3) for (nbls_wgroup& g : h->wgroups) g.screen = false;
    h->screen_wp = maxWP;
    return 0;
}

// Step 7: the unit batch of the screening correlator and its buffers.
static int plan_screen_batch(nbls_handle* h, const plan_args& a) {
    if (h->xcorr_impl != 3) return 0;
    const int E = a.E, WP_ = h->screen_wp;
    const int64_t U = h->nunits;
    int rc;
    // unit batches small enough for the quantised windows to stay in the 256 MiB Infinity Cache (192 MB: measured
    // against 96 — the value of rounds 1-2 — and 384 at every BASELINE shape: 0.2-1.2 % of the pass, fewer launch tails)
    const int64_t batch_mb = h->opt.screen_batch_mb > 0 ? h->opt.screen_batch_mb : 192;
    int64_t batch = (int64_t)(batch_mb << 20) / ((int64_t)E * 2 * WP_);
    if (batch < 64) batch = 64;
    if (batch > U) batch = U > 0 ? U : 1;
    // equal batches (a multiple of 8 units, the XCD grouping of the screening grid) instead of full ones plus a
    // remainder: a 200-unit tail batch pays four kernel launches and their drain for next to nothing
    if (U > batch) {
        const int64_t nb_ = (U + batch - 1) / batch;
        int64_t eq = ((U + nb_ - 1) / nb_ + 7) / 8 * 8;
        if (eq < batch) batch = eq;
    }
    h->screen_batch = batch;
    if ((rc = ensure(h, h->d_qbuf, (size_t)batch * E * 2 * WP_))) return rc;
    if ((rc = ensure(h, h->d_qmeta, (size_t)batch * E * (10 + WP_ / 32) * sizeof(double)))) return rc;
    if (h->opt.screen_stamps || h->opt.lts_stamps) {
        if ((rc = ensure(h, h->d_stamps, (size_t)(batch + 8) * E * ((E + 1) / 2) * 8 * sizeof(unsigned long long)))) return rc;   // one record per screening workgroup: (unit, sliding channel, partner group)
    }
    return ensure(h, h->d_cand, (size_t)batch * E * E * 32 * sizeof(int32_t));
}

// Step 8: per estimator, its array's tables (est[0]'s geometry is nbls_set_geometry's and stays where that put it) and,
// for the further ones, their own result buffers (est[0]'s were sized with the work buffers).
static int plan_estimators(nbls_handle* h, const plan_args& a) {
    int rc;
    for (int e = 0; e <= h->nest; ++e) {
        nbls_estimator& x = h->est[e];
        if (e > 0) {
            if ((rc = alloc_copy(h, x.d_xij, x.h_xij.data(), x.h_xij.size()))) return rc;
            if ((rc = alloc_copy(h, x.d_xpinv, x.h_xpinv.data(), x.h_xpinv.size()))) return rc;
            if (!x.kept_pair.empty() && (rc = alloc_copy(h, x.d_kept_pair, x.kept_pair.data(), x.kept_pair.size()))) return rc;
            if (h->req.beam && (rc = alloc_copy(h, x.d_kept, x.kept.data(), x.kept.size()))) return rc;
        }
        if (x.lts && (rc = upload_lts_tables(h, x))) return rc;
        if (e > 0 && (rc = size_result_buffers(h, x, (size_t)a.R * a.vector_len, 0))) return rc;
    }
    if (h->derived.grid_n > 0) {             // the slowness-grid search: its two tables and its result buffers, for a plan that asks only
        const size_t cells = (size_t)a.R * a.vector_len;
        if ((rc = alloc_copy(h, h->d_grid, h->req.grid.data(), h->req.grid.size()))) return rc;
        if ((rc = alloc_copy(h, h->d_grid_delay, h->derived.grid_delay.data(), h->derived.grid_delay.size()))) return rc;
        if (h->req.grid_taps() && (rc = alloc_copy(h, h->d_grid_coef, h->derived.grid_coef.data(), h->derived.grid_coef.size()))) return rc;
        if ((rc = ensure(h, h->d_grid_index, cells * sizeof(int32_t)))) return rc;
        if ((rc = ensure(h, h->d_grid_fp, 2 * cells * sizeof(double)))) return rc;
        if (h->req.grid_map() && (rc = ensure(h, h->d_grid_map, cells * (size_t)h->derived.grid_n * sizeof(double)))) return rc;
        if (h->req.grid_refined()) {         // ... and its refinement: slowness (2), fstat, power and stencil (9) per cell, and the path
            if ((rc = ensure(h, h->d_grid_refine_fp, 13 * cells * sizeof(double)))) return rc;
            if ((rc = ensure(h, h->d_grid_refine_path, cells * (size_t)h->req.grid_refine.levels * sizeof(int32_t)))) return rc;
        }
    }
    if (h->req.kept_q > 0) {             // the elements LTS kept: the mask and the count of every cell
        const size_t cells = (size_t)a.R * a.vector_len;
        if ((rc = ensure(h, h->d_kept_mask, cells * sizeof(uint32_t)))) return rc;
        if ((rc = ensure(h, h->d_kept_count, cells * sizeof(int32_t)))) return rc;
    }
    if (h->req.bt) {                     // the beam trace: the synthesis windows, where every row's starts, and the trace of every row
        std::vector<int32_t> off((size_t)a.R);
        for (int r = 0, o = 0, b = 0; r < a.R; ++r) {
            if (r / a.NS != b) { o += a.winlen[b]; ++b; }
            off[(size_t)r] = o;
        }
        if ((rc = alloc_copy(h, h->d_bt_win, h->req.bt_win.data(), h->req.bt_win.size()))) return rc;
        if ((rc = alloc_copy(h, h->d_bt_off, off.data(), off.size()))) return rc;
        if ((rc = ensure(h, h->d_bt, (size_t)a.R * (size_t)h->npts_pad * sizeof(double)))) return rc;
    }
    if (h->req.fam) {                    // the families: the union-find's arrays and the three results
        const hipError_t e = h->fam.grow((int64_t)a.R * a.vector_len, h->req.fam_par.min_pixels);
        if (e != hipSuccess) return fail(h, NBLS_ERR_NOMEM, std::string("hipMalloc (nbls_set_families): ") + hipGetErrorString(e));
    }
    if (h->req.ed) {                     // the element delays: every row's max_shift and the three grids
        const size_t vals = (size_t)a.R * a.vector_len * (size_t)a.E;
        std::vector<int32_t> kb((size_t)a.R);
        for (int r = 0; r < a.R; ++r) kb[(size_t)r] = h->req.ed_K[(size_t)(r / a.NS)];
        if ((rc = alloc_copy(h, h->d_ed_K, kb.data(), kb.size()))) return rc;
        if ((rc = ensure(h, h->d_ed_fp, 2 * vals * sizeof(double)))) return rc;
        if ((rc = ensure(h, h->d_ed_shift, vals * sizeof(int32_t)))) return rc;
    }
    if (h->derived.capon_n > 0) {            // the Capon spectra: the band tables and the result buffers, likewise
        const size_t cells = (size_t)a.R * a.vector_len;
        const int E = a.E, G = h->derived.capon_n, nb = a.nbands;
        int maxls = 1;
        h->h_capon_par.resize((size_t)nb * 3);
        for (int b = 0; b < nb; ++b) {
            const int ls = h->req.capon.ls[b], hs = h->req.capon.hs[b];
            h->h_capon_par[3 * b] = ls;
            h->h_capon_par[3 * b + 1] = hs;
            h->h_capon_par[3 * b + 2] = 1 + (a.winlen[b] - ls) / hs;
            if (ls > maxls) maxls = ls;
        }
        h->derived.capon_maxls = maxls;
        h->h_capon_coef.resize((size_t)nb * maxls * 2);
        h->h_capon_steer.resize((size_t)nb * E * G * 2);
        nbls_capon_tables_of(h->est[0].h_xij.data(), E, h->fs, h->req.capon.grid.data(), G, h->req.capon.freq.data(), h->req.capon.ls.data(),
                             nb, maxls, h->h_capon_coef.data(), h->h_capon_steer.data());
        if ((rc = alloc_copy(h, h->d_capon_par, h->h_capon_par.data(), h->h_capon_par.size()))) return rc;
        if ((rc = alloc_copy(h, h->d_capon_coef, h->h_capon_coef.data(), h->h_capon_coef.size()))) return rc;
        if ((rc = alloc_copy(h, h->d_capon_steer, h->h_capon_steer.data(), h->h_capon_steer.size()))) return rc;
        if ((rc = ensure(h, h->d_capon_index, 2 * cells * sizeof(int32_t)))) return rc;
        if ((rc = ensure(h, h->d_capon_power, 2 * cells * sizeof(double)))) return rc;
        if (h->req.capon_maps() && (rc = ensure(h, h->d_capon_map, 2 * cells * (size_t)G * sizeof(double)))) return rc;
        if ((h->req.capon_csdm() || h->req.clean.iterations > 0 || h->req.music.sources >= 0) && (rc = ensure(h, h->d_capon_csdm, cells * (size_t)E * E * 2 * sizeof(double)))) return rc;
        if (h->req.music.sources >= 0) {     // the MUSIC request: it reads R from d_capon_csdm whether or not the plan returns it
            if ((rc = ensure(h, h->d_music_eig, cells * (size_t)E * sizeof(double)))) return rc;
            if ((rc = ensure(h, h->d_music_int, 3 * cells * sizeof(int32_t)))) return rc;
            if ((rc = ensure(h, h->d_music_power, cells * sizeof(double)))) return rc;
            if ((h->req.music.flags & NBLS_MUSIC_MAP) && (rc = ensure(h, h->d_music_map, cells * (size_t)G * sizeof(double)))) return rc;
            if ((h->req.music.flags & NBLS_MUSIC_VECTORS) && (rc = ensure(h, h->d_music_vec, cells * (size_t)E * E * 2 * sizeof(double)))) return rc;
            if (h->req.music.flags & NBLS_MUSIC_PEAKS) {     // K of the plan's peak request; the slabs where the plan keeps no MUSIC map
                const size_t K = (size_t)h->req.peaks.k;
                if ((rc = ensure(h, h->d_music_peak_count, cells * sizeof(int32_t)))) return rc;
                if ((rc = ensure(h, h->d_music_peak_index, cells * K * sizeof(int32_t)))) return rc;
                if ((rc = ensure(h, h->d_music_peak_power, cells * K * sizeof(double)))) return rc;
                if ((rc = ensure(h, h->d_music_peak_offset, cells * K * 2 * sizeof(double)))) return rc;
                if (!(h->req.music.flags & NBLS_MUSIC_MAP)) {
                    const size_t slabs = std::min<size_t>((size_t)h->derived.peak_slabs, std::max<size_t>((size_t)h->nunits, 1));
                    if ((rc = ensure(h, h->d_music_slab, slabs * (size_t)G * sizeof(double)))) return rc;
                }
            }
        }
        if (h->req.clean.iterations > 0) {   // the CLEAN-SC request: it reads R from d_capon_csdm whether or not the plan returns it
            const size_t I = (size_t)h->req.clean.iterations;
            if ((rc = ensure(h, h->d_clean_count, cells * sizeof(int32_t)))) return rc;
            if ((rc = ensure(h, h->d_clean_index, cells * I * sizeof(int32_t)))) return rc;
            if ((rc = ensure(h, h->d_clean_power, cells * I * sizeof(double)))) return rc;
            if ((rc = ensure(h, h->d_clean_tr, 2 * cells * sizeof(double)))) return rc;
            if ((h->req.clean.flags & NBLS_CLEAN_RESIDUAL) && (rc = ensure(h, h->d_clean_csdm, cells * (size_t)E * E * 2 * sizeof(double)))) return rc;
        }
        if (h->req.peaks.k > 0) {    // the peak request: its neighbour table, the four results and, on the HBM route of a plan without the maps, the slabs
            const size_t K = (size_t)h->req.peaks.k;
            if ((rc = alloc_copy(h, h->d_capon_nbr, h->req.peaks.nbr.data(), h->req.peaks.nbr.size()))) return rc;
            if ((rc = ensure(h, h->d_capon_peak_count, 2 * cells * sizeof(int32_t)))) return rc;
            if ((rc = ensure(h, h->d_capon_peak_index, 2 * cells * K * sizeof(int32_t)))) return rc;
            if ((rc = ensure(h, h->d_capon_peak_power, 2 * cells * K * sizeof(double)))) return rc;
            if ((rc = ensure(h, h->d_capon_peak_offset, 2 * cells * K * 2 * sizeof(double)))) return rc;
            if (h->derived.peak_route == 2 && !h->req.capon_maps()) {
                const size_t slabs = std::min<size_t>((size_t)h->derived.peak_slabs, std::max<size_t>((size_t)h->nunits, 1));
                if ((rc = ensure(h, h->d_capon_peak_slab, slabs * 2 * (size_t)G * sizeof(double)))) return rc;
            }
        }
    }
    return 0;
}

// Step 9: the arena's tables in one piece (copies queued before it on the same stream came from other parts of the staging arena).
static int plan_upload_arena(nbls_handle* h) {
    h->arena_mode = false;
    if (h->stage && h->d_parena && h->stage_used)
        HIPCHK(h, hipMemcpyAsync(h->d_parena, h->stage, h->stage_used, hipMemcpyHostToDevice, h->up));
    return 0;
}

int nbls_plan(nbls_handle* h, int32_t nbands, const double* sos, int32_t nsections, int32_t zero_phase,
              const double* taper_left, const double* taper_right, int32_t taper_len,
              const int32_t* winlen, const int32_t* wininc, int32_t vector_len,
              const nbls_lts_params* lts, int32_t xcorr_impl) {
    if (!h) return NBLS_ERR_ARG;
    h->planned = false;
    plan_args a{nbands, sos, nsections, zero_phase, taper_left, taper_right, taper_len, winlen, wininc, vector_len, lts, xcorr_impl,
                0, 0, 0, 0, 0};
    int rc;
    if ((rc = plan_check_args(h, a))) return rc;
    const auto tp0 = std::chrono::steady_clock::now();
    plan_filter_tables(h, a);
    const auto tp1 = std::chrono::steady_clock::now();

    HIPCHK(h, hipSetDevice(h->device));
    StreamGuard guard(h);
    h->planned = false;
    h->res_loaded = false;
    h->arena_mode = true;                                // alloc_copy: places in the arena, ONE upload at the end
    if ((rc = plan_windows(h, a))) return rc;
    if ((rc = plan_upload_tables(h, a))) return rc;
    const auto tp2 = std::chrono::steady_clock::now();
    if ((rc = plan_work_buffers(h, a))) return rc;
    if ((rc = plan_window_groups(h, a))) return rc;
    if ((rc = plan_screen_batch(h, a))) return rc;
    if ((rc = plan_estimators(h, a))) return rc;
    if ((rc = plan_upload_arena(h))) return rc;
    h->planned = true;
    if (h->opt.plan_timing) {
        const auto tp3 = std::chrono::steady_clock::now();
        auto ms = [](auto t0, auto t1) { return std::chrono::duration<double, std::milli>(t1 - t0).count(); };
        fprintf(stderr, "nbls_plan: tables %.3f ms, uploads %.3f ms, buffers+rest %.3f ms\n", ms(tp0, tp1), ms(tp1, tp2), ms(tp2, tp3));
    }
    return NBLS_OK;
}

int nbls_execute(nbls_handle* h) { return nbls_execute_stages(h, 7); }

int nbls_execute_after(nbls_handle* h, nbls_handle* prev) {
    if (!h || !prev || prev == h) return NBLS_ERR_ARG;
    if (prev->device != h->device) return fail(h, NBLS_ERR_ARG, "nbls_execute_after: the two handles are on different devices");
    if (!prev->ev_xd || !prev->ev_xd_recorded) return fail(h, NBLS_ERR_STATE, "nbls_execute_after: the other handle has not queued a pass");
    h->after = prev;
    const int rc = nbls_execute_stages(h, 7);
    h->after = nullptr;
    return rc;
}

int nbls_execute_stages(nbls_handle* h, int32_t stage_mask) {
    if (!h) return NBLS_ERR_ARG;
    if (!h->planned) return fail(h, NBLS_ERR_STATE, "nbls_execute: no plan");
    if ((stage_mask & 6) && !h->est[0].d_xij) return fail(h, NBLS_ERR_STATE, "nbls_execute: no geometry set");
    // the samples: uploaded — or on their way (nbls_upload_rows on another thread): a pass with a filter stage then takes
    // the channels as they land; any other pass needs them all before it is queued
    const int upload_st = h->upload_state.load(std::memory_order_acquire);      // (read BEFORE trace_loaded: the upload thread sets that first)
    if (!((stage_mask & 1) && (upload_st == 1 || upload_st == 3)) && !h->trace_loaded)
        return fail(h, NBLS_ERR_STATE, "nbls_execute: the trace was declared (nbls_set_trace_shape) but not uploaded");
    HIPCHK(h, hipSetDevice(h->device));
    wait_uploads(h);
    h->work_queued = true;
    // padding beyond nwin[b] is zeros (narrow_band_least_squares.py:268-272): the result block (grids + weight mask) is
    // cleared here; the per-pair side arrays (lag, cmax, weights, z: 25 MB at cfg-3, five fill kernels per band group) are
    // written for every computed window and read for no other — the rows nobody computed are zeroed on the host by the
    // rare caller that fetches them (nbls_fetch: zero_uncomputed)
    // (a caller that did not wait for every streamed batch of the previous pass: its copies still read the block)
    if (!h->rbatches.empty() && h->cstream) HIPCHK(h, hipStreamWaitEvent(h->stream, h->rev[2 * (h->rbatches.size() - 1) + 1], 0));
    h->rbatches.clear();
    for (int e = 0; e <= h->nest; ++e) HIPCHK(h, hipMemsetAsync(h->est[e].d_res, 0, h->est[e].res_bytes, h->stream));
    if (h->prof) HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
    if (stage_mask & 1) {
        // every (band, channel) series is filtered on its own: the channels that have landed so far, then the next ones
        // as their events are recorded (one launch of all channels when the trace is there already)
        for (int done = 0; done < h->nchans;) {
            int landed = wait_rows(h, done);
            if (landed < 0 || landed <= done)
                return fail(h, NBLS_ERR_STATE, landed == -2 ? "nbls_execute: the announced trace did not arrive (no nbls_upload_rows within 120 s)"
                                               : landed == -3 ? "nbls_execute: the trace was declared (nbls_set_trace_shape) but not uploaded"
                                                              : "nbls_execute: the upload of the trace failed");
            if (h->opt.filter_row_step > 0 && landed > done + h->opt.filter_row_step) landed = done + h->opt.filter_row_step;   // (A/B and tests)
            if ((int)h->uev.size() >= landed) HIPCHK(h, hipStreamWaitEvent(h->stream, h->uev[landed - 1], 0));
            HIPCHK(h, nbls_launch_filter(h, done, landed - done));
            done = landed;
        }
    }
    if (h->prof) HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
    h->solve_done = false;
    h->last_stage_mask = stage_mask;
    if (stage_mask & 4) h->solve_ran = true;             // (a pass without a stage leaves the opt-in results it writes as they are)
    if (stage_mask & 2) h->xcorr_ran = true;
    // per-batch solves: behind each unit batch of the correlation stage (streamed results: a batch's rows are complete
    // while later batches are still being correlated), on the second stream with option "overlap"
    h->fuse_solve = ((stage_mask & 6) == 6) && h->xcorr_impl == 3 && (h->opt.overlap > 0 || h->stream_results);
    // option "overlap": 1 on, -1 off, 0 auto = on for a streamed pass of several SMALL unit batches (under 1024 units on
    // average: adaptive windows give every window length a batch of its own, and a batch of a few dozen units is all
    // launch latency and drain — device pass of cfg-1b 0.95 -> 0.75 ms).  Big batches gain 1.5-3 % (cfg-3 14.7 -> 14.3 ms,
    // cfg-5 174.6 -> 169.0) at the price of kernels whose measured durations include their neighbour's: left off there.
    int64_t nbatch_est = 0;
    for (const nbls_wgroup& g : h->wgroups)
        if (g.u1 > g.u0) nbatch_est += g.screen && h->screen_batch > 0 ? (g.u1 - g.u0 + h->screen_batch - 1) / h->screen_batch : 1;
    const bool small_batches = nbatch_est > 1 && h->nunits / nbatch_est < 1024;
    h->solve_on_stream2 = h->fuse_solve && h->stream2 && (h->opt.overlap > 0 || (h->opt.overlap == 0 && h->stream_results && small_batches));
    if (h->stream_results) {
        if (!h->cstream) HIPCHK(h, hipStreamCreateWithFlags(&h->cstream, hipStreamNonBlocking));
        for (int e = 0; e <= h->nest; ++e) { const int rc = ensure_mirror(h, h->est[e]); if (rc) return rc; }
    }
    // nbls_execute_after: this pass's filter may run beside the other handle's correlation stage (memory-bound next to
    // matrix-core-bound), its own correlation stage starts when the other one's is through
    if (h->after && (stage_mask & 2)) HIPCHK(h, hipStreamWaitEvent(h->stream, h->after->ev_xd, 0));
    h->ev_xd_by_launcher = false;
    if (stage_mask & 2) HIPCHK(h, nbls_launch_xcorr(h));
    if (h->ev_xd && (stage_mask & 2) && !h->ev_xd_by_launcher) { HIPCHK(h, hipEventRecord(h->ev_xd, h->stream)); h->ev_xd_recorded = true; }
    if (h->prof) HIPCHK(h, hipEventRecord(h->ev[2], h->stream));
    if ((stage_mask & 4) && !h->solve_done) HIPCHK(h, nbls_launch_solve(h));
    // the beam trace of a plan that asked for one (nbls_set_beam_trace): one launch behind the pass's last solve — per-batch
    // solves on the second stream have been joined into this one (nbls_xcorr_screen_finish) — and ahead of the closing event
    if ((stage_mask & 4) && h->req.bt) HIPCHK(h, nbls_launch_beam_trace(h, h->stream));
    // the families of a plan that asked for them (nbls_set_families): likewise one launch sequence behind the last solve
    if ((stage_mask & 4) && h->req.fam) {
        const nbls_est_view v = nbls_view_of(h, h->est[0]);
        HIPCHK(h, nbls_launch_families(h->req.fam_par, h->fam, h->nbands, h->nseg, h->vector_len, h->d_W, h->d_inc, h->d_nwin, v.vel, v.baz,
                                       v.mdccm, v.sig, h->stream));
    }
    if (h->prof) { HIPCHK(h, hipEventRecord(h->ev[3], h->stream)); h->ev_valid = true; }
    // streamed results of a pass that was not cut into batches (general correlators, stage subsets, no units): ONE batch
    if (h->stream_results && h->rbatches.empty()) HIPCHK(h, nbls_queue_result_batch(h, 0, h->nunits, h->stream));
    return NBLS_OK;
}

}  // extern "C"

// The rows of units [u0, u1) are complete once `producer` has run what is queued on it: their part of the result block
// (the cell range [c0, c1) of each of the four grids and of the mask; padding cells between two bands ride along, they
// are zero) goes to the pinned mirror on the copy stream, and an event marks the landing (nbls_wait_result_batch).
hipError_t nbls_queue_result_batch(nbls_handle* h, int64_t u0, int64_t u1, hipStream_t producer) {
    if (!h->stream_results || !h->cstream || !h->est[0].h_res) return hipSuccess;
    const size_t k = h->rbatches.size();
    while (h->rev.size() < 2 * (k + 1)) {
        hipEvent_t e;
        hipError_t ce = hipEventCreateWithFlags(&e, hipEventDisableTiming);
        if (ce != hipSuccess) return ce;
        h->rev.push_back(e);
    }
    nbls_handle::result_batch rb{u0, u1, 0, 0};
    if (u1 > u0) {
        auto cell = [&](int64_t u) {
            const int b = (int)(std::upper_bound(h->unit_off.begin(), h->unit_off.end(), (int32_t)u) - h->unit_off.begin()) - 1;
            return (int64_t)b * h->vector_len + first_window(h, b) + (u - h->unit_off[b]);
        };
        rb.c0 = cell(u0);
        rb.c1 = cell(u1 - 1) + 1;
    }
    hipError_t e = hipEventRecord(h->rev[2 * k], producer);
    if (e != hipSuccess) return e;
    if ((e = hipStreamWaitEvent(h->cstream, h->rev[2 * k], 0)) != hipSuccess) return e;
    // (the plan's own estimator, then the further ones: the event behind them marks the batch of EVERY estimator)
    for (int q = 0; q <= h->nest && rb.c1 > rb.c0; ++q) {
        const size_t cells = (size_t)h->nbands * h->vector_len;
        unsigned char* const hres = h->est[q].h_res;
        const unsigned char* const dres = h->est[q].d_res;
        const size_t mbytes = (size_t)h->est[q].mask_bytes;
        if (!hres) return hipErrorInvalidValue;
        for (int g = 0; g < 4; ++g) {
            const size_t off = ((size_t)g * cells + (size_t)rb.c0) * sizeof(double);
            if ((e = hipMemcpyAsync(hres + off, dres + off, (size_t)(rb.c1 - rb.c0) * sizeof(double), hipMemcpyDeviceToHost, h->cstream)) != hipSuccess) return e;
        }
        const size_t moff = 4 * cells * sizeof(double) + (size_t)rb.c0 * mbytes;
        if ((e = hipMemcpyAsync(hres + moff, dres + moff, (size_t)(rb.c1 - rb.c0) * mbytes, hipMemcpyDeviceToHost, h->cstream)) != hipSuccess) return e;
    }
    if ((e = hipEventRecord(h->rev[2 * k + 1], h->cstream)) != hipSuccess) return e;
    h->rbatches.push_back(rb);
    return hipSuccess;
}

extern "C" {

int nbls_stream_results(nbls_handle* h, int32_t on) {
    if (!h) return NBLS_ERR_ARG;
    h->stream_results = on != 0;
    return NBLS_OK;
}

int nbls_result_batches(nbls_handle* h, int32_t* nbatches) {
    if (!h || !nbatches) return NBLS_ERR_ARG;
    *nbatches = h->stream_results ? (int32_t)h->rbatches.size() : 0;
    return NBLS_OK;
}

int nbls_wait_result_batch(nbls_handle* h, int32_t k, int64_t* out4, const void** host_block) {
    return nbls_est_wait_result_batch(h, 0, k, out4, host_block);
}

int nbls_est_wait_result_batch(nbls_handle* h, int32_t est, int32_t k, int64_t* out4, const void** host_block) {
    if (!h) return NBLS_ERR_ARG;
    if (est < 0 || est > h->nest) return fail(h, NBLS_ERR_ARG, "nbls_est_wait_result_batch: no such estimator");
    if (!h->stream_results || k < 0 || (size_t)k >= h->rbatches.size())
        return fail(h, NBLS_ERR_STATE, "nbls_wait_result_batch: no such batch (nbls_stream_results + nbls_execute first)");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipEventSynchronize(h->rev[2 * (size_t)k + 1]));
    const nbls_handle::result_batch& rb = h->rbatches[(size_t)k];
    if (out4) { out4[0] = rb.u0; out4[1] = rb.u1; out4[2] = rb.c0; out4[3] = rb.c1; }
    if (host_block) *host_block = h->est[est].h_res;
    return NBLS_OK;
}

// Wait for the handle's stream and, when profiling is on, turn the events of the last pass into timings.
static int finish_pass(nbls_handle* h) {
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (h->cstream && !h->rbatches.empty()) HIPCHK(h, hipStreamSynchronize(h->cstream));
    h->work_queued = false;
    if (h->prof && h->ev_valid) {
        float f = 0, x = 0, s = 0, t = 0;
        HIPCHK(h, hipEventElapsedTime(&f, h->ev[0], h->ev[1]));
        HIPCHK(h, hipEventElapsedTime(&x, h->ev[1], h->ev[2]));
        HIPCHK(h, hipEventElapsedTime(&s, h->ev[2], h->ev[3]));
        HIPCHK(h, hipEventElapsedTime(&t, h->ev[0], h->ev[3]));
        h->tim.filter_ms = f; h->tim.xcorr_ms = x; h->tim.solve_ms = s; h->tim.total_ms = t;
        h->tim.quantize_ms = h->tim.screen_ms = h->tim.verify_ms = 0.0;
        double fused_solve = 0.0;
        for (int b = 0; b + 4 < h->bev_used; b += 5) {
            float q = 0, sc = 0, v = 0, so = 0;
            HIPCHK(h, hipEventElapsedTime(&q, h->bev[b], h->bev[b + 1]));
            HIPCHK(h, hipEventElapsedTime(&sc, h->bev[b + 1], h->bev[b + 2]));
            HIPCHK(h, hipEventElapsedTime(&v, h->bev[b + 2], h->bev[b + 3]));
            if (h->prof_fused) HIPCHK(h, hipEventElapsedTime(&so, h->bev[b + 3], h->bev[b + 4]));
            h->tim.quantize_ms += q; h->tim.screen_ms += sc; h->tim.verify_ms += v; fused_solve += so;
        }
        if (h->prof_fused && h->bev_used > 0) {
            // per-batch solves sit inside the correlation stage's interval: report the stages as if they were separate
            // (with option "overlap" the solves run beside the next batch's correlation: their sum is not wall time)
            h->tim.solve_ms += fused_solve;
            if (!h->solve_on_stream2) h->tim.xcorr_ms -= fused_solve;
        }
        h->bev_used = 0;
        h->tim.xcorr_impl = h->xcorr_impl_used;
        h->ev_valid = false;
    }
    return NBLS_OK;
}

int nbls_sync(nbls_handle* h) {
    if (!h) return NBLS_ERR_ARG;
    return finish_pass(h);
}

int nbls_fetch(nbls_handle* h, double* vel, double* baz, double* mdccm, double* sigma_tau, int32_t* nwin,
               int32_t* lag, double* cmax, uint8_t* weights, double* z) {
    return nbls_est_fetch(h, 0, vel, baz, mdccm, sigma_tau, nwin, lag, cmax, weights, z);
}

int nbls_est_fetch(nbls_handle* h, int32_t est, double* vel, double* baz, double* mdccm, double* sigma_tau, int32_t* nwin,
                   int32_t* lag, double* cmax, uint8_t* weights, double* z) {
    if (!h) return NBLS_ERR_ARG;
    if (!h->planned) return fail(h, NBLS_ERR_STATE, "nbls_fetch: no plan");
    if (est < 0 || est > h->nest) return fail(h, NBLS_ERR_ARG, "nbls_est_fetch: no such estimator");
    { const int rc = finish_pass(h); if (rc) return rc; }
    const size_t cells = (size_t)h->nbands * h->vector_len;
    const nbls_estimator& s = h->est[est];
    const nbls_est_view v = nbls_view_of(h, s);
    const size_t P = (size_t)s.npairs;
    const double* dg[4] = {v.vel, v.baz, v.mdccm, v.sig};
    double* hg[4] = {vel, baz, mdccm, sigma_tau};
    if (vel && baz == vel + cells && mdccm == baz + cells && sigma_tau == mdccm + cells) {
        HIPCHK(h, copy_sync(h, vel, v.vel, 4 * cells * sizeof(double), hipMemcpyDeviceToHost));   // caller's grids are one block too
    } else {
        for (int g = 0; g < 4; ++g)
            if (hg[g]) HIPCHK(h, copy_sync(h, hg[g], dg[g], cells * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (nwin) memcpy(nwin, h->nwin.data(), h->nbands * sizeof(int32_t));
    // rows of windows this plan did not compute are zeros (zero_uncomputed)
    // the side arrays are not cleared by a pass (see nbls_execute_stages): what a stage that did NOT run in the last pass
    // would have written is zeros here, not the previous pass's values
    const bool ran_x = (h->last_stage_mask & 2) != 0, ran_s = (h->last_stage_mask & 4) != 0;
    if (lag) {
        // (a sub-array's compact rows are gathered behind the verifier as part of its solve)
        const bool have = ran_x && (s.kept_pair.empty() || ran_s);
        if (have) { HIPCHK(h, copy_sync(h, lag, v.lag, cells * P * sizeof(int32_t), hipMemcpyDeviceToHost)); zero_uncomputed(h, lag, P * sizeof(int32_t)); }
        else memset(lag, 0, cells * P * sizeof(int32_t));
    }
    if (cmax) {
        const bool have = ran_x && (s.kept_pair.empty() || ran_s);
        if (have) { HIPCHK(h, copy_sync(h, cmax, v.cmax, cells * P * sizeof(double), hipMemcpyDeviceToHost)); zero_uncomputed(h, cmax, P * sizeof(double)); }
        else memset(cmax, 0, cells * P * sizeof(double));
    }
    if (weights) {
        if (ran_s) { HIPCHK(h, copy_sync(h, weights, s.d_wts, cells * P, hipMemcpyDeviceToHost)); zero_uncomputed(h, weights, P); }
        else memset(weights, 0, cells * P);
    }
    if (z) {
        if (ran_s) { HIPCHK(h, copy_sync(h, z, s.d_z, 2 * cells * sizeof(double), hipMemcpyDeviceToHost)); zero_uncomputed(h, z, 2 * sizeof(double)); }
        else memset(z, 0, 2 * cells * sizeof(double));
    }
    return NBLS_OK;
}

int nbls_set_uncertainty(nbls_handle* h, const double* eig6) {
    if (!h) return NBLS_ERR_ARG;
    h->est[0].want_unc = eig6 != nullptr;
    if (eig6) {
        if (!(eig6[0] > 0.0) || !(eig6[1] > 0.0)) return fail(h, NBLS_ERR_ARG, "nbls_set_uncertainty: the eigenvalues of X^T X must be positive");
        for (int i = 0; i < 6; ++i) h->est[0].unc_par[i] = eig6[i];
    }
    h->planned = false;                      // (the next plan sizes the output buffer)
    return NBLS_OK;
}

int nbls_fetch_uncertainty(nbls_handle* h, double* vel_uncert, double* baz_uncert) {
    return nbls_est_fetch_uncertainty(h, 0, vel_uncert, baz_uncert);
}

int nbls_est_fetch_uncertainty(nbls_handle* h, int32_t est, double* vel_uncert, double* baz_uncert) {
    if (!h) return NBLS_ERR_ARG;
    if (!h->planned) return fail(h, NBLS_ERR_STATE, "nbls_fetch_uncertainty: no plan");
    if (est < 0 || est > h->nest) return fail(h, NBLS_ERR_ARG, "nbls_est_fetch_uncertainty: no such estimator");
    const nbls_estimator& s = h->est[est];
    if (!s.want_unc || !s.d_unc) return fail(h, NBLS_ERR_STATE, "nbls_fetch_uncertainty: nbls_set_uncertainty (or the estimator's eig6) before nbls_plan");
    { const int rc = finish_pass(h); if (rc) return rc; }
    const size_t cells = (size_t)h->nbands * h->vector_len;
    const bool ran = (h->last_stage_mask & 4) != 0;          // like the grids of nbls_fetch: those of the LAST pass, or zeros
    if (int rc = fetch_plane(h, ran, vel_uncert, s.d_unc.p, sizeof(double))) return rc;
    return fetch_plane(h, ran, baz_uncert, s.d_unc.p + cells, sizeof(double));
}

int nbls_set_beam(nbls_handle* h, int32_t on) {
    if (!h) return NBLS_ERR_ARG;
    h->want.beam = on != 0;                  // consumed by the NEXT nbls_plan; an existing plan keeps what it was made with
    return NBLS_OK;
}

int nbls_fetch_beam(nbls_handle* h, double* beam_power, double* fstat) { return nbls_est_fetch_beam(h, 0, beam_power, fstat); }

int nbls_est_fetch_beam(nbls_handle* h, int32_t est, double* beam_power, double* fstat) {
    if (!h) return NBLS_ERR_ARG;
    if (!h->planned) return fail(h, NBLS_ERR_STATE, "nbls_fetch_beam: no plan");
    if (est < 0 || est > h->nest) return fail(h, NBLS_ERR_ARG, "nbls_est_fetch_beam: no such estimator");
    const nbls_estimator& s = h->est[est];
    if (!h->req.beam || !s.d_beam) return fail(h, NBLS_ERR_STATE, "nbls_fetch_beam: nbls_set_beam before nbls_plan");
    int rc;
    if ((rc = finish_pass(h))) return rc;
    const size_t cells = (size_t)h->nbands * h->vector_len;
    if ((rc = fetch_plane(h, h->solve_ran, beam_power, s.d_beam.p, sizeof(double)))) return rc;
    return fetch_plane(h, h->solve_ran, fstat, s.d_beam.p + cells, sizeof(double));
}

int nbls_set_closure(nbls_handle* h, int32_t on) {
    if (!h) return NBLS_ERR_ARG;
    h->want.closure = on != 0;               // consumed by the NEXT nbls_plan; an existing plan keeps what it was made with
    return NBLS_OK;
}

int nbls_fetch_closure(nbls_handle* h, double* consistency, double* closure_max, double* element_consistency) {
    return nbls_est_fetch_closure(h, 0, consistency, closure_max, element_consistency);
}

int nbls_est_fetch_closure(nbls_handle* h, int32_t est, double* consistency, double* closure_max, double* element_consistency) {
    if (!h) return NBLS_ERR_ARG;
    if (!h->planned) return fail(h, NBLS_ERR_STATE, "nbls_fetch_closure: no plan");
    if (est < 0 || est > h->nest) return fail(h, NBLS_ERR_ARG, "nbls_est_fetch_closure: no such estimator");
    const nbls_estimator& s = h->est[est];
    if (!h->req.closure || !s.d_closure || !s.d_closure_el) return fail(h, NBLS_ERR_STATE, "nbls_fetch_closure: nbls_set_closure before nbls_plan");
    int rc;
    if ((rc = finish_pass(h))) return rc;
    const size_t cells = (size_t)h->nbands * h->vector_len;
    const size_t N = s.kept.empty() ? (size_t)h->nelem : s.kept.size();
    if ((rc = fetch_plane(h, h->solve_ran, consistency, s.d_closure.p, sizeof(double)))) return rc;
    if ((rc = fetch_plane(h, h->solve_ran, closure_max, s.d_closure.p + cells, sizeof(double)))) return rc;
    return fetch_plane(h, h->solve_ran, element_consistency, s.d_closure_el.p, N * sizeof(double));
}

int nbls_set_kept_elements(nbls_handle* h, int32_t min_pairs, int32_t flags) {
    if (!h) return NBLS_ERR_ARG;
    if (min_pairs < 0) return fail(h, NBLS_ERR_ARG, "nbls_set_kept_elements: min_pairs must not be negative");
    if (flags & ~(NBLS_KEPT_BEAM | NBLS_KEPT_CAPON)) return fail(h, NBLS_ERR_ARG, "nbls_set_kept_elements: unknown flags");
    h->want.kept_q = min_pairs;              // consumed by the NEXT nbls_plan; an existing plan keeps what it was made with
    h->want.kept_flags = min_pairs > 0 ? flags : 0;
    return NBLS_OK;
}

int nbls_fetch_kept_elements(nbls_handle* h, uint32_t* dropped_mask, int32_t* kept_count) {
    if (!h) return NBLS_ERR_ARG;
    if (!h->planned) return fail(h, NBLS_ERR_STATE, "nbls_fetch_kept_elements: no plan");
    if (h->req.kept_q < 1 || !h->d_kept_mask || !h->d_kept_count) return fail(h, NBLS_ERR_STATE, "nbls_fetch_kept_elements: nbls_set_kept_elements before nbls_plan");
    int rc;
    if ((rc = finish_pass(h))) return rc;
    if ((rc = fetch_plane(h, h->solve_ran, dropped_mask, h->d_kept_mask.p, sizeof(uint32_t)))) return rc;
    return fetch_plane(h, h->solve_ran, kept_count, h->d_kept_count.p, sizeof(int32_t));
}

int nbls_set_beam_trace(nbls_handle* h, const double* window, int64_t nwindow, double mdccm_min, int32_t flags) {
    if (!h) return NBLS_ERR_ARG;
    if (!window) { h->want.bt = false; h->want.bt_win.clear(); h->want.bt_flags = 0; return NBLS_OK; }    // off: the next plan forms no trace
    if (nwindow < 0) return fail(h, NBLS_ERR_ARG, "nbls_set_beam_trace: nwindow must not be negative");
    if (flags & ~NBLS_BEAM_TRACE_KEPT) return fail(h, NBLS_ERR_ARG, "nbls_set_beam_trace: unknown flags");
    h->want.bt = true;                       // consumed by the NEXT nbls_plan; an existing plan keeps what it was made with
    h->want.bt_win.assign(window, window + nwindow);
    h->want.bt_min = mdccm_min;
    h->want.bt_flags = flags;
    return NBLS_OK;
}

int nbls_fetch_beam_trace(nbls_handle* h, int32_t row, double* out) {
    if (!h || !out) return NBLS_ERR_ARG;
    if (!h->planned) return fail(h, NBLS_ERR_STATE, "nbls_fetch_beam_trace: no plan");
    if (!h->req.bt || !h->d_bt) return fail(h, NBLS_ERR_STATE, "nbls_fetch_beam_trace: nbls_set_beam_trace before nbls_plan");
    if (row < 0 || row >= h->nbands) return fail(h, NBLS_ERR_ARG, "nbls_fetch_beam_trace: row out of range");
    { const int rc = finish_pass(h); if (rc) return rc; }
    // written behind the solve stage alone: zeros until a pass of this plan has run it, and a later pass without it leaves
    // the trace as it is
    if (!h->solve_ran) { memset(out, 0, (size_t)h->npts * sizeof(double)); return NBLS_OK; }
    HIPCHK(h, copy_sync(h, out, h->d_bt + (size_t)row * h->npts_pad, (size_t)h->npts * sizeof(double), hipMemcpyDeviceToHost));
    return NBLS_OK;
}

// What is wrong with a family request (nbls_set_families, nbls_label_families); empty: nothing.
static std::string family_params_error(const nbls_family_params& p) {
    if (!std::isfinite(p.mdccm_min)) return "mdccm_min must be finite";
    if (!std::isfinite(p.vel_min) || !std::isfinite(p.vel_max) || !(p.vel_min <= p.vel_max)) return "vel_min <= vel_max, both finite";
    if (std::isinf(p.sigma_tau_max)) return "sigma_tau_max must be finite, or NaN for no gate";
    if (!(p.baz_tol >= 0.0 && p.baz_tol <= 180.0)) return "baz_tol must lie in [0, 180]";
    if (!(p.vel_tol >= 0.0) || std::isinf(p.vel_tol)) return "vel_tol must be finite and not negative";
    if (p.band_reach < 0 || p.band_reach > NBLS_FAMILY_MAX_REACH) return "band_reach must lie in 0.." + std::to_string(NBLS_FAMILY_MAX_REACH);
    if (p.time_reach < 1 || p.time_reach > NBLS_FAMILY_MAX_REACH) return "time_reach must lie in 1.." + std::to_string(NBLS_FAMILY_MAX_REACH);
    if (p.min_pixels < 1) return "min_pixels must be at least 1";
    if (p.flags != 0) return "unknown flags";
    return std::string();
}

int nbls_set_families(nbls_handle* h, const nbls_family_params* params) {
    if (!h) return NBLS_ERR_ARG;
    if (!params) { h->want.fam = false; h->want.fam_par = nbls_family_params{}; return NBLS_OK; }    // off: the next plan labels nothing
    const std::string bad = family_params_error(*params);
    if (!bad.empty()) return fail(h, NBLS_ERR_ARG, "nbls_set_families: " + bad);
    h->want.fam = true;                      // consumed by the NEXT nbls_plan; an existing plan keeps what it was made with
    h->want.fam_par = *params;
    return NBLS_OK;
}

// The three results of a labelling of `cells` cells to the host; valid false: nothing has been labelled yet.
static int fetch_family_results(nbls_handle* h, const nbls_family_work& wk, size_t cells, int min_pixels, bool valid, int32_t* family,
                                int32_t* nfamilies, int64_t* table, int64_t capacity) {
    if (!valid) {
        if (family) for (size_t i = 0; i < cells; ++i) family[i] = -1;
        if (nfamilies) *nfamilies = 0;
        return NBLS_OK;
    }
    int32_t F = 0;
    HIPCHK(h, copy_sync(h, &F, wk.nfam.p, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (nfamilies) *nfamilies = F;
    if (family) HIPCHK(h, copy_sync(h, family, wk.family.p, cells * sizeof(int32_t), hipMemcpyDeviceToHost));
    int64_t n = F < capacity ? F : capacity;
    const int64_t have = (int64_t)nbls_family_table_rows_of((int64_t)cells, min_pixels);
    if (n > have) n = have;
    if (table && n > 0) HIPCHK(h, copy_sync(h, table, wk.table.p, (size_t)n * NBLS_FAMILY_COLUMNS * sizeof(int64_t), hipMemcpyDeviceToHost));
    return NBLS_OK;
}

int nbls_fetch_families(nbls_handle* h, int32_t* family, int32_t* nfamilies, int64_t* table, int64_t capacity) {
    if (!h) return NBLS_ERR_ARG;
    if (!h->planned) return fail(h, NBLS_ERR_STATE, "nbls_fetch_families: no plan");
    if (!h->req.fam || !h->fam.family) return fail(h, NBLS_ERR_STATE, "nbls_fetch_families: nbls_set_families before nbls_plan");
    if (table && capacity < 0) return fail(h, NBLS_ERR_ARG, "nbls_fetch_families: capacity must not be negative");
    { const int rc = finish_pass(h); if (rc) return rc; }
    // written behind the solve stage alone: nothing labelled until a pass of this plan has run it
    return fetch_family_results(h, h->fam, (size_t)h->nbands * h->vector_len, h->req.fam_par.min_pixels, h->solve_ran, family, nfamilies,
                                table, capacity);
}

int nbls_label_families(nbls_handle* h, const nbls_family_params* params, int32_t nbands, int32_t nseg, int32_t vector_len,
                        const int32_t* winlen, const int32_t* wininc, const int32_t* nwin, const double* vel, const double* baz,
                        const double* mdccm, const double* sigma_tau, int32_t* family, int32_t* nfamilies, int64_t* table,
                        int64_t capacity) {
    if (!h) return NBLS_ERR_ARG;
    if (!params || nbands < 1 || nseg < 1 || vector_len < 1 || !winlen || !wininc || !nwin || !vel || !baz || !mdccm)
        return fail(h, NBLS_ERR_ARG, "nbls_label_families: bad argument");
    const std::string bad = family_params_error(*params);
    if (!bad.empty()) return fail(h, NBLS_ERR_ARG, "nbls_label_families: " + bad);
    const bool gate = params->sigma_tau_max == params->sigma_tau_max;
    if (gate != (sigma_tau != nullptr))
        return fail(h, NBLS_ERR_ARG, "nbls_label_families: sigma_tau is given exactly when sigma_tau_max is not NaN");
    if (table && capacity < 0) return fail(h, NBLS_ERR_ARG, "nbls_label_families: capacity must not be negative");
    const int64_t rows = (int64_t)nbands * nseg, ncells = rows * vector_len;
    if (ncells >= ((int64_t)1 << 31)) return fail(h, NBLS_ERR_ARG, "nbls_label_families: fewer than 2^31 cells are taken");
    std::vector<int32_t> tabs((size_t)(3 * rows));
    for (int64_t r = 0; r < rows; ++r) {
        const int b = (int)(r / nseg);
        if (winlen[b] < 1 || wininc[b] < 1)
            return fail(h, NBLS_ERR_ARG, "nbls_label_families: window length and hop of band " + std::to_string(b) + " must be positive");
        if (nwin[r] < 0 || nwin[r] > vector_len)
            return fail(h, NBLS_ERR_ARG, "nbls_label_families: nwin of row " + std::to_string(r) + " is " + std::to_string(nwin[r]) +
                                             ", not in 0.." + std::to_string(vector_len));
        tabs[(size_t)r] = winlen[b];
        tabs[(size_t)(rows + r)] = wininc[b];
        tabs[(size_t)(2 * rows + r)] = nwin[r];
    }
    HIPCHK(h, hipSetDevice(h->device));
    nbls_family_work& wk = h->fam_label;
    const size_t cells = (size_t)ncells, ngrids = gate ? 4 : 3;
    {
        hipError_t e = wk.grow(ncells, params->min_pixels);
        if (e == hipSuccess) e = wk.grids.grow(ngrids * cells * sizeof(double));
        if (e == hipSuccess) e = wk.tabs.grow(tabs.size() * sizeof(int32_t));
        if (e != hipSuccess) return fail(h, NBLS_ERR_NOMEM, std::string("hipMalloc (nbls_label_families): ") + hipGetErrorString(e));
    }
    const double* src[4] = {vel, baz, mdccm, sigma_tau};
    for (size_t g = 0; g < ngrids; ++g)
        HIPCHK(h, hipMemcpyAsync(wk.grids.p + g * cells, src[g], cells * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, copy_sync(h, wk.tabs.p, tabs.data(), tabs.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(h, nbls_launch_families(*params, wk, (int)rows, nseg, vector_len, wk.tabs.p, wk.tabs.p + rows, wk.tabs.p + 2 * rows, wk.grids.p,
                                   wk.grids.p + cells, wk.grids.p + 2 * cells, gate ? wk.grids.p + 3 * cells : nullptr, h->stream));
    return fetch_family_results(h, wk, cells, params->min_pixels, true, family, nfamilies, table, capacity);
}

int nbls_set_element_delays(nbls_handle* h, const int32_t* max_shift, int32_t nbands, int32_t flags) {
    if (!h) return NBLS_ERR_ARG;
    if (!max_shift) { h->want.ed = false; h->want.ed_K.clear(); h->want.ed_flags = 0; return NBLS_OK; }   // off: the next plan measures none
    if (nbands < 1) return fail(h, NBLS_ERR_ARG, "nbls_set_element_delays: nbands must be at least 1");
    if (flags & ~NBLS_ELEMENT_DELAY_KEPT) return fail(h, NBLS_ERR_ARG, "nbls_set_element_delays: unknown flags");
    for (int b = 0; b < nbands; ++b)
        if (max_shift[b] < 0 || max_shift[b] > NBLS_ELEMENT_DELAY_MAX_SHIFT)
            return fail(h, NBLS_ERR_ARG, "nbls_set_element_delays: max_shift of band " + std::to_string(b) + " is " + std::to_string(max_shift[b]) +
                                             ", not in 0.." + std::to_string(NBLS_ELEMENT_DELAY_MAX_SHIFT));
    h->want.ed = true;                       // consumed by the NEXT nbls_plan; an existing plan keeps what it was made with
    h->want.ed_K.assign(max_shift, max_shift + nbands);
    h->want.ed_flags = flags;
    return NBLS_OK;
}

int nbls_fetch_element_delays(nbls_handle* h, double* delay, double* cc, int32_t* shift) {
    if (!h) return NBLS_ERR_ARG;
    if (!h->planned) return fail(h, NBLS_ERR_STATE, "nbls_fetch_element_delays: no plan");
    if (!h->req.ed || !h->d_ed_fp || !h->d_ed_shift) return fail(h, NBLS_ERR_STATE, "nbls_fetch_element_delays: nbls_set_element_delays before nbls_plan");
    int rc;
    if ((rc = finish_pass(h))) return rc;
    const size_t cells = (size_t)h->nbands * h->vector_len, N = (size_t)h->nelem;
    if ((rc = fetch_plane(h, h->solve_ran, delay, h->d_ed_fp.p, N * sizeof(double)))) return rc;
    if ((rc = fetch_plane(h, h->solve_ran, cc, h->d_ed_fp.p + cells * N, N * sizeof(double)))) return rc;
    return fetch_plane(h, h->solve_ran, shift, h->d_ed_shift.p, N * sizeof(int32_t));
}

int nbls_element_delay_lds_bytes(int32_t nelem, int32_t W, int32_t max_shift) {
    if (nelem < 1 || W < 1 || max_shift < 0 || max_shift > NBLS_ELEMENT_DELAY_MAX_SHIFT) return NBLS_ERR_ARG;
    return (int)nbls_element_delay_lds_bytes_of(nelem, W, max_shift);
}

int nbls_set_beam_grid(nbls_handle* h, const double* grid, int32_t G, int32_t want_map) {
    if (!h) return NBLS_ERR_ARG;
    if (!grid) { h->want.grid.clear(); h->want.grid_keep_map = false; return NBLS_OK; }      // off: the next plan does not search
    if (G < 1 || G > NBLS_BEAM_GRID_MAX) return fail(h, NBLS_ERR_ARG, "nbls_set_beam_grid: G must be 1.." + std::to_string(NBLS_BEAM_GRID_MAX));
    for (int64_t k = 0; k < 2 * (int64_t)G; ++k)                 // everything is checked before the handle changes
        if (!(fabs(grid[k]) < INFINITY)) return fail(h, NBLS_ERR_ARG, "nbls_set_beam_grid: slowness vector " + std::to_string(k / 2) + " is not finite");
    h->want.grid.assign(grid, grid + 2 * (size_t)G);             // consumed by the NEXT nbls_plan; an existing plan keeps what it was made with
    h->want.grid_keep_map = want_map != 0;
    return NBLS_OK;
}

int nbls_beam_grid_lds_bytes(int32_t nelem, int32_t W, int32_t halo) {
    if (nelem < 1 || W < 1 || halo < 0) return NBLS_ERR_ARG;
    return (int)nbls_beam_grid_lds_bytes_of(nelem, W, halo);
}

// what the three grid fetches share: the plan asked, and the pass is through
static int grid_fetch_ready(nbls_handle* h, const char* who, bool map) {
    if (!h->planned) return fail(h, NBLS_ERR_STATE, std::string(who) + ": no plan");
    if (h->derived.grid_n < 1 || !h->d_grid_index) return fail(h, NBLS_ERR_STATE, std::string(who) + ": nbls_set_beam_grid before nbls_plan");
    if (map && (!h->req.grid_map() || !h->d_grid_map)) return fail(h, NBLS_ERR_STATE, std::string(who) + ": the plan did not ask for the map (nbls_set_beam_grid, want_map)");
    return finish_pass(h);
}

int nbls_fetch_beam_grid(nbls_handle* h, int32_t* index, double* fstat, double* power) {
    if (!h) return NBLS_ERR_ARG;
    { const int rc = grid_fetch_ready(h, "nbls_fetch_beam_grid", false); if (rc) return rc; }
    const size_t cells = (size_t)h->nbands * h->vector_len;
    int rc;
    if ((rc = fetch_plane(h, h->grid_ran(), index, h->d_grid_index.p, sizeof(int32_t)))) return rc;
    if ((rc = fetch_plane(h, h->grid_ran(), fstat, h->d_grid_fp.p, sizeof(double)))) return rc;
    return fetch_plane(h, h->grid_ran(), power, h->d_grid_fp.p + cells, sizeof(double));
}

int nbls_set_beam_grid_refinement(nbls_handle* h, int32_t levels, const double* step) {
    if (!h) return NBLS_ERR_ARG;
    if (levels == 0 || !step) { h->want.grid_refine = nbls_requests::grid_refine_request(); return NBLS_OK; }   // off: the next plan does not refine
    if (levels < 1 || levels > NBLS_BEAM_GRID_REFINE_MAX_LEVELS)
        return fail(h, NBLS_ERR_ARG, "nbls_set_beam_grid_refinement: levels must be 0 (off) or 1.." + std::to_string(NBLS_BEAM_GRID_REFINE_MAX_LEVELS));
    for (int k = 0; k < 2; ++k)
        if (!(step[k] > 0.0 && step[k] < INFINITY))
            return fail(h, NBLS_ERR_ARG, "nbls_set_beam_grid_refinement: step " + std::to_string(k) + " must be finite and > 0");
    nbls_requests::grid_refine_request r;    // consumed by the NEXT nbls_plan; an existing plan keeps what it was made with
    r.levels = levels;
    r.step[0] = step[0]; r.step[1] = step[1];
    h->want.grid_refine = r;
    return NBLS_OK;
}

int nbls_beam_grid_refine_lds_bytes(int32_t nelem, int32_t W, int32_t halo) {
    if (nelem < 1 || W < 1 || halo < 0) return NBLS_ERR_ARG;
    return (int)nbls_beam_grid_refine_lds_bytes_of(nelem, W, halo);
}

int nbls_fetch_beam_grid_refined(nbls_handle* h, double* slowness, double* fstat, double* power, int32_t* path, double* stencil) {
    if (!h) return NBLS_ERR_ARG;
    if (!h->planned) return fail(h, NBLS_ERR_STATE, "nbls_fetch_beam_grid_refined: no plan");
    if (!h->req.grid_refined() || !h->d_grid_refine_fp || !h->d_grid_refine_path)
        return fail(h, NBLS_ERR_STATE, "nbls_fetch_beam_grid_refined: nbls_set_beam_grid_refinement before nbls_plan");
    { const int rc = finish_pass(h); if (rc) return rc; }
    const size_t cells = (size_t)h->nbands * h->vector_len;
    const double* fp = h->d_grid_refine_fp.p;
    int rc;
    if ((rc = fetch_plane(h, h->solve_ran, slowness, fp, 2 * sizeof(double)))) return rc;
    if ((rc = fetch_plane(h, h->solve_ran, fstat, fp + 2 * cells, sizeof(double)))) return rc;
    if ((rc = fetch_plane(h, h->solve_ran, power, fp + 3 * cells, sizeof(double)))) return rc;
    if ((rc = fetch_plane(h, h->solve_ran, path, h->d_grid_refine_path.p, (size_t)h->req.grid_refine.levels * sizeof(int32_t)))) return rc;
    return fetch_plane(h, h->solve_ran, stencil, fp + 4 * cells, 9 * sizeof(double));
}

int nbls_fetch_beam_grid_map(nbls_handle* h, double* map) {
    if (!h || !map) return NBLS_ERR_ARG;
    { const int rc = grid_fetch_ready(h, "nbls_fetch_beam_grid_map", true); if (rc) return rc; }
    return fetch_plane(h, h->grid_ran(), map, h->d_grid_map.p, (size_t)h->derived.grid_n * sizeof(double));
}

int nbls_fetch_beam_grid_delays(nbls_handle* h, int32_t* d) {
    if (!h || !d) return NBLS_ERR_ARG;
    if (!h->planned) return fail(h, NBLS_ERR_STATE, "nbls_fetch_beam_grid_delays: no plan");
    if (h->derived.grid_n < 1) return fail(h, NBLS_ERR_STATE, "nbls_fetch_beam_grid_delays: nbls_set_beam_grid before nbls_plan");
    memcpy(d, h->derived.grid_delay.data(), h->derived.grid_delay.size() * sizeof(int32_t));   // the plan's own table (the device holds a copy)
    return NBLS_OK;
}

int nbls_set_capon(nbls_handle* h, const double* grid, int32_t G, const double* freq, const int32_t* snap_len,
                   const int32_t* snap_hop, int32_t nbands, double loading, int32_t flags) {
    if (!h) return NBLS_ERR_ARG;
    if (!grid || G == 0) { h->want.capon = nbls_requests::capon_request(); return NBLS_OK; }      // off: the next plan computes no spectra
    if (G < 1 || G > NBLS_CAPON_GRID_MAX) return fail(h, NBLS_ERR_ARG, "nbls_set_capon: G must be 1.." + std::to_string(NBLS_CAPON_GRID_MAX));
    if (nbands < 1 || !freq || !snap_len || !snap_hop) return fail(h, NBLS_ERR_ARG, "nbls_set_capon: at least one band with its frequency, snapshot length and hop");
    for (int64_t k = 0; k < 2 * (int64_t)G; ++k)                 // everything is checked before the handle changes
        if (!(fabs(grid[k]) < INFINITY)) return fail(h, NBLS_ERR_ARG, "nbls_set_capon: slowness vector " + std::to_string(k / 2) + " is not finite");
    for (int b = 0; b < nbands; ++b) {
        if (!(freq[b] > 0.0 && freq[b] < INFINITY)) return fail(h, NBLS_ERR_ARG, "nbls_set_capon: the frequency of band " + std::to_string(b) + " is not in (0, inf)");
        if (snap_len[b] < 1 || snap_hop[b] < 1) return fail(h, NBLS_ERR_ARG, "nbls_set_capon: the snapshot length and hop of band " + std::to_string(b) + " must be at least 1");
    }
    if (!(loading >= 0.0 && loading < INFINITY)) return fail(h, NBLS_ERR_ARG, "nbls_set_capon: the loading must be finite and not negative");
    nbls_requests::capon_request& c = h->want.capon;               // consumed by the NEXT nbls_plan; an existing plan keeps what it was made with
    c.grid.assign(grid, grid + 2 * (size_t)G);
    c.freq.assign(freq, freq + nbands);
    c.ls.assign(snap_len, snap_len + nbands);
    c.hs.assign(snap_hop, snap_hop + nbands);
    c.loading = loading;
    c.flags = flags;
    return NBLS_OK;
}

// what the Capon fetches share: the plan asked, and the pass is through
static int capon_fetch_ready(nbls_handle* h, const char* who) {
    if (!h->planned) return fail(h, NBLS_ERR_STATE, std::string(who) + ": no plan");
    if (h->derived.capon_n < 1 || !h->d_capon_index) return fail(h, NBLS_ERR_STATE, std::string(who) + ": nbls_set_capon before nbls_plan");
    return 0;
}

int nbls_fetch_capon(nbls_handle* h, int32_t* capon_index, double* capon_power, int32_t* bartlett_index, double* bartlett_power) {
    if (!h) return NBLS_ERR_ARG;
    int rc;
    if ((rc = capon_fetch_ready(h, "nbls_fetch_capon")) || (rc = finish_pass(h))) return rc;
    const size_t cells = (size_t)h->nbands * h->vector_len;
    if ((rc = fetch_plane(h, h->solve_ran, capon_index, h->d_capon_index.p, sizeof(int32_t)))) return rc;
    if ((rc = fetch_plane(h, h->solve_ran, bartlett_index, h->d_capon_index.p + cells, sizeof(int32_t)))) return rc;
    if ((rc = fetch_plane(h, h->solve_ran, capon_power, h->d_capon_power.p, sizeof(double)))) return rc;
    return fetch_plane(h, h->solve_ran, bartlett_power, h->d_capon_power.p + cells, sizeof(double));
}

int nbls_set_capon_peaks(nbls_handle* h, const int32_t* cell, int32_t G, int32_t K, double floor) {
    if (!h) return NBLS_ERR_ARG;
    if (!cell || K == 0) { h->want.peaks = nbls_requests::capon_peak_request(); return NBLS_OK; }   // off: the next plan picks no peaks
    if (K < 1 || K > NBLS_CAPON_PEAKS_MAX) return fail(h, NBLS_ERR_ARG, "nbls_set_capon_peaks: K must be 1.." + std::to_string(NBLS_CAPON_PEAKS_MAX));
    if (G < 1 || G > NBLS_CAPON_GRID_MAX) return fail(h, NBLS_ERR_ARG, "nbls_set_capon_peaks: G must be 1.." + std::to_string(NBLS_CAPON_GRID_MAX));
    if (!(floor >= 0.0 && floor <= 1.0)) return fail(h, NBLS_ERR_ARG, "nbls_set_capon_peaks: the floor must lie in [0, 1]");
    std::vector<int32_t> key((size_t)G);                         // everything is checked before the handle changes
    for (int g = 0; g < G; ++g) {
        const int32_t i = cell[2 * g], j = cell[2 * g + 1];
        if (i < 0 || i >= 32768 || j < 0 || j >= 32768)
            return fail(h, NBLS_ERR_ARG, "nbls_set_capon_peaks: the lattice coordinates of point " + std::to_string(g) + " are not in 0..32767");
        key[g] = i * 32768 + j;
    }
    std::sort(key.begin(), key.end());
    if (std::adjacent_find(key.begin(), key.end()) != key.end())
        return fail(h, NBLS_ERR_ARG, "nbls_set_capon_peaks: two points share one lattice cell");
    nbls_requests::capon_peak_request& r = h->want.peaks;    // consumed by the NEXT nbls_plan; an existing plan keeps what it was made with
    r.nbr.resize((size_t)8 * G);
    nbls_capon_neighbours_of(cell, G, r.nbr.data());
    r.k = K;
    r.floor = floor;
    return NBLS_OK;
}

int nbls_fetch_capon_peaks(nbls_handle* h, int32_t which, int32_t* count, int32_t* index, double* power, double* offset) {
    if (!h) return NBLS_ERR_ARG;
    int rc;
    if ((rc = capon_fetch_ready(h, "nbls_fetch_capon_peaks"))) return rc;
    if (which < 0 || which > 1) return fail(h, NBLS_ERR_ARG, "nbls_fetch_capon_peaks: which is 0 (Capon) or 1 (Bartlett)");
    if (h->req.peaks.k < 1 || !h->d_capon_peak_count) return fail(h, NBLS_ERR_STATE, "nbls_fetch_capon_peaks: the plan did not ask for the peaks (nbls_set_capon_peaks before nbls_plan)");
    if ((rc = finish_pass(h))) return rc;
    const size_t cells = (size_t)h->nbands * h->vector_len, K = (size_t)h->req.peaks.k, w = (size_t)which;
    if ((rc = fetch_plane(h, h->solve_ran, count, h->d_capon_peak_count.p + w * cells, sizeof(int32_t)))) return rc;
    if ((rc = fetch_plane(h, h->solve_ran, index, h->d_capon_peak_index.p + w * cells * K, K * sizeof(int32_t)))) return rc;
    if ((rc = fetch_plane(h, h->solve_ran, power, h->d_capon_peak_power.p + w * cells * K, K * sizeof(double)))) return rc;
    return fetch_plane(h, h->solve_ran, offset, h->d_capon_peak_offset.p + w * cells * K * 2, K * 2 * sizeof(double));
}

int nbls_fetch_capon_maps(nbls_handle* h, double* capon_map, double* bartlett_map) {
    if (!h) return NBLS_ERR_ARG;
    int rc;
    if ((rc = capon_fetch_ready(h, "nbls_fetch_capon_maps"))) return rc;
    if (!h->req.capon_maps() || !h->d_capon_map) return fail(h, NBLS_ERR_STATE, "nbls_fetch_capon_maps: the plan did not ask for the maps (nbls_set_capon, NBLS_CAPON_MAPS)");
    if ((rc = finish_pass(h))) return rc;
    const size_t cells = (size_t)h->nbands * h->vector_len, row = (size_t)h->derived.capon_n * sizeof(double);
    if ((rc = fetch_plane(h, h->solve_ran, capon_map, h->d_capon_map.p, row))) return rc;
    return fetch_plane(h, h->solve_ran, bartlett_map, h->d_capon_map.p + cells * h->derived.capon_n, row);
}

int nbls_fetch_capon_csdm(nbls_handle* h, double* R) {
    if (!h || !R) return NBLS_ERR_ARG;
    int rc;
    if ((rc = capon_fetch_ready(h, "nbls_fetch_capon_csdm"))) return rc;
    if (!h->req.capon_csdm() || !h->d_capon_csdm) return fail(h, NBLS_ERR_STATE, "nbls_fetch_capon_csdm: the plan did not ask for the matrix (nbls_set_capon, NBLS_CAPON_CSDM)");
    if ((rc = finish_pass(h))) return rc;
    return fetch_plane(h, h->solve_ran, R, h->d_capon_csdm.p, (size_t)h->nelem * h->nelem * 2 * sizeof(double));
}

int nbls_set_capon_clean(nbls_handle* h, int32_t iterations, double gain, double floor, int32_t flags) {
    if (!h) return NBLS_ERR_ARG;
    if (iterations == 0) { h->want.clean = nbls_requests::capon_clean_request(); return NBLS_OK; }   // off: the next plan launches no capon_clean_kernel
    if (iterations < 1 || iterations > NBLS_CAPON_CLEAN_MAX) return fail(h, NBLS_ERR_ARG, "nbls_set_capon_clean: iterations must be 1.." + std::to_string(NBLS_CAPON_CLEAN_MAX));
    if (!(gain > 0.0 && gain <= 1.0)) return fail(h, NBLS_ERR_ARG, "nbls_set_capon_clean: the gain must lie in (0, 1]");
    if (!(floor >= 0.0 && floor < 1.0)) return fail(h, NBLS_ERR_ARG, "nbls_set_capon_clean: the floor must lie in [0, 1)");
    if (flags & ~NBLS_CLEAN_RESIDUAL) return fail(h, NBLS_ERR_ARG, "nbls_set_capon_clean: unknown flags");
    nbls_requests::capon_clean_request& r = h->want.clean;         // consumed by the NEXT nbls_plan; an existing plan keeps what it was made with
    r.iterations = iterations;
    r.gain = gain;
    r.floor = floor;
    r.flags = flags;
    return NBLS_OK;
}

int nbls_fetch_capon_clean(nbls_handle* h, int32_t* count, int32_t* index, double* power, double* total, double* residual) {
    if (!h) return NBLS_ERR_ARG;
    int rc;
    if ((rc = capon_fetch_ready(h, "nbls_fetch_capon_clean"))) return rc;
    if (h->req.clean.iterations < 1 || !h->d_clean_count) return fail(h, NBLS_ERR_STATE, "nbls_fetch_capon_clean: the plan did not ask for the components (nbls_set_capon_clean before nbls_plan)");
    if ((rc = finish_pass(h))) return rc;
    const size_t cells = (size_t)h->nbands * h->vector_len, I = (size_t)h->req.clean.iterations;
    if ((rc = fetch_plane(h, h->solve_ran, count, h->d_clean_count.p, sizeof(int32_t)))) return rc;
    if ((rc = fetch_plane(h, h->solve_ran, index, h->d_clean_index.p, I * sizeof(int32_t)))) return rc;
    if ((rc = fetch_plane(h, h->solve_ran, power, h->d_clean_power.p, I * sizeof(double)))) return rc;
    if ((rc = fetch_plane(h, h->solve_ran, total, h->d_clean_tr.p, sizeof(double)))) return rc;
    return fetch_plane(h, h->solve_ran, residual, h->d_clean_tr.p + cells, sizeof(double));
}

int nbls_fetch_capon_clean_csdm(nbls_handle* h, double* R) {
    if (!h || !R) return NBLS_ERR_ARG;
    int rc;
    if ((rc = capon_fetch_ready(h, "nbls_fetch_capon_clean_csdm"))) return rc;
    if (h->req.clean.iterations < 1 || !(h->req.clean.flags & NBLS_CLEAN_RESIDUAL) || !h->d_clean_csdm)
        return fail(h, NBLS_ERR_STATE, "nbls_fetch_capon_clean_csdm: the plan did not ask for the residual matrix (nbls_set_capon_clean, NBLS_CLEAN_RESIDUAL)");
    if ((rc = finish_pass(h))) return rc;
    return fetch_plane(h, h->solve_ran, R, h->d_clean_csdm.p, (size_t)h->nelem * h->nelem * 2 * sizeof(double));
}

int nbls_capon_clean_lds_bytes(int32_t nelem) {
    if (nelem < 1 || nelem > NBLS_CAPON_MAX_ELEMENTS) return NBLS_ERR_ARG;
    return (int)nbls_capon_clean_lds_bytes_of(nelem);
}

int nbls_set_capon_music(nbls_handle* h, int32_t sources, double eig_floor, double peak_floor, int32_t flags) {
    if (!h) return NBLS_ERR_ARG;
    if (sources == -1) { h->want.music = nbls_requests::capon_music_request(); return NBLS_OK; }   // off: the next plan launches no capon_music_kernel
    if (sources < 0 || sources > NBLS_CAPON_MAX_ELEMENTS - 1) return fail(h, NBLS_ERR_ARG, "nbls_set_capon_music: sources must be -1 (off), 0 (by the floor) or 1.." + std::to_string(NBLS_CAPON_MAX_ELEMENTS - 1));
    if (sources == 0 && !(eig_floor > 0.0 && eig_floor < 1.0)) return fail(h, NBLS_ERR_ARG, "nbls_set_capon_music: the eigenvalue floor must lie in (0, 1)");
    if (!(peak_floor >= 0.0 && peak_floor < 1.0)) return fail(h, NBLS_ERR_ARG, "nbls_set_capon_music: the peak floor must lie in [0, 1)");
    if (flags & ~(NBLS_MUSIC_MAP | NBLS_MUSIC_VECTORS | NBLS_MUSIC_PEAKS)) return fail(h, NBLS_ERR_ARG, "nbls_set_capon_music: unknown flags");
    nbls_requests::capon_music_request& r = h->want.music;         // consumed by the NEXT nbls_plan; an existing plan keeps what it was made with
    r.sources = sources;
    r.eig_floor = sources == 0 ? eig_floor : 0.0;
    r.peak_floor = peak_floor;
    r.flags = flags;
    return NBLS_OK;
}

// what the MUSIC fetches share beyond capon_fetch_ready: the plan asked
static int music_fetch_ready(nbls_handle* h, const char* who) {
    int rc;
    if ((rc = capon_fetch_ready(h, who))) return rc;
    if (h->req.music.sources < 0 || !h->d_music_eig) return fail(h, NBLS_ERR_STATE, std::string(who) + ": the plan did not ask for the eigenvalues (nbls_set_capon_music before nbls_plan)");
    return 0;
}

int nbls_fetch_capon_music(nbls_handle* h, double* eigenvalues, int32_t* sources, int32_t* sweeps, int32_t* index, double* power) {
    if (!h) return NBLS_ERR_ARG;
    int rc;
    if ((rc = music_fetch_ready(h, "nbls_fetch_capon_music")) || (rc = finish_pass(h))) return rc;
    const size_t cells = (size_t)h->nbands * h->vector_len;
    if ((rc = fetch_plane(h, h->solve_ran, eigenvalues, h->d_music_eig.p, (size_t)h->nelem * sizeof(double)))) return rc;
    if ((rc = fetch_plane(h, h->solve_ran, sources, h->d_music_int.p, sizeof(int32_t)))) return rc;
    if ((rc = fetch_plane(h, h->solve_ran, sweeps, h->d_music_int.p + cells, sizeof(int32_t)))) return rc;
    if ((rc = fetch_plane(h, h->solve_ran, index, h->d_music_int.p + 2 * cells, sizeof(int32_t)))) return rc;
    return fetch_plane(h, h->solve_ran, power, h->d_music_power.p, sizeof(double));
}

int nbls_fetch_capon_music_map(nbls_handle* h, double* map) {
    if (!h || !map) return NBLS_ERR_ARG;
    int rc;
    if ((rc = music_fetch_ready(h, "nbls_fetch_capon_music_map"))) return rc;
    if (!(h->req.music.flags & NBLS_MUSIC_MAP) || !h->d_music_map)
        return fail(h, NBLS_ERR_STATE, "nbls_fetch_capon_music_map: the plan did not ask for the map (nbls_set_capon_music, NBLS_MUSIC_MAP)");
    if ((rc = finish_pass(h))) return rc;
    return fetch_plane(h, h->solve_ran, map, h->d_music_map.p, (size_t)h->derived.capon_n * sizeof(double));
}

int nbls_fetch_capon_music_vectors(nbls_handle* h, double* E) {
    if (!h || !E) return NBLS_ERR_ARG;
    int rc;
    if ((rc = music_fetch_ready(h, "nbls_fetch_capon_music_vectors"))) return rc;
    if (!(h->req.music.flags & NBLS_MUSIC_VECTORS) || !h->d_music_vec)
        return fail(h, NBLS_ERR_STATE, "nbls_fetch_capon_music_vectors: the plan did not ask for the eigenvectors (nbls_set_capon_music, NBLS_MUSIC_VECTORS)");
    if ((rc = finish_pass(h))) return rc;
    return fetch_plane(h, h->solve_ran, E, h->d_music_vec.p, (size_t)h->nelem * h->nelem * 2 * sizeof(double));
}

int nbls_fetch_capon_music_peaks(nbls_handle* h, int32_t* count, int32_t* index, double* power, double* offset) {
    if (!h) return NBLS_ERR_ARG;
    int rc;
    if ((rc = music_fetch_ready(h, "nbls_fetch_capon_music_peaks"))) return rc;
    if (!(h->req.music.flags & NBLS_MUSIC_PEAKS) || h->req.peaks.k < 1 || !h->d_music_peak_count)
        return fail(h, NBLS_ERR_STATE, "nbls_fetch_capon_music_peaks: the plan did not ask for the peaks (nbls_set_capon_music, NBLS_MUSIC_PEAKS)");
    if ((rc = finish_pass(h))) return rc;
    const size_t K = (size_t)h->req.peaks.k;
    if ((rc = fetch_plane(h, h->solve_ran, count, h->d_music_peak_count.p, sizeof(int32_t)))) return rc;
    if ((rc = fetch_plane(h, h->solve_ran, index, h->d_music_peak_index.p, K * sizeof(int32_t)))) return rc;
    if ((rc = fetch_plane(h, h->solve_ran, power, h->d_music_peak_power.p, K * sizeof(double)))) return rc;
    return fetch_plane(h, h->solve_ran, offset, h->d_music_peak_offset.p, K * 2 * sizeof(double));
}

int nbls_capon_music_lds_bytes(int32_t nelem) {
    if (nelem < 3 || nelem > NBLS_CAPON_MAX_ELEMENTS) return NBLS_ERR_ARG;
    return (int)nbls_capon_music_lds_bytes_of(nelem);
}

int nbls_fetch_capon_tables(nbls_handle* h, int32_t band, double* coef, double* steer) {
    if (!h) return NBLS_ERR_ARG;
    if (!h->planned) return fail(h, NBLS_ERR_STATE, "nbls_fetch_capon_tables: no plan");
    if (h->derived.capon_n < 1) return fail(h, NBLS_ERR_STATE, "nbls_fetch_capon_tables: nbls_set_capon before nbls_plan");
    if (band < 0 || band >= h->fbands) return fail(h, NBLS_ERR_ARG, "nbls_fetch_capon_tables: no such band");
    const int G = h->derived.capon_n, N = h->nelem;                      // the plan's own tables (the device holds copies)
    if (coef) memcpy(coef, h->h_capon_coef.data() + (size_t)band * h->derived.capon_maxls * 2, (size_t)h->h_capon_par[3 * band] * 2 * sizeof(double));
    if (steer) {
        const double* s = h->h_capon_steer.data() + (size_t)band * N * G * 2;
        for (int g = 0; g < G; ++g)
            for (int i = 0; i < N; ++i) {
                steer[((size_t)g * N + i) * 2] = s[((size_t)i * G + g) * 2];
                steer[((size_t)g * N + i) * 2 + 1] = s[((size_t)i * G + g) * 2 + 1];
            }
    }
    return NBLS_OK;
}

int nbls_set_beam_interpolation(nbls_handle* h, int32_t taps) {
    if (!h) return NBLS_ERR_ARG;
    if (taps != 0 && taps != 4 && taps != 6 && taps != 8)
        return fail(h, NBLS_ERR_ARG, "nbls_set_beam_interpolation: taps must be 0 (off), 4, 6 or 8");
    h->want.steer_taps = taps;               // consumed by the NEXT nbls_plan; an existing plan keeps what it was made with
    return NBLS_OK;
}

int nbls_fetch_beam_grid_coefficients(nbls_handle* h, double* c) {
    if (!h || !c) return NBLS_ERR_ARG;
    if (!h->planned) return fail(h, NBLS_ERR_STATE, "nbls_fetch_beam_grid_coefficients: no plan");
    if (h->derived.grid_n < 1 || !h->req.grid_taps())
        return fail(h, NBLS_ERR_STATE, "nbls_fetch_beam_grid_coefficients: nbls_set_beam_grid and nbls_set_beam_interpolation before nbls_plan");
    memcpy(c, h->derived.grid_coef.data(), h->derived.grid_coef.size() * sizeof(double));   // the plan's own table (the device holds a copy)
    return NBLS_OK;
}

int nbls_set_lag_refinement(nbls_handle* h, int32_t on) {
    if (!h) return NBLS_ERR_ARG;
    h->want.refine = on != 0;                // consumed by the NEXT nbls_plan; an existing plan keeps what it was made with
    return NBLS_OK;
}

int nbls_set_lag_limits(nbls_handle* h, const int32_t* max_lag, int32_t npairs) {
    if (!h) return NBLS_ERR_ARG;
    if (!max_lag) { h->want.lim.clear(); return NBLS_OK; }      // off: the next plan searches every lag
    if (npairs < 1) return fail(h, NBLS_ERR_ARG, "nbls_set_lag_limits: npairs must be at least 1");
    for (int32_t k = 0; k < npairs; ++k)                         // everything is checked before the handle changes
        if (max_lag[k] < 0) return fail(h, NBLS_ERR_ARG, "nbls_set_lag_limits: negative limit of pair " + std::to_string(k));
    h->want.lim.assign(max_lag, max_lag + npairs);               // consumed by the NEXT nbls_plan; an existing plan keeps what it was made with
    return NBLS_OK;
}

int nbls_set_lag_seed(nbls_handle* h, const int32_t* halfwidth, int32_t nbands) {
    if (!h) return NBLS_ERR_ARG;
    if (!halfwidth) { h->want.seed.clear(); return NBLS_OK; }   // off: the next plan does not seed its lag search
    if (nbands < 1) return fail(h, NBLS_ERR_ARG, "nbls_set_lag_seed: nbands must be at least 1");
    for (int32_t b = 0; b < nbands; ++b)
        if (halfwidth[b] < 0) return fail(h, NBLS_ERR_ARG, "nbls_set_lag_seed: negative half-width of band " + std::to_string(b));
    h->want.seed.assign(halfwidth, halfwidth + nbands);         // consumed by the NEXT nbls_plan; an existing plan keeps what it was made with
    return NBLS_OK;
}

int nbls_lag_seed_form(int32_t nelem, int32_t W, int32_t max_halfwidth, int32_t halo) {
    if (nelem < 3 || nelem > 32 || W < 2 || max_halfwidth < 0 || halo < 0) return NBLS_ERR_ARG;
    return nbls_lag_seed_form_of(nelem, W);        // (the staged form has no padding: neither enters the fit)
}

int nbls_lag_limit_form(int32_t nelem, int32_t W, int32_t min_limit) {
    if (nelem < 3 || nelem > 32 || W < 2 || min_limit < 0) return NBLS_ERR_ARG;
    return nbls_lag_limit_form_of(nelem, W, min_limit);
}

int nbls_refine_lds_bytes(int32_t nelem, int32_t W) {
    if (nelem < 1 || W < 1) return NBLS_ERR_ARG;
    return (int)nbls_refine_lds_bytes_of(nelem, W);
}

int nbls_fetch_lag_fraction(nbls_handle* h, double* frac) { return nbls_est_fetch_lag_fraction(h, 0, frac); }

int nbls_est_fetch_lag_fraction(nbls_handle* h, int32_t est, double* frac) {
    if (!h || !frac) return NBLS_ERR_ARG;
    if (!h->planned) return fail(h, NBLS_ERR_STATE, "nbls_fetch_lag_fraction: no plan");
    if (est < 0 || est > h->nest) return fail(h, NBLS_ERR_ARG, "nbls_est_fetch_lag_fraction: no such estimator");
    const nbls_estimator& s = h->est[est];
    const nbls_est_view v = nbls_view_of(h, s);
    if (!h->req.refine || !v.frac) return fail(h, NBLS_ERR_STATE, "nbls_fetch_lag_fraction: nbls_set_lag_refinement before nbls_plan");
    { const int rc = finish_pass(h); if (rc) return rc; }
    const size_t cells = (size_t)h->nbands * h->vector_len, P = (size_t)s.npairs;
    // the fractions are written by the correlation stage alone (a sub-array's compact rows: gathered as part of its solve):
    // zeros until a pass of this plan has run it, and a later pass without it leaves them as they are
    const bool have = h->xcorr_ran && (s.kept_pair.empty() || h->solve_ran);
    if (!have) { memset(frac, 0, cells * P * sizeof(double)); return NBLS_OK; }
    HIPCHK(h, copy_sync(h, frac, v.frac, cells * P * sizeof(double), hipMemcpyDeviceToHost));
    zero_uncomputed(h, frac, P * sizeof(double));
    return NBLS_OK;
}

int nbls_fetch_filtered(nbls_handle* h, int32_t band, double* out) {
    if (!h || !out) return NBLS_ERR_ARG;
    if (!h->planned) return fail(h, NBLS_ERR_STATE, "nbls_fetch_filtered: no plan");
    if (band < 0 || band >= h->fbands) return fail(h, NBLS_ERR_ARG, "nbls_fetch_filtered: band out of range");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy2DAsync(out, h->npts * sizeof(double),
                               h->d_filt + (size_t)band * h->nchans * h->npts_pad, h->npts_pad * sizeof(double),
                               h->npts * sizeof(double), h->nchans, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return NBLS_OK;
}

int nbls_set_filtered(nbls_handle* h, int32_t band, const double* data) {
    if (!h || !data) return NBLS_ERR_ARG;
    if (!h->planned) return fail(h, NBLS_ERR_STATE, "nbls_set_filtered: no plan");
    if (band < 0 || band >= h->fbands) return fail(h, NBLS_ERR_ARG, "nbls_set_filtered: band out of range");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpy2DAsync(h->d_filt + (size_t)band * h->nchans * h->npts_pad, h->npts_pad * sizeof(double), data,
                               h->npts * sizeof(double), h->npts * sizeof(double), h->nchans, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return NBLS_OK;
}

int nbls_filter_segment(nbls_handle* h, int32_t reverse, const double* state_in, double* state_out) {
    if (!h) return NBLS_ERR_ARG;
    if (!h->planned) return fail(h, NBLS_ERR_STATE, "nbls_filter_segment: no plan");
    if (h->nsections < 1) return fail(h, NBLS_ERR_ARG, "nbls_filter_segment: the plan has no filter sections");
    if (state_out && (h->npts % NBLS_FILTER_CHUNK) != 0 && !reverse)
        return fail(h, NBLS_ERR_ARG, "nbls_filter_segment: a segment whose end state is wanted must be a whole number of 512-sample chunks");
    if (reverse && state_in && (h->npts % NBLS_FILTER_CHUNK) != 0)
        return fail(h, NBLS_ERR_ARG, "nbls_filter_segment: a backward segment that continues a state must be a whole number of 512-sample chunks");
    HIPCHK(h, hipSetDevice(h->device));
    wait_uploads(h);
    h->work_queued = true;
    const size_t n = (size_t)h->fbands * h->nchans * 2 * h->nsections;
    int rc;
    if ((rc = ensure(h, h->d_seg_state, 2 * n * sizeof(double)))) return rc;
    double* d_init = nullptr;
    double* d_fin = state_out ? h->d_seg_state + n : nullptr;
    if (state_in) {
        d_init = h->d_seg_state;
        HIPCHK(h, hipMemcpyAsync(d_init, state_in, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    HIPCHK(h, nbls_launch_filter_segment(h, reverse ? 1 : 0, d_init, d_fin));
    if (state_out) HIPCHK(h, hipMemcpyAsync(state_out, d_fin, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return NBLS_OK;
}

int nbls_device_results(nbls_handle* h, void** ptrs, int64_t* bytes_per_grid) {
    if (!h || !ptrs) return NBLS_ERR_ARG;
    if (!h->planned) return fail(h, NBLS_ERR_STATE, "nbls_device_results: no plan");
    const nbls_est_view v = nbls_view_of(h, h->est[0]);
    ptrs[0] = v.vel; ptrs[1] = v.baz; ptrs[2] = v.mdccm; ptrs[3] = v.sig; ptrs[4] = h->d_nwin;
    if (bytes_per_grid) *bytes_per_grid = (int64_t)h->nbands * h->vector_len * (int64_t)sizeof(double);
    return NBLS_OK;
}

int nbls_result_layout(nbls_handle* h, int64_t* out4) { return nbls_est_result_layout(h, 0, out4); }

int nbls_est_result_layout(nbls_handle* h, int32_t est, int64_t* out4) {
    if (!h || !out4) return NBLS_ERR_ARG;
    if (!h->planned) return fail(h, NBLS_ERR_STATE, "nbls_result_layout: no plan");
    if (est < 0 || est > h->nest) return fail(h, NBLS_ERR_ARG, "nbls_est_result_layout: no such estimator");
    out4[0] = (int64_t)h->nbands * h->vector_len;
    out4[1] = h->est[est].mask_bytes;
    out4[2] = (int64_t)h->est[est].res_bytes;
    out4[3] = (int64_t)(4 * sizeof(double)) * out4[0];      // byte offset of the mask
    return NBLS_OK;
}

int nbls_fetch_packed(nbls_handle* h, void* out, int64_t nbytes) { return nbls_est_fetch_packed(h, 0, out, nbytes); }

int nbls_est_fetch_packed(nbls_handle* h, int32_t est, void* out, int64_t nbytes) {
    if (!h || !out) return NBLS_ERR_ARG;
    if (!h->planned) return fail(h, NBLS_ERR_STATE, "nbls_fetch_packed: no plan");
    if (est < 0 || est > h->nest) return fail(h, NBLS_ERR_ARG, "nbls_est_fetch_packed: no such estimator");
    const unsigned char* dres = h->est[est].d_res;
    const size_t rbytes = h->est[est].res_bytes;
    if (nbytes != (int64_t)rbytes) return fail(h, NBLS_ERR_ARG, "nbls_fetch_packed: size does not match nbls_result_layout");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(out, dres, rbytes, hipMemcpyDeviceToHost, h->stream));   // ordered after the pass
    return finish_pass(h);
}

int nbls_load_result_block(nbls_handle* h, const void* block, int64_t nbytes) {
    // the block a rank assembled on the host from several HBM rounds (nbls_fetch_packed per round) goes back into the
    // handle's result block, where nbls_comm_gather sends from
    if (!h || !block || nbytes < 0) return NBLS_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    const size_t need = std::max((size_t)nbytes + 8, h->reserve_res);
    int rc;
    nbls_estimator& x = h->est[0];
    if ((rc = ensure(h, x.d_res, need))) return rc;
    HIPCHK(h, hipMemsetAsync(x.d_res, 0, x.d_res.cap, h->stream));
    HIPCHK(h, hipMemcpyAsync(x.d_res, block, (size_t)nbytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));              // the host buffer may go away
    x.res_bytes = (size_t)nbytes;
    h->planned = false;                                      // the last plan no longer describes the block: a new pass needs a new plan
    h->res_loaded = true;                                    // (nbls_comm_gather: this block is a result, whatever its allocation's size)
    return NBLS_OK;
}

int nbls_set_option(nbls_handle* h, const char* key, int64_t value) {
    if (!h || !key) return NBLS_ERR_ARG;
    struct Key { const char* name; int nbls_options::*field; bool developer; };
    static const Key keys[] = {
        {"lts_impl", &nbls_options::lts_impl, false},
        {"lts_generic_h", &nbls_options::lts_generic_h, false},
        {"lts_coop_threads", &nbls_options::lts_coop_threads, false},
        {"lts_sample_its", &nbls_options::lts_sample_its, false},
        {"screen_nsl1", &nbls_options::screen_nsl1, false},
        {"screen_static", &nbls_options::screen_static, false},
        {"screen_tb4", &nbls_options::screen_tb4, false},
        {"screen_pretest", &nbls_options::screen_pretest, false},
        {"screen_tb8", &nbls_options::screen_tb8, false},
        {"screen_cxx", &nbls_options::screen_cxx, false},
        {"screen_nc4", &nbls_options::screen_nc4, false},
        {"screen_batch_mb", &nbls_options::screen_batch_mb, false},
        {"overlap", &nbls_options::overlap, false},
        {"solve_min_units", &nbls_options::solve_min_units, false},
        {"result_tail_units", &nbls_options::result_tail_units, false},
        {"filter_row_step", &nbls_options::filter_row_step, false},
        {"filter_nofuse", &nbls_options::filter_nofuse, false},
        {"filter_nomfma", &nbls_options::filter_nomfma, false},
        {"capon_peak_route", &nbls_options::capon_peak_route, false},
        {"capon_peak_slabs", &nbls_options::capon_peak_slabs, false},
        {"element_delay_form", &nbls_options::element_delay_form, false},
        {"element_delay_chunk", &nbls_options::element_delay_chunk, false},
        {"ablate", &nbls_options::ablate, true},
        {"screen_stamps", &nbls_options::screen_stamps, true},
        {"screen_seed", &nbls_options::screen_seed, true},
        {"lts_stamps", &nbls_options::lts_stamps, true},
        {"screen_pad_kb", &nbls_options::screen_pad_kb, true},
        {"lts_pad_kb", &nbls_options::lts_pad_kb, true},
        {"plan_timing", &nbls_options::plan_timing, true},
    };
    if (strcmp(key, "stream_priority") == 0) {
        // 0 normal, > 0 lower, < 0 higher (clamped to what the device offers).  Several handles of one GPU running
        // passes side by side (the band groups of a pipelined call): the pass whose results the host wants first
        // gets its workgroups dispatched first.  The handle must be idle; results do not depend on it.
        HIPCHK(h, hipSetDevice(h->device));
        int least = 0, greatest = 0;
        HIPCHK(h, hipDeviceGetStreamPriorityRange(&least, &greatest));       // numerically: greatest <= least
        int prio = (int)value;
        if (prio < greatest) prio = greatest;
        if (prio > least) prio = least;
        if (prio == h->stream_priority) return NBLS_OK;
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (h->stream2) HIPCHK(h, hipStreamSynchronize(h->stream2));
        hipStream_t s1 = nullptr, s2 = nullptr;
        HIPCHK(h, hipStreamCreateWithPriority(&s1, hipStreamNonBlocking, prio));
        if (hipStreamCreateWithPriority(&s2, hipStreamNonBlocking, prio) != hipSuccess) s2 = nullptr;
        if (h->stream2) (void)hipStreamDestroy(h->stream2);
        if (h->up == h->stream) h->up = s1;
        (void)hipStreamDestroy(h->stream);
        h->stream = s1;
        h->stream2 = s2;
        h->stream_priority = prio;
        return NBLS_OK;
    }
    for (const Key& k : keys) {
        if (strcmp(k.name, key) != 0) continue;
#ifndef NBLS_DEVELOPER
        if (k.developer) return fail(h, NBLS_ERR_UNSUPPORTED, std::string("option '") + key + "' exists only in the developer build (make dev)");
#endif
        if (k.field == &nbls_options::capon_peak_route && (value < 0 || value > 2))
            return fail(h, NBLS_ERR_ARG, "option 'capon_peak_route' is 0 (automatic), 1 (LDS) or 2 (HBM)");
        if (k.field == &nbls_options::capon_peak_slabs && (value < 0 || value > 4096))
            return fail(h, NBLS_ERR_ARG, "option 'capon_peak_slabs' is 1..4096 (0: the default)");
        if (k.field == &nbls_options::element_delay_form && (value < 0 || value > 2))
            return fail(h, NBLS_ERR_ARG, "option 'element_delay_form' is 0 (automatic), 1 (staged in LDS) or 2 (global memory)");
        if (k.field == &nbls_options::element_delay_chunk && value != 0 && value != 1 && value != 4)
            return fail(h, NBLS_ERR_ARG, "option 'element_delay_chunk' is 0 (the default), 1 or 4 shifts per wave and item");
        h->opt.*(k.field) = (int)value;
        h->planned = false;                 // options are read by nbls_plan and by the launchers of the next pass
        return NBLS_OK;
    }
    return fail(h, NBLS_ERR_ARG, std::string("unknown option '") + key + "'");
}

int nbls_developer_build(void) {
#ifdef NBLS_DEVELOPER
    return 1;
#else
    return 0;
#endif
}

int nbls_set_profiling(nbls_handle* h, int32_t on) {
    if (!h) return NBLS_ERR_ARG;
    h->prof = on != 0;
    return NBLS_OK;
}

int nbls_get_timings(nbls_handle* h, nbls_timings* out) {
    if (!h || !out) return NBLS_ERR_ARG;
    *out = h->tim;
    return NBLS_OK;
}

int nbls_run(nbls_handle* h, int32_t nbands, const double* sos, int32_t nsections, int32_t zero_phase,
             const double* taper_left, const double* taper_right, int32_t taper_len, const int32_t* winlen,
             const int32_t* wininc, int32_t vector_len, const nbls_lts_params* lts, int32_t xcorr_impl,
             double* vel, double* baz, double* mdccm, double* sigma_tau, int32_t* nwin, int32_t* lag,
             double* cmax, uint8_t* weights, double* z) {
    int rc = nbls_plan(h, nbands, sos, nsections, zero_phase, taper_left, taper_right, taper_len, winlen,
                       wininc, vector_len, lts, xcorr_impl);
    if (rc) return rc;
    if ((rc = nbls_execute(h))) return rc;
    if ((rc = nbls_sync(h))) return rc;
    return nbls_fetch(h, vel, baz, mdccm, sigma_tau, nwin, lag, cmax, weights, z);
}

int nbls_probe_mfma_f64(nbls_handle* h, const double* a, const double* b, double* out) {
    if (!h || !a || !b || !out) return NBLS_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    double *da = nullptr, *db = nullptr, *dout = nullptr;
    HIPCHK(h, hipMalloc((void**)&da, 64 * sizeof(double)));
    HIPCHK(h, hipMalloc((void**)&db, 64 * sizeof(double)));
    HIPCHK(h, hipMalloc((void**)&dout, 256 * sizeof(double)));
    HIPCHK(h, copy_sync(h, da, a, 64 * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(h, copy_sync(h, db, b, 64 * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(h, nbls_launch_probe_mfma(h, da, db, dout));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, copy_sync(h, out, dout, 256 * sizeof(double), hipMemcpyDeviceToHost));
    (void)hipFree(da); (void)hipFree(db); (void)hipFree(dout);
    return NBLS_OK;
}

// The candidate records the screening kernel left for the last unit batch, [units][N][N][32] int32 (layout: CHDR in
// xcorr_screen.hip), copied to `out`; -> the number of units.  Shared by the two developer read-outs below.
static int screen_records_copy(nbls_handle* h, int32_t* out, int64_t capacity, int64_t* units) {
    if (!h->d_cand || h->screen_batch <= 0) return fail(h, NBLS_ERR_STATE, "no screening run yet");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const int N = h->nelem;
    const int64_t last = h->last_batch > 0 ? h->last_batch : h->nunits - ((h->nunits - 1) / h->screen_batch) * h->screen_batch;
    *units = last;
    if (!out) return NBLS_OK;
    const int64_t n = last * N * N * 32;
    if (capacity < n) return fail(h, NBLS_ERR_ARG, "candidate records: the buffer is too small");
    HIPCHK(h, copy_sync(h, out, h->d_cand, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return NBLS_OK;
}

int nbls_debug_screen_records(nbls_handle* h, int32_t* out, int64_t capacity, int64_t* units) {
    if (!h || !units || capacity < 0) return NBLS_ERR_ARG;
    return screen_records_copy(h, out, capacity, units);
}

int nbls_debug_screen_stats(nbls_handle* h, int64_t* out4) {
    // out4 = {ordered pairs in the last batch, pairs whose candidate buffer overflowed,
    //         total candidates, max candidates}  (developer statistic of the int8 screening path)
    if (!h || !out4) return NBLS_ERR_ARG;
    const int N = h->nelem;
    int64_t last = 0;
    int rc = screen_records_copy(h, nullptr, 0, &last);
    if (rc) return rc;
    std::vector<int32_t> c((size_t)last * N * N * 32);
    if ((rc = screen_records_copy(h, c.data(), (int64_t)c.size(), &last))) return rc;
    for (int q = 0; q < 8; ++q) out4[q] = 0;
    for (int64_t u = 0; u < last; ++u)
        for (int i = 0; i < N; ++i)
            for (int j = 0; j < N; ++j) {
                if (i == j) continue;
                const int32_t* e = &c[((u * N + i) * N + j) * 32];
                out4[0] += 1;
                out4[1] += e[1] != 0;          // interval and/or list overflow
                out4[2] += e[0];
                if (e[0] > out4[3]) out4[3] = e[0];
                // how the listed lags cluster (developer: what a verifier that shares loads between adjacent lags could use)
                int n = e[0] < 26 ? e[0] : 26;
                int v[26];
                for (int q = 0; q < n; ++q) v[q] = e[6 + q];
                std::sort(v, v + n);
                for (int q = 0; q < n; ) {
                    int r = q + 1;
                    while (r < n && v[r] == v[r - 1] + 1) ++r;
                    out4[4] += 1;                       // runs of consecutive lags
                    if (r - q >= 2) out4[5] += r - q;   // listed lags that sit in a run of two or more
                    q = r;
                }
            }
    return NBLS_OK;
}

int nbls_debug_screen_stamps(nbls_handle* h, double* out6) {
    // mean cycle counts of the screen kernel's phases over the workgroups of the last batch:
    // out[10] = {stage issue, stage barrier wait, compute (wave 0), wait for the other waves, merge+write, total,
    //            wave 0: cycles inside the K loops, in the epilogues, of those: conversion + maximum, shared-maximum round trip}
    if (!h || !out6) return NBLS_ERR_ARG;
    if (!h->d_stamps) return fail(h, NBLS_ERR_STATE, "run with NBLS_SCREEN_STAMPS=1");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const int64_t last = h->last_batch > 0 ? h->last_batch : h->nunits - ((h->nunits - 1) / h->screen_batch) * h->screen_batch;
    const int64_t nwg = ((last + 7) / 8) * 8 * h->nelem;   // upper bound (one or two channels per workgroup)
    std::vector<unsigned long long> st((size_t)nwg * 8);
    HIPCHK(h, copy_sync(h, st.data(), h->d_stamps, st.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int i = 0; i < 10; ++i) out6[i] = 0.0;
    int64_t cnt = 0;
    for (int64_t g = 0; g < nwg; ++g) {
        const unsigned long long* s = &st[(size_t)g * 8];
        if (s[5] <= s[0] || s[5] - s[0] > 100000000ull) continue;
        for (int i = 0; i < 5; ++i) out6[i] += (double)(s[i + 1] - s[i]);
        out6[5] += (double)(s[5] - s[0]);
        out6[6] += (double)(s[6] & 0xffffffffull);    // wave 0: cycles inside the K loops | in the epilogues
        out6[7] += (double)(s[6] >> 32);
        out6[8] += (double)(s[7] & 0xffffffffull);    // of the epilogues: conversion + maximum | shared-maximum round trip
        out6[9] += (double)(s[7] >> 32);
        ++cnt;
    }
    for (int i = 0; i < 10; ++i) out6[i] /= (double)(cnt > 0 ? cnt : 1);
    return NBLS_OK;
}

int nbls_debug_lts_stamps(nbls_handle* h, double* out8) {
    if (!h || !out8) return NBLS_ERR_ARG;
    if (!h->d_stamps || h->lts_stamp_waves <= 0) return fail(h, NBLS_ERR_STATE, "run with NBLS_SCREEN_STAMPS=1 NBLS_LTS_STAMPS=1");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::vector<unsigned long long> st((size_t)h->lts_stamp_waves * 8);
    HIPCHK(h, copy_sync(h, st.data(), h->d_stamps, st.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int i = 0; i < 8; ++i) out8[i] = 0.0;
    int64_t cnt = 0;
    for (int64_t g = 0; g < h->lts_stamp_waves; ++g) {
        const unsigned long long* s = &st[(size_t)g * 8];
        if (s[6] <= s[0] || s[6] - s[0] > 1000000000ull) continue;
        for (int i = 0; i < 6; ++i) out8[i] += (double)(s[i + 1] - s[i]);
        out8[7] += (double)(s[6] - s[0]);
        out8[6] += (double)s[7];              // finished entries entering the candidate peel
        ++cnt;
    }
    for (int i = 0; i < 8; ++i) out8[i] /= (double)(cnt > 0 ? cnt : 1);
    return NBLS_OK;
}

int nbls_debug_lts_coop_breakdown(nbls_handle* h, double* out8) {
    // developer: mean over the units of the large-array LTS kernel's C-step phases, thread 0's cycles in
    // {groups (selection + sums), subset merging, compaction}, the live entries summed over the iterations, and
    // wave 0's {selection passes, selection cycles, sums cycles, groups}
    if (!h || !out8) return NBLS_ERR_ARG;
    if (!h->d_stamps || h->lts_stamp_waves <= 0) return fail(h, NBLS_ERR_STATE, "developer build with option lts_stamps needed");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::vector<unsigned long long> st((size_t)h->lts_stamp_waves * 8);
    HIPCHK(h, copy_sync(h, st.data(), h->d_stamps + (size_t)h->lts_stamp_waves * 8, st.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int i = 0; i < 8; ++i) out8[i] = 0.0;
    for (int64_t g = 0; g < h->lts_stamp_waves; ++g)
        for (int i = 0; i < 8; ++i) out8[i] += (double)st[(size_t)g * 8 + i];
    for (int i = 0; i < 8; ++i) out8[i] /= (double)h->lts_stamp_waves;
    return NBLS_OK;
}

int nbls_probe_mfma_i8(nbls_handle* h, const int32_t* a, const int32_t* b, int32_t* out) {
    if (!h || !a || !b || !out) return NBLS_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    int *da = nullptr, *db = nullptr, *dout = nullptr;
    HIPCHK(h, hipMalloc((void**)&da, 256 * sizeof(int)));
    HIPCHK(h, hipMalloc((void**)&db, 256 * sizeof(int)));
    HIPCHK(h, hipMalloc((void**)&dout, 256 * sizeof(int)));
    HIPCHK(h, copy_sync(h, da, a, 256 * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(h, copy_sync(h, db, b, 256 * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(h, nbls_launch_probe_mfma_i8(h, da, db, dout));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, copy_sync(h, out, dout, 256 * sizeof(int), hipMemcpyDeviceToHost));
    (void)hipFree(da); (void)hipFree(db); (void)hipFree(dout);
    return NBLS_OK;
}

}  // extern "C"
