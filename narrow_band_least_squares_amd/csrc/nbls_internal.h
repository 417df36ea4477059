// Internal declarations shared by the translation units of libnbls_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <mutex>
#include <string>
#include <vector>
#include "../../include/nbls.h"
#include "dev_buf.h"

#define NBLS_MAX_SECTIONS 8
#define NBLS_FILTER_CHUNK 512      // samples per scan chunk (one lane each)
#define NBLS_FILTER_TILE 16        // samples per LDS tile row
#define NBLS_FILTER_GROUP 64       // chunks per carry group
#define NBLS_MAX_PAIRS 512
#define NBLS_MAX_STARTS 1024
#define NBLS_MAX_CAND 16
// Static LDS of the correlation-stage kernels (bytes, = .amdhsa_group_segment_fixed_size of each; the kernels
// static_assert their __shared__ arrays against these): nbls_route_compute adds them to the dynamic part.  The kernels
// not named here have none.
#define NBLS_SLDS_XCORR_SIMPLE 80     // xcorr_simple_kernel: red_v[8] doubles + red_k[4] ints
#define NBLS_SLDS_VERIFY 16640        // verify_kernel: vscr[4][VRUN_SCR] doubles
#define NBLS_SCREEN_TB 4              // tile steps of the four-tile screening instances (the copy stride is sized for them)

// Per-handle switches (nbls_set_option).  The first group selects between implementations that give
// IDENTICAL results (A/B timing, tests that compare kernels with each other).  The second group exists only
// in a -DNBLS_DEVELOPER build (`make dev`): in-kernel time stamps and ablation switches that make results
// WRONG on purpose; the shipped library has none of that code in its kernels.
struct nbls_options {
    int lts_impl = 0;          // 0 auto; 1 lane-per-start generic LTS kernel everywhere; 3 generic only where no register kernel exists
    int lts_generic_h = 0;     // 1: the register LTS kernel without the h-specialised instantiation
    int lts_coop_threads = 0;  // > 0: workgroup size (64..512) of the large-array LTS kernel (solve_bucket.inc)
    int lts_sample_its = 0;    // large-array LTS kernel: the first n selections of a start take the coarse sample pass (0: all of them, < 0: none)
    int screen_nsl1 = 0;       // 1: one sliding channel per screening workgroup
    int screen_tb4 = 0;        // 1: four-tile lag groups also where the eight-tile instance of the screening kernel applies
    int screen_static = 0;     // 1: fixed (snake-order) deal of the lag groups instead of the dynamic one
    int screen_pretest = 0;    // 1: integer pre-test of a lag group's accumulators before the f32 conversion (epilogue)
    int screen_cxx = 0;        // 1: the compiler-scheduled K loop of the screening kernel everywhere (experiment)
    int screen_nc4 = 0;        // 1: four byte-shifted copies per sliding channel also where eight fit (experiment)
    int screen_tb8 = 0;        // 1: the eight-tile instance wherever one lag block per tile step applies (S == 1)
    int screen_batch_mb = 192;  // quantised-window bytes per unit batch
    int solve_min_units = 0;   // > 0: units a per-batch solve (and a streamed result batch) covers at least (default 8192)
    int filter_row_step = 0;   // > 0: the filter stage runs in launches of at most this many channels even when the whole trace is there
    int result_tail_units = 0; // streamed pass: the LAST result batch is cut to this many units (0: default 2048, < 0: not cut), see xcorr_screen.hip
    int overlap = 0;           // solve of batch k on a second stream while batch k+1 is correlated: 1 on, -1 off, 0 auto (streamed passes of several small batches)
    int filter_nofuse = 0;     // 1: separate state kernel for the backward filter pass
    int filter_nomfma = 0;     // 1: VALU state kernel
    int capon_peak_route = 0;  // where a unit's maps wait for the peak pick (nbls_set_capon_peaks): 0 auto, 1 LDS, 2 HBM
    int capon_peak_slabs = 0;  // HBM route: workgroups per launch, 1..4096 (0: what 256 MiB hold, 256 .. 4096)
    int element_delay_chunk = 0;   // shifts of an element a wave of element_delay_kernel takes together: 0 the default (4), 1 or 4; the same bits
    int element_delay_form = 0;    // where a unit's rows wait for the element delays (nbls_set_element_delays): 0 auto, 1 staged in LDS, 2 global
    // ---- developer build only ----
    int ablate = 0;            // skip parts of the screening / verify kernels (timing; results wrong)
    int screen_stamps = 0;     // s_memtime phase stamps of the screening kernel
    int screen_seed = 0;       // experiment: running maxima of the screening kernel seeded from the previous pass of the same batch
    int lts_stamps = 0;        // ... of the wave-per-unit LTS kernel
    int screen_pad_kb = 0;     // extra LDS per screening workgroup (occupancy experiment)
    int lts_pad_kb = 0;        // extra LDS per LTS workgroup
    int plan_timing = 0;       // print the host phases of nbls_plan
};

// Consecutive bands of one window length: the unit of the correlator choice (nbls_plan / nbls_launch_xcorr).
struct nbls_wgroup {
    int b0, b1, W; int64_t u0, u1; bool screen;
    int bform = 0;     // a plan with lag limits (nbls_set_lag_limits): 0 the ordinary route, 1 / 2 the form of the bounded-lag correlator
    int sform = 0;     // a plan with a lag seed (nbls_set_lag_seed): 1 / 2 the form of the seeded correlator (0: no seed)
};

// One estimator of a pass: the geometry and LTS plan of ONE array (the full one or a sub-array) as the caller described
// them, the device tables nbls_plan makes of them, and the buffers of its own results.  The handle holds 1 + 8 of these
// records: est[0] is the plan's own estimator (nbls_set_geometry, nbls_plan(lts = ...), nbls_set_uncertainty), est[1..nest]
// are the further ones (nbls_set_estimators).  What a record does not store is derived by nbls_view_of below.
// Every device and pinned buffer, here and in the handle, is a dev_buf / pinned_buf (dev_buf.h): it knows its own capacity
// and whether it is a place in the plan arena, and it is freed when the handle is deleted.
struct nbls_estimator {
    std::vector<int32_t> kept;         // element indices, ascending (est[0]: empty, it is the whole array)
    std::vector<int32_t> kept_pair;    // [P']: index of pair k of the sub-array in the full array's pair list (empty: all elements kept)
    int npairs = 0;                    // P'
    std::vector<double> h_xij, h_xpinv;
    bool lts = false;
    nbls_lts_params ltsp{};            // starts / rew_table are NULL here: the tables are the two vectors below
    std::vector<int32_t> h_starts;
    std::vector<double> h_rew;
    bool want_unc = false;             // confidence intervals of the slowness estimate: computed behind the solve when wanted
    double unc_par[6] = {0, 0, 0, 0, 0, 0};   // eigenvalues of X^T X, rotation into the eigen-frame (row major)
    // device side
    dev_buf<double> d_xij;             // [P'][2]
    dev_buf<double> d_xpinv;           // [2][P']
    dev_buf<int32_t> d_starts;         // [S][4]
    dev_buf<double> d_rew;             // [P'+1]
    dev_buf<double> d_xs;              // [P'][2] standardised co-array
    dev_buf<double> d_xc;              // [P'] c0*c1 of the standardised co-array; d_xs and d_xc are padded by 16 pairs (solve_bucket.inc reads one block ahead)
    dev_buf<double> d_xss;             // [ceil(P'/4)][2] every 4th row of d_xs (padded likewise)
    // a sub-array's solve reads compact copies of its pairs' rows (gather_pairs_kernel): its own [B][VL][P'] buffers,
    // filled per unit batch from the handle's through d_kept_pair [P']; a full array reads the handle's d_lag / d_cmax
    dev_buf<int32_t> d_kept_pair;
    dev_buf<int32_t> d_lag;
    dev_buf<double> d_cmax;
    dev_buf<double> d_lagfrac;         // ... and of their sub-sample fractions (a plan with lag refinement)
    dev_buf<double> d_z;               // [B][VL][2]
    dev_buf<uint8_t> d_wts;            // [B][VL][P'] one byte per pair (kernel-side form; packed into the mask after the solve)
    dev_buf<double> d_unc;             // [2][B][VL]: vel_uncert | baz_uncert
    dev_buf<int32_t> d_kept;           // [K] the kept elements' rows (a plan with beam results, est[1..]; est[0] takes every row)
    dev_buf<double> d_beam;            // [2][B][VL]: beam_power | fstat (a plan with beam results, nbls_set_beam)
    dev_buf<double> d_closure;         // [2][B][VL]: consistency | closure_max (a plan with closure results, nbls_set_closure)
    dev_buf<double> d_closure_el;      // [B][VL][N]: element_consistency, N this estimator's element count (likewise)
    // result block, ONE allocation = one D2H copy / one RCCL gather:
    //   [vel | baz | mdccm | sigma_tau] double[4][B][VL], then the LTS weight bit mask uint8[B][VL][MB],
    //   MB = ceil(P'/8), bit k & 7 of byte k >> 3 = weight of pair k (ceil(P/8) bytes per unit)
    dev_buf<unsigned char> d_res;
    pinned_buf h_res;                  // its pinned mirror, filled batch by batch (nbls_stream_results)
    size_t res_bytes = 0;              // the plan's block (d_res.cap may be more: a bigger plan before, nbls_reserve_results)
    int mask_bytes = 0;                // MB
};

#define NBLS_MAX_ESTIMATORS 8      // further estimators of one pass, beside estimator 0

// The opt-in requests of a plan, as the nbls_set_* calls record them.  The handle holds two: `want`, written by the setters
// and read by the next nbls_plan alone, and `req`, the plan's own copy (committed in one assignment once nbls_plan has
// refused nothing), which everything behind the plan's checks reads.  A request that is off is in its default state.
struct nbls_requests {
    bool beam = false;              // nbls_set_beam: beam power and F-statistic behind every estimator's solve (beam.hip)
    bool closure = false;           // nbls_set_closure: closure of the picked lags behind every estimator's solve (closure.hip)
    bool refine = false;            // nbls_set_lag_refinement: sub-sample lags behind the verifier (refine.hip)
    std::vector<int32_t> lim;       // nbls_set_lag_limits: [npairs] max_lag per pair (empty: every lag is searched)
    // nbls_set_lag_seed (xcorr_seeded.hip): [nbands] half-width per band (empty: off).  A plan with a slowness grid then picks
    // every pair's lag near the delay the unit's grid maximum predicts; the grid search belongs to the correlation stage
    std::vector<int32_t> seed;
    std::vector<double> grid;       // nbls_set_beam_grid (beam_grid.hip): [G][2] slowness vectors (empty: off)
    bool grid_keep_map = false;     // ... and whether the plan keeps every F(g)
    int steer_taps = 0;             // nbls_set_beam_interpolation (steer.h): 0 whole samples / 4 / 6 / 8 taps
    // ---- the grid maximum refined between grid points (nbls_set_beam_grid_refinement, beam_grid_refine.hip) ----
    struct grid_refine_request {
        int levels = 0;                 // R (0: off, no grid_refine_kernel is launched)
        double step[2] = {0.0, 0.0};    // (h0, h1) s/km
    } grid_refine;
    // ---- Capon / Bartlett spectra of the narrow band's cross-spectral matrix (nbls_set_capon, capon.hip) ----
    struct capon_request {
        std::vector<double> grid;       // [G][2] slowness vectors (empty: off)
        std::vector<double> freq;       // [nbands] Hz
        std::vector<int32_t> ls, hs;    // [nbands] snapshot length and hop
        double loading = 0.0;
        int flags = 0;
    } capon;
    // ---- the K strongest peaks of either spectrum (nbls_set_capon_peaks, capon.hip) ----
    struct capon_peak_request {
        std::vector<int32_t> nbr;       // [8][G] neighbour table of the request's cells (empty: off)
        int k = 0;                      // K (0: off)
        double floor = 0.0;
    } peaks;
    // ---- the window's arrivals by CLEAN-SC (nbls_set_capon_clean, capon_clean.hip) ----
    struct capon_clean_request {
        int iterations = 0;             // I (0: off, no capon_clean_kernel is launched)
        double gain = 0.0, floor = 0.0;
        int flags = 0;
    } clean;
    // ---- the window's eigenvalues and MUSIC spectrum (nbls_set_capon_music, capon_music.hip) ----
    struct capon_music_request {
        int sources = -1;               // M, 0: by eig_floor, -1: off (no capon_music_kernel is launched)
        double eig_floor = 0.0, peak_floor = 0.0;
        int flags = 0;
    } music;
    // ---- the elements LTS kept (nbls_set_kept_elements, kept.hip) ----
    int kept_q = 0, kept_flags = 0;     // min_pairs (0: off) and NBLS_KEPT_*
    // ---- the beam trace of every result row (nbls_set_beam_trace, beam_trace.hip) ----
    bool bt = false;                // the trace is formed behind the pass's last solve
    std::vector<double> bt_win;     // ... its synthesis windows, band after band
    double bt_min = 0.0;            // ... its MdCCM gate (NaN: off)
    int bt_flags = 0;
    // ---- each element's delay against the beam of the others (nbls_set_element_delays, element_delay.hip) ----
    bool ed = false;                // the delays are measured behind every solve of estimator 0
    std::vector<int32_t> ed_K;      // ... its max_shift, one per band
    int ed_flags = 0;
    // ---- the pass's windows grouped into families (nbls_set_families, families.hip) ----
    bool fam = false;               // the cells are labelled behind the pass's last solve
    nbls_family_params fam_par{};   // ... under this request

    // what the flags resolve to
    bool kept_beam() const { return kept_q > 0 && (kept_flags & NBLS_KEPT_BEAM); }      // the beam is that of the kept elements
    bool kept_capon() const { return kept_q > 0 && (kept_flags & NBLS_KEPT_CAPON); }    // ... and so are the spectra
    bool bt_kept() const { return bt && (bt_flags & NBLS_BEAM_TRACE_KEPT); }            // the trace over the elements LTS kept in each window
    bool ed_kept() const { return ed && (ed_flags & NBLS_ELEMENT_DELAY_KEPT); }         // the delays against the beam of the kept elements
    bool capon_maps() const { return !capon.grid.empty() && (capon.flags & NBLS_CAPON_MAPS); }   // the plan keeps both maps
    bool capon_csdm() const { return !capon.grid.empty() && (capon.flags & NBLS_CAPON_CSDM); }   // ... the matrix R
    bool grid_map() const { return !grid.empty() && grid_keep_map; }
    int grid_taps() const { return grid.empty() ? 0 : steer_taps; }                     // the taps of the grid search (0: none, or whole samples)
    bool grid_refined() const { return grid_refine.levels > 0; }                        // the grid maximum is refined behind the search
};

// What nbls_plan derives from its requests and the trace; valid with `req`.
struct nbls_plan_derived {
    int grid_n = 0, grid_halo = 0;          // G of the slowness grid (0: the plan does not search) and H = max |delay|
    std::vector<int32_t> grid_delay;        // [G][nelem] the delay table (interpolated: floor(tau))
    std::vector<double> grid_coef;          // [G][nelem][taps] the coefficient table of an interpolated grid
    int grid_refine_halo = 0;               // H_r of a plan that refines the grid maximum: the reach of every candidate's taps
    int capon_n = 0;                        // G of the spectra (0: the plan computes none)
    int capon_maxls = 0;                    // the longest snapshot: the row length of h_capon_coef
    int peak_route = 0;                     // a peak request's route: 1 the unit's maps in LDS, 2 in HBM (its rows of d_capon_map, or a slab)
    int peak_slabs = 0;                     // HBM route: slabs of d_capon_peak_slab = workgroups per launch
    size_t ed_lds = 0;                      // dynamic LDS of the staged element-delay form (the largest row's block); 0: the global form
};

// Device side of one labelling of a lattice into families (families.hip): the union-find's parent array, the records the
// roots accumulate, the scan's block sums and the three results.  The handle holds two: the plan's and that of
// nbls_label_families, which also keeps the caller's grids and window tables here.
struct nbls_family_work {
    struct ptrs { int32_t *parent, *count, *band_hi, *peak, *fid; unsigned long long *smin, *smax, *key; int32_t* sums; };
    dev_buf<int32_t> parent, count, band_hi, peak, fid;    // [cells]: root or -1 | members | highest band | peak cell | family id (at the root)
    dev_buf<unsigned long long> smin, smax, key;           // [cells]: min s0 | max s0 + W | image of the largest MdCCM (at the root)
    dev_buf<int32_t> sums;                                 // [ceil(cells / 256)]
    dev_buf<int32_t> family;                               // [cells]
    dev_buf<int64_t> table;                                // [cells / min_pixels][8]
    dev_buf<int32_t> nfam;                                 // [1]
    dev_buf<double> grids;                                 // nbls_label_families: [4][cells] vel | baz | mdccm | sigma_tau
    dev_buf<int32_t> tabs;                                 // ... [3][rows] W | inc | nwin
    hipError_t grow(int64_t ncells, int min_pixels);       // everything but grids and tabs; contents are not kept
};

struct nbls_handle {
    int device = 0;
    nbls_options opt;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;  // solve of batch k runs here while batch k+1 is correlated on `stream`
    hipEvent_t ev_xd = nullptr;        // recorded behind the correlation stage of every pass (nbls_execute_after)
    bool ev_xd_recorded = false;
    hipEvent_t ev_plan = nullptr;      // plan-time uploads wait for this handle's queued kernels (StreamGuard)
    bool ev_xd_by_launcher = false;    // the screening launcher recorded it ahead of its join with the solve stream
    nbls_handle* after = nullptr;      // set for the duration of nbls_execute_after
    int num_cus = 0;                   // compute units of the device (persistent grids)
    hipStream_t up = nullptr;          // plan-time table uploads (highest priority, see alloc_copy)
    int stream_priority = 0;           // nbls_set_option("stream_priority")
    std::vector<hipEvent_t> pev;    // pipeline hand-off events
    bool fuse_solve = false;        // set by nbls_execute_stages: every unit batch of the correlation stage is followed by its solve
    bool solve_on_stream2 = false;  // ... on the second stream (option "overlap"), else behind the batch on `stream`
    bool solve_done = false;
    int last_stage_mask = 7;        // stages of the last pass (nbls_fetch zeroes the outputs of stages that did not run)
    nbls_requests want;             // the nbls_set_* calls write here; read by the next nbls_plan, and by nothing else
    nbls_requests req;              // the plan's requests
    nbls_plan_derived derived;      // ... and what the plan made of them for this trace
    // What a pass of this plan has left in the buffers of the opt-in results, which no pass clears: the solve stage has run
    // (the results written behind a solve, and a sub-array's compact rows, gathered there), the correlation stage has run
    // (d_lagfrac, and the grid search of a plan with a lag seed).  A fetch returns zeros until then, and a later pass
    // without the stage leaves the results as they are.
    bool solve_ran = false, xcorr_ran = false;
    bool grid_ran() const { return req.seed.empty() ? solve_ran : xcorr_ran; }     // the grid search's results are there
    dev_buf<int32_t> d_limsq;       // [nelem][nelem] the plan's limit of the pair of two elements, symmetric, 0 on the diagonal
    dev_buf<int32_t> d_seed;        // [rows] the seed half-width of every result row (row r: band r / nseg)
    bool seed_attr_set = false;     // the staged form of the seeded correlator has been given its dynamic LDS limit
    bool refine_attr_set = false;   // the LDS form of refine_lag_kernel has been given its dynamic LDS limit on this handle's device
    // ---- slowness-grid search of the beam F-statistic (beam_grid.hip) ----
    unsigned grid_attr_set = 0;     // the LDS forms of beam_grid_kernel that have been given their dynamic LDS limit (bit taps / 2)
    dev_buf<double> d_grid;         // [G][2]
    dev_buf<int32_t> d_grid_delay;  // [G][nelem]
    dev_buf<double> d_grid_coef;    // [G][nelem][taps] (an interpolated grid)
    dev_buf<int32_t> d_grid_index;  // [B][VL]
    dev_buf<double> d_grid_fp;      // [2][B][VL]: grid_fstat | grid_power
    dev_buf<double> d_grid_map;     // [B][VL][G] (a plan that asked for the map)
    // ---- the grid maximum refined between grid points (beam_grid_refine.hip) ----
    unsigned grid_refine_attr_set = 0;  // the LDS forms of grid_refine_kernel that have their dynamic LDS limit (bit taps / 2)
    dev_buf<double> d_grid_refine_fp;   // [B][VL][2] slowness | [B][VL] fstat | [B][VL] power | [B][VL][9] stencil
    dev_buf<int32_t> d_grid_refine_path;    // [B][VL][R]
    // ---- Capon / Bartlett spectra (capon.hip) ----
    bool capon_attr_set = false;    // capon_kernel has been given its dynamic LDS limit on this handle's device
    std::vector<int32_t> h_capon_par;   // [fbands][3]: Ls, Hs, K
    std::vector<double> h_capon_coef;   // [fbands][maxLs][2] snapshot coefficients (zeros beyond Ls_b)
    std::vector<double> h_capon_steer;  // [fbands][nelem][G][2] steering vectors, consecutive g side by side
    dev_buf<int32_t> d_capon_par;
    dev_buf<double> d_capon_coef;
    dev_buf<double> d_capon_steer;
    dev_buf<int32_t> d_capon_index; // [2][B][VL]: capon_index | bartlett_index
    dev_buf<double> d_capon_power;  // [2][B][VL]: capon_power | bartlett_power
    dev_buf<double> d_capon_map;    // [2][B][VL][G] (a plan that asked for the maps)
    dev_buf<double> d_capon_csdm;   // [B][VL][N][N][2] (a plan that asked for R)
    // ---- the K strongest peaks of either spectrum (capon.hip) ----
    bool capon_peak_attr_set[2] = {false, false};   // the two instances with peaks have their dynamic LDS limit
    dev_buf<int32_t> d_capon_nbr;           // [8][G]
    dev_buf<double> d_capon_peak_slab;      // [slabs][2][G] (HBM route of a plan without the maps)
    // the slabs belong to one launch at a time.  A pass may solve on two streams (solve_on_stream2: the screened window
    // groups on stream2, a group on a general correlator on stream), so the last launch that used them records this event,
    // and a launch on the other stream waits for it
    hipEvent_t ev_capon_slab = nullptr;
    hipStream_t capon_slab_stream = nullptr;    // where ev_capon_slab was recorded last (nullptr: nowhere yet)
    dev_buf<int32_t> d_capon_peak_count;    // [2][B][VL]: Capon | Bartlett
    dev_buf<int32_t> d_capon_peak_index;    // [2][B][VL][K]
    dev_buf<double> d_capon_peak_power;     // [2][B][VL][K]
    dev_buf<double> d_capon_peak_offset;    // [2][B][VL][K][2]
    // ---- the window's arrivals by CLEAN-SC (capon_clean.hip) ----
    bool clean_attr_set[2] = {false, false};    // the plain and the KEPT instance have their dynamic LDS limit
    dev_buf<int32_t> d_clean_count; // [B][VL]
    dev_buf<int32_t> d_clean_index; // [B][VL][I]
    dev_buf<double> d_clean_power;  // [B][VL][I]
    dev_buf<double> d_clean_tr;     // [2][B][VL]: total | residual
    dev_buf<double> d_clean_csdm;   // [B][VL][N][N][2] (NBLS_CLEAN_RESIDUAL)
    // ---- the window's eigenvalues and MUSIC spectrum (capon_music.hip) ----
    bool music_attr_set[2] = {false, false};    // the plain and the peak instance have their dynamic LDS limit
    dev_buf<double> d_music_eig;    // [B][VL][N]
    dev_buf<int32_t> d_music_int;   // [3][B][VL]: sources | sweeps | index
    dev_buf<double> d_music_power;  // [B][VL]
    dev_buf<double> d_music_map;    // [B][VL][G] (NBLS_MUSIC_MAP)
    dev_buf<double> d_music_vec;    // [B][VL][N][N][2] (NBLS_MUSIC_VECTORS)
    dev_buf<int32_t> d_music_peak_count;    // [B][VL] (NBLS_MUSIC_PEAKS; K of the plan's peak request)
    dev_buf<int32_t> d_music_peak_index;    // [B][VL][K]
    dev_buf<double> d_music_peak_power;     // [B][VL][K]
    dev_buf<double> d_music_peak_offset;    // [B][VL][K][2]
    dev_buf<double> d_music_slab;           // [slabs][G] (a peak request on a plan without NBLS_MUSIC_MAP)
    hipEvent_t ev_music_slab = nullptr;     // behind the last launch that used the slabs
    hipStream_t music_slab_stream = nullptr;    // where ev_music_slab was recorded last (nullptr: nowhere yet)
    // ---- the elements LTS kept (kept.hip) ----
    bool capon_kept_attr_set[3] = {false, false, false};    // the KEPT instances of capon_kernel have their dynamic LDS limit
    dev_buf<uint32_t> d_kept_mask;  // [B][VL] bit m: element m is dropped
    dev_buf<int32_t> d_kept_count;  // [B][VL] M
    // ---- the beam trace of every result row (beam_trace.hip) ----
    dev_buf<double> d_bt;           // [B][npts_pad]
    dev_buf<double> d_bt_win;       // the plan's synthesis windows
    dev_buf<int32_t> d_bt_off;      // [B] where the window of result row r starts in d_bt_win
    // ---- each element's delay against the beam of the others (element_delay.hip) ----
    bool ed_attr_set[4] = {false, false, false, false};   // the staged instances (plain, KEPT; x chunk) have their dynamic LDS limit
    dev_buf<int32_t> d_ed_K;        // [B] max_shift of the row's band
    dev_buf<double> d_ed_fp;        // [2][B][VL][N]: delay | cc
    dev_buf<int32_t> d_ed_shift;    // [B][VL][N]
    // ---- the pass's windows grouped into families (families.hip) ----
    nbls_family_work fam;           // the plan's labelling
    nbls_family_work fam_label;     // nbls_label_families' own: it changes nothing of a plan

    // ---- streamed results (nbls_stream_results): a pinned host mirror of the result block, filled batch by batch ----
    bool stream_results = false;
    hipStream_t cstream = nullptr;  // the D2H copies of the batches (a DMA engine beside the compute streams)
    struct result_batch { int64_t u0, u1, c0, c1; };
    std::vector<result_batch> rbatches;   // batches queued by the last nbls_execute*, in the order they finish
    std::vector<hipEvent_t> rev;    // 2 per batch: [2k] rows complete on the producing stream, [2k+1] copy landed
    std::string err;
    std::mutex err_mu;                 // fail() may be called from the upload thread (nbls_upload_rows) too
    bool trace_loaded = false;         // samples behind the declared shape (nbls_set_trace_shape / nbls_upload_rows)
    // The rows of a trace go up on a stream of their own, an event behind each: a pass queued while nbls_upload_rows is
    // still running on another thread filters the channels as they land (nbls_execute_stages) instead of waiting for the
    // last one — 16 elements x 24 h at 100 Hz are 1.1 GB = 20 ms over PCIe, the filter of a 12-band share 11 ms.
    hipStream_t ustream = nullptr;
    std::vector<hipEvent_t> uev;       // uev[c]: channel c is in HBM
    hipEvent_t ev_uprev = nullptr;     // what was queued on the compute streams before the upload (it may still read d_trace)
    std::atomic<int> rows_landed{0};   // channels whose copy is queued and whose event is recorded (published by the upload thread)
    std::atomic<int> upload_state{0};  // 0 no upload under way, 1 running, 2 shape declared (no samples yet), -1 the upload failed

    // ---- trace (HBM resident) ----
    dev_buf<double> d_trace;       // [nchans][npts_pad]
    int nchans = 0;                // trace rows
    int nseg = 1;                  // recordings in the trace (nbls_set_segments): nseg blocks of nelem consecutive rows
    int nelem = 0;                 // array elements = nchans / nseg: what the correlators, the screening buffers and the geometry see
    int64_t npts = 0, npts_pad = 0;
    double fs = 0.0;

    // ---- geometry: the pass's array, what the correlators see (its co-array is est[0]'s) ----
    int npairs = 0;
    dev_buf<int32_t> d_pair;       // [P][2]
    std::vector<int32_t> h_pair;   // host copy (as est[0].h_xij / h_xpinv): an identical nbls_set_geometry uploads nothing
    std::vector<double> h_tl, h_tr;   // host copies of the taper ramps (the same for every band group and call of one trace length: uploaded once)

    // ---- plan ----
    bool planned = false;
    int fbands = 0;                // filter bands of the plan (d_sos, d_M, d_fw; series of d_filt = fbands x nchans)
    int nbands = 0, nsections = 0, zero_phase = 0, taper_len = 0, vector_len = 0, xcorr_impl = 0;
    // nbands = result rows = fbands * nseg, row r = band r / nseg of recording r % nseg: the window / unit tables, the
    // result block and everything the correlators and solvers index are per row.  d_filt [fbands][nchans][npts_pad] is
    // the layout [nbands][nelem][npts_pad]
    std::vector<int32_t> W, inc, nwin, unit_off;
    int64_t nunits = 0;
    int maxW = 0;
    int uniW = 0;                  // the window length if every band has the same one, else 0
    int64_t nchunks = 0;
    dev_buf<double> d_sos;         // [B][S][6]
    dev_buf<double> d_M;           // [B][G+1][D][D] powers M^0..M^G of the chunk transition (D = 2S)
    dev_buf<double> d_fw;          // [B][C][D] zero-state end-state weights
    dev_buf<double> d_gend;        // [ngroups][B*N][D]
    dev_buf<double> d_gin;         // [ngroups][B*N][D]
    dev_buf<double> d_seg_state;   // [2][B*N][D] initial / final state of a time segment (nbls_filter_segment)
    dev_buf<double> d_tl;          // [taper_len]
    dev_buf<double> d_tr;          // [taper_len]
    dev_buf<int32_t> d_W;          // [B]
    dev_buf<int32_t> d_inc;        // [B]
    dev_buf<int32_t> d_nwin;       // [B]
    dev_buf<int32_t> d_unit_off;   // [B+1]
    dev_buf<int32_t> d_win_off;    // [B] first window processed per band
    std::vector<int32_t> win_first, win_count;   // optional per-band window ranges (nbls_set_window_ranges)
    dev_buf<int32_t> d_unit_band;// [U]
    dev_buf<int32_t> d_unit_win;   // [U] window index (global, inside the band) of every unit: saves the kernels a dependent load

    // ---- work + results ----
    dev_buf<double> d_filt;        // [B][N][npts_pad]
    dev_buf<double> d_cstate;      // [B*N][nchunks][D]
    dev_buf<double> d_cstate2;     // same, for the backward pass (its chunk states are produced by the forward apply)
    dev_buf<double> d_tstate;      // [B*N][C/T][nchunks][D] forward states at the tile boundaries (zero-phase, recompute form)
    dev_buf<int32_t> d_lag;        // [B][VL][P]
    dev_buf<double> d_cmax;        // [B][VL][P]
    dev_buf<double> d_lagfrac;     // [B][VL][P] sub-sample fraction of every lag (a plan with lag refinement, else not allocated)
    bool res_loaded = false;       // est[0].d_res holds a block put there by nbls_load_result_block (cleared by the next nbls_plan)
    size_t reserve_res = 0;        // minimum allocation of est[0]'s result block (nbls_reserve_results: equal gather blocks)
    // ---- RCCL gather (comm.hip) ----
    void* comm = nullptr;          // ncclComm_t
    int comm_world = 1, comm_rank = 0;
    dev_buf<unsigned char> d_gather; // [world][block_bytes] receive side
    int64_t gather_status = 0;     // host copy of the status word while its H2D copy is in flight
    // pinned staging of the plan tables (api.hip: alloc_copy): a copy from pinned memory goes through the DMA engines,
    // a copy from pageable memory is a shader copy that has to find a free CU — with three other band groups of the
    // call filling the GPU each of a plan's ~25 small uploads took ~60 us instead of ~5
    pinned_buf stage;
    size_t stage_used = 0;
    // a plan whose tables all went through the arena does not wait for their copies: the upload stream records ev_up,
    // and whatever launches kernels that read the tables (nbls_execute*, nbls_filter_segment) makes its streams wait
    // for it on the GPU; the next plan / geometry call waits for the upload stream before it reuses the arena
    hipEvent_t ev_up = nullptr;
    bool up_pending = false, stage_bypass = false;
    // nbls_plan's tables live in ONE device arena at the offsets they have in the staging arena and go up in ONE copy
    // when the plan returns (a plan is ~25 tables; each HIP call of a plan that runs beside the trace upload of a
    // pipelined call's first group waited for the runtime's lock: 0.8 instead of 0.4 ms before the first launch)
    std::vector<double> hp_M, hp_FW;       // host side of the plan's filter tables, kept between plans (no allocation per call)
    std::vector<int32_t> hp_ub, hp_uw;     // ... and of the unit -> (band, window) tables
    std::vector<int32_t> woff;     // first computed window of every band of the plan (0 unless window-sharded)
    bool work_queued = false;      // kernels that read the plan / geometry tables may still be queued (set by nbls_execute*, cleared by
                                   // the calls that wait for the handle's stream): a plan has to order its uploads behind them only then
    dev_buf<unsigned char> d_parena; // the tables placed in it say so themselves (dev_buf::in_arena) and are never freed one by one
    bool arena_mode = false;

    // ---- int8 screening correlator (xcorr_screen.hip) ----
    dev_buf<int8_t> d_qbuf;        // [batch][N][2][WP]
    dev_buf<double> d_qmeta;       // [batch][N][4]
    dev_buf<int32_t> d_cand;       // [batch][N][N][16]
    int64_t screen_batch = 0;
    int screen_wp = 0;             // padded window length the screening buffers are sized for (largest screened group)
    int64_t last_batch = 0;        // units of the last screening batch queued (developer statistics)
    std::vector<nbls_wgroup> wgroups;
    int skew_n = -1, skew_s = -1;  // partner-image skew of the screening kernel, solved once per (array size, tile shape)
    int skew_o[32] = {0};
    int64_t lts_stamp_waves = 0;              // developer: waves of the last LTS launch that wrote stamps
    dev_buf<unsigned long long> d_stamps; // developer: s_memtime stamps of the screen kernel's workgroups

    // ---- the estimators of the pass: est[0] the plan's own, est[1..nest] the further ones (nest == 0: the plain pass)
    int nest = 0;
    nbls_estimator est[1 + NBLS_MAX_ESTIMATORS];

    // ---- profiling ----
    bool prof = false;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool ev_valid = false;
    std::vector<hipEvent_t> bev;   // per-batch events of the screening path (5 per batch: quantize | screen | verify | solve)
    int bev_used = 0;
    bool prof_fused = false;       // the last profiled pass ran its solves per batch (bev[5k+4] recorded)
    int xcorr_impl_used = 0;       // 1 VALU, 2 f64 MFMA, 3 int8 screening, 4 bounded-lag correlator (at least one window group), 5 seeded correlator
    nbls_timings tim{};
};

// Kernel launchers (each returns hipError_t of the launch).
hipError_t nbls_launch_filter(nbls_handle* h, int ch0, int nch);    // channels [ch0, ch0 + nch) of every band
hipError_t nbls_launch_filter_segment(nbls_handle* h, int reverse, const double* d_init, double* d_fin);
hipError_t nbls_launch_xcorr(nbls_handle* h);
hipError_t nbls_launch_solve(nbls_handle* h);
hipError_t nbls_launch_solve_range(nbls_handle* h, int64_t u0, int64_t nu, hipStream_t st);
hipError_t nbls_launch_pack_weights(nbls_handle* h, int64_t u0, int64_t nu, hipStream_t st);
// What a record does not store: the four grids [B][VL] and the mask inside its result block, and the lag / cmax rows its
// solve reads (the pass's own for a full array, the record's compact ones for a sub-array; frac only under lag refinement).
struct nbls_est_view { double *vel, *baz, *mdccm, *sig; uint8_t* mask; int32_t* lag; double* cmax; double* frac; };
inline nbls_est_view nbls_view_of(const nbls_handle* h, const nbls_estimator& x) {
    const size_t cells = (size_t)h->nbands * h->vector_len;
    double* const g = (double*)x.d_res.p;
    const bool own = x.kept_pair.empty();
    return {g, g + cells, g + 2 * cells, g + 3 * cells, x.d_res ? x.d_res + 4 * cells * sizeof(double) : nullptr,
            own ? h->d_lag : x.d_lag, own ? h->d_cmax : x.d_cmax,
            h->req.refine ? (own ? h->d_lagfrac.p : x.d_lagfrac.p) : nullptr};       // (NULL: the solve reads tau = lag / fs)
}
// sub-sample fractions of the lags of units [u0, u0 + nu), behind their verifier (refine.hip; a plan with lag refinement)
hipError_t nbls_launch_refine(nbls_handle* h, int64_t u0, int64_t nu, int gW, hipStream_t st);
// dynamic LDS bytes of the form refine_lag_kernel takes for windows of W samples of nelem elements; 0: the global-memory form
size_t nbls_refine_lds_bytes_of(int nelem, int W);
// beam power and F-statistic of units [u0, u0 + nu) at the slowness estimator x has solved for them (beam.hip)
hipError_t nbls_launch_beam(nbls_handle* h, const nbls_estimator& x, int64_t u0, int64_t nu, hipStream_t st);
// ... its interpolated instances (beam_steer.hip; taps 4, 6 or 8): args is the argument block nbls_launch_beam has filled
hipError_t nbls_launch_beam_steer(int taps, bool kept, dim3 grid, dim3 block, hipStream_t st, const void* args);
// closure of the picked lags of units [u0, u0 + nu), per window and per element of estimator x (closure.hip)
hipError_t nbls_launch_closure(nbls_handle* h, const nbls_estimator& x, int64_t u0, int64_t nu, hipStream_t st);
// the elements LTS dropped in units [u0, u0 + nu), from estimator 0's unpacked weights (kept.hip)
hipError_t nbls_launch_kept_elements(nbls_handle* h, int64_t u0, int64_t nu, hipStream_t st);
// The kept set of a unit from its dropped mask (nbls_set_kept_elements): the complement among N elements, or the whole
// array where fewer than 3 would remain.  -> the kept bits; M is their count.
__host__ __device__ inline uint32_t nbls_kept_bits_of(uint32_t dropped, int N, int& M) {
    const uint32_t all = N >= 32 ? 0xffffffffu : ((1u << N) - 1u);
    uint32_t kept = ~dropped & all;
    M = __builtin_popcount(kept);
    if (M < 3) { kept = all; M = N; }
    return kept;
}
// the beam trace of every result row at the slowness estimator 0 has solved for its windows: one launch per pass, behind
// the last solve (beam_trace.hip)
hipError_t nbls_launch_beam_trace(nbls_handle* h, hipStream_t st);
// the families of a lattice of rows x vector_len cells (row r: band r / nseg of recording r % nseg; d_W, d_inc, d_nwin per
// row) from its four grids, into wk.family / wk.nfam / wk.table: eight launches on st (families.hip).  In a pass: once,
// behind the last solve, on estimator 0's result grids
hipError_t nbls_launch_families(const nbls_family_params& p, nbls_family_work& wk, int rows, int nseg, int vector_len,
                                const int32_t* d_W, const int32_t* d_inc, const int32_t* d_nwin, const double* vel, const double* baz,
                                const double* mdccm, const double* sig, hipStream_t st);
// rows of the device table of a labelling: no lattice of ncells cells has more families of min_pixels cells
size_t nbls_family_table_rows_of(int64_t ncells, int min_pixels);
// each element's delay against the beam of the others in units [u0, u0 + nu), at the slowness estimator 0 has solved for
// them; behind nbls_launch_kept_elements, whose mask the KEPT form reads (element_delay.hip)
hipError_t nbls_launch_element_delays(nbls_handle* h, int64_t u0, int64_t nu, hipStream_t st);
// dynamic LDS bytes of the staged form of element_delay_kernel for windows of W samples of nelem elements and shifts up to
// max_shift; 0: the global-memory form
size_t nbls_element_delay_lds_bytes_of(int nelem, int W, int max_shift);
// slowness-grid search of the beam F-statistic over units [u0, u0 + nu) for the plan's full array (beam_grid.hip)
hipError_t nbls_launch_beam_grid(nbls_handle* h, int64_t u0, int64_t nu, hipStream_t st);
// dynamic LDS bytes of the form beam_grid_kernel takes for windows of W samples of nelem elements and a halo of `halo`
// samples; 0: the global-memory form
size_t nbls_beam_grid_lds_bytes_of(int nelem, int W, int halo);
// the delay table d[G][nelem] of a grid and its halo (host, un-fused arithmetic); false: some |fs xij . s_g| reaches 2^30
bool nbls_beam_grid_delays_of(const double* xij, int nelem, double fs, const double* grid, int G, int32_t* d, int* halo);
// the tables of an interpolated grid plan: n[G][nelem] = floor(tau), c[G][nelem][taps] and the halo max(|n - K + 1|, |n + K|)
bool nbls_beam_grid_steer_of(const double* xij, int nelem, double fs, const double* grid, int G, int taps, int32_t* n, double* c,
                             int* halo);
// the grid maximum of units [u0, u0 + nu) refined between grid points, behind nbls_launch_beam_grid on the same stream
// (beam_grid_refine.hip)
hipError_t nbls_launch_beam_grid_refine(nbls_handle* h, int64_t u0, int64_t nu, hipStream_t st);
// dynamic LDS bytes of the form grid_refine_kernel takes for windows of W samples of nelem elements and a halo of `halo`
// samples; 0: the global-memory form
size_t nbls_beam_grid_refine_lds_bytes_of(int nelem, int W, int halo);
// the halo H_r of a refining plan: grid_halo + ceil(fs max_i(|xij[i][0]| step[0] + |xij[i][1]| step[1])) + 1 over the pairs
// (0, i); -1: it reaches 2^30
int64_t nbls_beam_grid_refine_halo_of(const double* xij, int nelem, double fs, int grid_halo, const double* step);
// Capon / Bartlett spectra of units [u0, u0 + nu) for the plan's full array (capon.hip)
hipError_t nbls_launch_capon(nbls_handle* h, int64_t u0, int64_t nu, hipStream_t st);
size_t nbls_capon_lds_bytes_of(int nelem);
// the CLEAN-SC components of units [u0, u0 + nu), behind nbls_launch_capon on the same stream (capon_clean.hip)
hipError_t nbls_launch_capon_clean(nbls_handle* h, int64_t u0, int64_t nu, hipStream_t st);
// dynamic LDS bytes of capon_clean_kernel: R, v and a column of a per lane
size_t nbls_capon_clean_lds_bytes_of(int nelem);
// the eigenvalues and the MUSIC spectrum of units [u0, u0 + nu), behind nbls_launch_capon on the same stream (capon_music.hip)
hipError_t nbls_launch_capon_music(nbls_handle* h, int64_t u0, int64_t nu, hipStream_t st);
// dynamic LDS bytes of capon_music_kernel: R, E, a column of a per lane, the step's rotations, the eigenvalues and their order
size_t nbls_capon_music_lds_bytes_of(int nelem);
// ... of the instance that keeps the unit's two maps of G points in LDS (the LDS route of a peak request); 0: it does not fit
size_t nbls_capon_peak_lds_bytes_of(int nelem, int G);
// the automatic route of a peak request: 1 LDS, 2 HBM
int nbls_capon_peak_route_of(int nelem, int G);
// the neighbour table nbr [8][G] of the lattice cells cell [G][2] of a peak request (host)
void nbls_capon_neighbours_of(const int32_t* cell, int G, int32_t* nbr);
// the snapshot coefficients coef [nbands][maxLs][2] and steering vectors steer [nbands][nelem][G][2] of a plan (host, un-fused)
void nbls_capon_tables_of(const double* xij, int nelem, double fs, const double* grid, int G, const double* freq,
                          const int32_t* snap_len, int nbands, int maxLs, double* coef, double* steer);
// [gather ->] solve -> [uncertainty ->] [beam ->] [closure ->] [grid search [-> its refinement] ->] [Capon ->] pack of units [u0, u0 + nu) for one estimator of the handle's plan
hipError_t nbls_launch_solve_set(nbls_handle* h, const nbls_estimator& x, int64_t u0, int64_t nu, hipStream_t st);
// streamed results: queue the copy of the rows of units [u0, u1) into the pinned mirror behind what `producer` has queued
hipError_t nbls_queue_result_batch(nbls_handle* h, int64_t u0, int64_t u1, hipStream_t producer);
hipError_t nbls_launch_probe_mfma(nbls_handle* h, const double* da, const double* db, double* dout);
// The correlator route of a window group (xcorr_route.hip; nbls_route_xcorr is its C ABI form).  no_screen: the general
// correlators only (a group that does not take the screening path); pad_kb: developer option screen_pad_kb.
struct nbls_route_query {
    int N, W, npairs, vrows;
    int64_t npts_pad;
    int impl, flags, pad_kb;
    bool no_screen;
};
void nbls_route_compute(const nbls_route_query& q, nbls_route* r);
// the query of a launch of handle h: its array, pair count, padded trace length and route options
nbls_route_query nbls_route_query_of(const nbls_handle* h, int W, int vrows, int impl, bool no_screen);
hipError_t nbls_launch_xcorr_screen_range(nbls_handle* h, int64_t ub, int64_t ue, int gW, int64_t* launches_io);
hipError_t nbls_xcorr_screen_finish(nbls_handle* h, int64_t launches);
// The tail of every launch of an FP64 correlator over the units [ub, ub + nu): the launch's error, then, in a plan with lag
// refinement, the lags' sub-sample fractions (refine.hip) behind the lag pick.
inline hipError_t nbls_finish_lag_pick(nbls_handle* h, int64_t ub, int64_t nu, int gW) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || !h->req.refine) return e;
    return nbls_launch_refine(h, ub, nu, gW, h->stream);
}
// Kernel arguments of the two range-restricted correlators (xcorr_bounded.hip, xcorr_seeded.hip; their kernels share the
// parts of lag_pick.h).
struct nbls_range_args {
    const double* filt;       // [B][N][npts_pad]
    int64_t npts_pad;
    int nchans;               // array elements N
    int npairs;
    const int32_t* pair;      // [P][2]
    const int32_t* Wb;        // [B]
    const int32_t* incb;      // [B]
    const int32_t* unit_band; // [U]
    const int32_t* unit_win;  // [U]
    int vector_len;
    int32_t* lag;             // [B][VL][P]
    double* cmax;             // [B][VL][P]
    int u0;                   // first unit of this launch
    int64_t nitems;           // general forms: (unit, pair) items of this launch
    // bounded
    const int32_t* limsq;     // [N][N] max_lag of the pair of two elements, symmetric, 0 on the diagonal (not yet clamped to W-1)
    int S, CS, PF;            // matrix-core form: lag blocks per tile, channel stride (doubles), zero prefix — as xcorr_mfma_kernel
    // seeded
    const int32_t* halfw;     // [B] half-width K of every result row
    const int32_t* delay;     // [G][N] the plan's delay table (beam_grid.hip)
    const int32_t* gindex;    // [B][VL] the grid maximum of every unit, -1: none
};
// ... with the common fields filled for the units [ub, ub + nu) of handle h
inline nbls_range_args nbls_range_args_of(const nbls_handle* h, int64_t ub, int64_t nu) {
    nbls_range_args a{};
    a.filt = h->d_filt;
    a.npts_pad = h->npts_pad;
    a.nchans = h->nelem;
    a.npairs = h->npairs;
    a.pair = h->d_pair;
    a.Wb = h->d_W;
    a.incb = h->d_inc;
    a.unit_band = h->d_unit_band;
    a.unit_win = h->d_unit_win;
    a.vector_len = h->vector_len;
    a.lag = h->d_lag;
    a.cmax = h->d_cmax;
    a.u0 = (int)ub;
    a.nitems = nu * h->npairs;
    return a;
}
// bounded-lag correlator (xcorr_bounded.hip): the form a window group takes (nbls_lag_limit_form is its C ABI form;
// min_limit: the smallest limit of the table) and the launch of units [ub, ue) of a group in form 1 / 2
int nbls_lag_limit_form_of(int nelem, int W, int min_limit);
hipError_t nbls_launch_xcorr_bounded(nbls_handle* h, int64_t ub, int64_t ue, int gW, int form);
// seeded correlator (xcorr_seeded.hip): the form a window group takes (nbls_lag_seed_form is its C ABI form: neither the
// half-width nor the halo enters) and the launch of units [ub, ue) of a group in form 1 / 2, behind the grid search of the
// same units on the handle's stream
int nbls_lag_seed_form_of(int nelem, int W);
hipError_t nbls_launch_xcorr_seeded(nbls_handle* h, int64_t ub, int64_t ue, int gW, int form);
hipError_t nbls_launch_probe_mfma_i8(nbls_handle* h, const int* da, const int* db, int* dout);
