/*
 * nbls.h — C ABI of libnbls_hip.so: the MI355X (gfx950) narrow-band least-squares /
 * least-trimmed-squares array processor.
 *
 * The reference (amiezzi/narrow_band_least_squares) is pure Python and has no FFI of its
 * own; this ABI is what a ctypes binding for its hot path binds (INTEGRATION.md shows the
 * stub).  Each entry point names the reference interface it replaces (file:line relative
 * to the reference checkout):
 *
 *   nbls_set_trace      <- the `st` argument of narrow_band_least_squares()
 *                          (narrow_band_least_squares.py:8,43) / ltsva() (:91)
 *   nbls_set_geometry   <- lat_list/lon_list -> rij -> co-array inside ltsva
 *                          (helpers.py:239-284; lts_array DataBin/LsBeam, source absent)
 *   nbls_plan           <- the per-band arguments of the band loop
 *                          (narrow_band_least_squares.py:67-91: filter_data() SOS,
 *                          WINLEN_list[ii], WINOVER, ALPHA)
 *   nbls_execute        <- one pass of the band loop body for every planned band:
 *                          helpers.py:124-139 (filter + taper) and ltsva
 *                          (narrow_band_least_squares.py:91 / :183)
 *   nbls_fetch[_packed] <- the result rows written at narrow_band_least_squares.py:104-113
 *                          (vel/baz/mdccm/sigma_tau), the lag vectors tau and the LTS
 *                          weights that become `stdict` (:114-124)
 *   nbls_run            <- convenience: plan + execute + sync + fetch
 *
 * Conventions: plain pointers and sizes; the caller owns every host buffer; the library
 * keeps no host pointer after a call returns; every function returns 0 on success or a
 * negative nbls_status; nbls_last_error() gives the message.  One handle = one GPU = one
 * host thread at a time.  All floating point is IEEE double.
 *
 * Amplitude.  The trace may be in any unit: no result depends on an absolute amplitude.  Every threshold below is a
 * ratio (the floors of the peak, CLEAN-SC and MUSIC requests, the diagonal loading, the tie rule of the lag pick), the
 * int8 screening quantises each channel window by its own max |x|, and no data-domain value is held in float.  So, as
 * long as no sample and no window's sum of squares is subnormal and every product of two such sums is finite — samples
 * within 2^+-100 of unit scale, the range the tests run, are far inside —
 *   - multiplying every sample by 2^k leaves every lag, cmax, MdCCM, weight, slowness, F ratio, index, count, offset,
 *     eigenvector and pseudo-spectrum unchanged bit for bit, multiplies the filtered samples and the beam trace by 2^k
 *     exactly, and every power, cross-spectral matrix and eigenvalue by 2^(2k) exactly;
 *   - negating every sample leaves everything unchanged and negates the filtered samples and the beam trace;
 *   - a positive gain 2^(k_i) of its own on every channel leaves the lags and everything computed from them alone
 *     unchanged (cmax, MdCCM, the sub-sample fractions, the solve, the confidence intervals, the closures, the dropped
 *     elements, the families); beams, spectra and element delays weight the elements by their amplitude and change.  The
 *     lags of a plan with a lag seed (nbls_set_lag_seed) start from a beam maximum and may change with them.
 * Gains that are no powers of two give the same to rounding.  One window's results depend on no other window's
 * amplitude, and one recording's of a batch on no other's (tests/test_gpu_scale.py).
 */
#ifndef NBLS_H
#define NBLS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nbls_handle nbls_handle;

typedef enum {
    NBLS_OK = 0,
    NBLS_ERR_ARG = -1,        /* bad shape / NULL pointer / out-of-range parameter   */
    NBLS_ERR_STATE = -2,      /* call order (no trace / geometry / plan yet)          */
    NBLS_ERR_GEOMETRY = -3,   /* < 3 elements, < 4 for LTS, rank-deficient co-array   */
    NBLS_ERR_HIP = -4,        /* HIP runtime failure                                  */
    NBLS_ERR_NOMEM = -5,      /* device allocation failed                             */
    NBLS_ERR_UNSUPPORTED = -6,/* size beyond what the kernels are built for           */
    NBLS_ERR_COMM = -7        /* RCCL not loadable / communicator failure             */
} nbls_status;

/* FAST-LTS parameters (lts_array LTSEstimator / robustbase ltsReg; host computes them). */
typedef struct {
    double alpha;           /* subset fraction in [0.5, 1)                              */
    int32_t h;              /* subset size                                              */
    int32_t nstarts;        /* number of elemental starts (<= 1024)                     */
    const int32_t* starts;  /* [nstarts][4] pair indices, -1 padded                     */
    int32_t csteps;         /* C-steps per start (4)                                    */
    int32_t csteps2;        /* max C-steps in the refinement (100)                      */
    int32_t ncand;          /* candidates refined (10, <= 16)                           */
    double xij_mad[2];      /* 1.4826 * median |xij| per column                         */
    double raw_factor;      /* raw consistency * small-sample correction factor         */
    const double* rew_table;/* [npairs+1] reweighted factor by number of unit weights   */
    double quantile;        /* weight cut-off (qnorm(0.9875))                           */
    double zero_scale;      /* exact-fit threshold (1e-7)                               */
} nbls_lts_params;

/* Per-run timing of the three stages, measured with HIP events on the handle's stream. */
typedef struct {
    double filter_ms;
    double xcorr_ms;
    double solve_ms;
    double total_ms;
    int64_t xcorr_launches;   /* unit batches of the correlation stage                         */
    double quantize_ms;       /* int8 screening path only: sums over the batches               */
    double screen_ms;         /*   the int8-MFMA screening kernel (dominant kernel)            */
    double verify_ms;         /*   the FP64 verification kernel                                */
    int32_t xcorr_impl;       /* correlator actually used: 1 VALU, 2 f64 MFMA, 3 int8 screening, 4 bounded-lag correlator,
                                 5 seeded correlator (nbls_set_lag_seed) */
    int32_t xcorr_fallback_bands; /* xcorr_impl == 3: bands whose window length does not fit the screening
                                   * kernel's LDS even with partner groups (> ~7900 samples) and ran on a general
                                   * correlator; the other bands of the plan were screened                    */
} nbls_timings;

int nbls_version(void);
/* Number of visible HIP devices (0 if the runtime cannot be initialised). */
int nbls_device_count(void);

/* Create a handle on HIP device `device_id` (lazy HIP init happens here, so it is safe to
 * fork before the first call).  *out is NULL on failure; nbls_last_error(NULL) explains. */
int nbls_create(int device_id, nbls_handle** out);
void nbls_destroy(nbls_handle* h);
const char* nbls_last_error(const nbls_handle* h);

/* Raw multichannel trace, channel-major contiguous trace[nchans][npts], copied to HBM and
 * kept resident until the next nbls_set_trace. */
int nbls_set_trace(nbls_handle* h, const double* trace, int32_t nchans, int64_t npts, double fs);

/* Same, from one pointer per channel (rows[c][npts], each contiguous): the traces of an obspy-like
 * Stream are separate arrays, this form uploads them without first packing them into one host block. */
int nbls_set_trace_rows(nbls_handle* h, const double* const* rows, int32_t nchans, int64_t npts, double fs);

/* Same trace as another handle of the SAME device, copied device-to-device (no second trip over PCIe): the
 * band groups of one call run as concurrent passes on several handles of one GPU. */
int nbls_set_trace_from(nbls_handle* h, const nbls_handle* src);

/* Two-step form of nbls_set_trace_rows (the `st` argument, narrow_band_least_squares.py:8,43; the reference copies it
 * per band, helpers.py:124) for a caller that overlaps the host-to-device copy with planning:
 * nbls_set_trace_shape declares the trace (allocation and shape, no samples), after which nbls_set_geometry and
 * nbls_plan may be called; nbls_upload_rows copies the samples (returns when the rows may be reused) and MAY RUN ON
 * ANOTHER THREAD meanwhile — the one exception to "one handle, one thread at a time".  nbls_execute returns
 * NBLS_ERR_STATE until nbls_upload_rows has returned — unless the upload was ANNOUNCED:
 * nbls_expect_upload (after nbls_set_trace_shape, by the thread that goes on to plan and execute) says that
 * nbls_upload_rows is about to run on another thread.  nbls_execute may then be called while the rows are still going
 * up: the rows travel on a stream of their own with an event behind each, and a pass with a filter stage filters the
 * channels as they land ((band, channel) series are independent: identical results) instead of starting after the last
 * one — the copy of a long trace (16 elements x 24 h at 100 Hz: 1.1 GB, 20 ms over PCIe) hides the filter.  It waits on
 * the host for each next row to be queued, and fails with NBLS_ERR_STATE if the upload fails, is aborted
 * (nbls_abort_upload: the announcing side learned that the rows will not come) or does not start within 120 s. */
int nbls_set_trace_shape(nbls_handle* h, int32_t nchans, int64_t npts, double fs);
int nbls_upload_rows(nbls_handle* h, const double* const* rows, int32_t nchans, int64_t npts);
int nbls_expect_upload(nbls_handle* h);
int nbls_abort_upload(nbls_handle* h);

/* Co-array: xij[npairs][2] (km; pair k = (i,j), i<j, lexicographic; xij = r_i - r_j),
 * pair_idx[npairs][2], xpinv[2][npairs] = pseudo-inverse of xij (OLS). */
int nbls_set_geometry(nbls_handle* h, const double* xij, const int32_t* pair_idx,
                      const double* xpinv, int32_t npairs);

/* Describe the bands to process.
 *   sos[nbands][nsections][6]   second-order sections actually applied (a0 == 1);
 *                               nsections == 0 (sos NULL): the trace is already filtered
 *                               (ltsva() on a filtered stream), it is only copied/tapered
 *   zero_phase                  0 causal single pass, 1 forward-backward
 *   taper_left/right[taper_len] whole-trace taper ramps multiplied onto the first/last samples
 *   winlen/wininc[nbands]       window length / hop in samples
 *   vector_len                  row length of the result grids (>= max windows per band)
 *   lts                         NULL -> ordinary least squares
 *   xcorr_impl                  0 auto, 1 plain VALU kernel, 2 f64-MFMA kernel,
 *                               3 int8-MFMA screening + FP64 verification
 * May be called while a pass of this handle is still queued (nbls_execute is asynchronous): the table uploads of
 * the new plan are ordered behind that pass on the GPU, without a host wait.  Fetch that pass's results BEFORE
 * planning again: the layout nbls_fetch* / nbls_result_layout use is the current plan's.
 */
int nbls_plan(nbls_handle* h, int32_t nbands, const double* sos, int32_t nsections,
              int32_t zero_phase, const double* taper_left, const double* taper_right,
              int32_t taper_len, const int32_t* winlen, const int32_t* wininc,
              int32_t vector_len, const nbls_lts_params* lts, int32_t xcorr_impl);

/* Several recordings of ONE array in one pass: the trace's nchans rows are nseg consecutive blocks of
 * E = nchans / nseg rows, block s = recording s (same element order, npts and fs for all).  The geometry
 * describes one array of E elements.  The next nbls_plan with B bands gives B*nseg result rows, row
 * r = b*nseg + s (band-major): nbls_fetch, nbls_fetch_packed, nbls_result_layout, nbls_fetch_uncertainty and the
 * streamed result batches all describe B*nseg rows; nbls_fetch_filtered still takes a band b < B and returns all
 * nchans trace rows.  nseg = 1 (the default) is the one-recording behaviour.  At plan time: NBLS_ERR_ARG if
 * nchans % nseg != 0, NBLS_ERR_GEOMETRY if E is outside 3..32 (or below 4 under LTS), NBLS_ERR_UNSUPPORTED
 * together with nbls_set_window_ranges or an RCCL communicator (nbls_comm_*).  No kernel changes: the filter
 * writes [B][nseg*E][npts] = [B*nseg][E][npts], which is what the correlators read for B*nseg rows of E elements. */
int nbls_set_segments(nbls_handle* h, int32_t nseg);

/* Window sharding (fewer bands than GPUs, or traces too long for one GPU's time
 * budget): restrict the NEXT plans to windows [first[b], first[b] + count[b]) of band b (count < 0 =
 * to the end).  The filter still runs over the whole trace (zero-phase filtering is not local in time),
 * correlation and solve only over the slice; result rows keep their global window index, rows outside
 * the slice stay zero, so the slices of several GPUs combine by addition.  nbands <= 0 resets. */
int nbls_set_window_ranges(nbls_handle* h, int32_t nbands, const int32_t* first, const int32_t* count);

/* Launch the whole pass (filter -> xcorr/lag pick -> MdCCM + OLS|LTS) asynchronously on the
 * handle's stream; nbls_sync waits for it. */
int nbls_execute(nbls_handle* h);
/* Same, restricted to a subset of stages: bit 0 filter, bit 1 xcorr/lag pick, bit 2 solve
 * (filter only = the reference's filter_data(), helpers.py:108-141). */
int nbls_execute_stages(nbls_handle* h, int32_t stage_mask);
/* nbls_execute for several handles of ONE GPU whose passes are queued one after the other (the band groups of one
 * call = consecutive iterations of the reference's band loop, narrow_band_least_squares.py:64-124): the correlation stage of `h` starts when the correlation stage `prev` has queued is through (a GPU-side
 * wait, the call itself returns at once); h's filter stage may run beside it.  The passes then finish in the order
 * they were queued, so the caller can work on the first one's results while the later ones are still running —
 * without this the GPU shares itself between the passes and they all finish together at the end.  Results are the
 * same either way.  NBLS_ERR_STATE if `prev` has not queued a pass, NBLS_ERR_ARG for handles of different devices. */
int nbls_execute_after(nbls_handle* h, nbls_handle* prev);
int nbls_sync(nbls_handle* h);

/* Copy results to host.  Any pointer may be NULL to skip it.
 *   vel/baz/mdccm/sigma_tau [nbands][vector_len]   (zeros beyond nwin[b])
 *   nwin[nbands]
 *   lag [nbands][vector_len][npairs] int32: tau = lag / fs  (lag = W - 1 - argmax)
 *   cmax[nbands][vector_len][npairs] normalised cross-correlation maxima
 *   weights[nbands][vector_len][npairs] uint8 (1 = kept, 0 = dropped by LTS; all 1 for OLS)
 *   z[nbands][vector_len][2] slowness estimate (s/km) */
int nbls_fetch(nbls_handle* h, double* vel, double* baz, double* mdccm, double* sigma_tau,
               int32_t* nwin, int32_t* lag, double* cmax, uint8_t* weights, double* z);

/* Confidence intervals of the slowness estimate — the 7th / 8th returns of ltsva (vel_uncert, baz_uncert at
 * narrow_band_least_squares.py:91, example.py:109; Szuberla & Olson 2004 as used by lts_array): half the spread of the
 * trace velocity over the 90 % confidence ellipse of the slowness vector (semi-axes sqrt(chi2_{0.90,2}) sigma_tau /
 * sqrt(lambda_i) along the eigenvectors of X^T X) and half the angle the ellipse subtends at the origin (NaN when the
 * origin is inside).  Computed on the GPU behind every unit's solve when wanted:
 *   nbls_set_uncertainty(h, eig6)   eig6 = {lambda_0, lambda_1 (ascending), R00, R01, R10, R11}: eigenvalues of X^T X
 *                                   and the rotation into its eigen-frame (c = R z); NULL switches it off (default:
 *                                   the band loop discards these two returns).  Read by the next nbls_plan.
 *   nbls_fetch_uncertainty(h, vel_uncert, baz_uncert)   [nbands][vector_len] each (either may be NULL), zeros beyond
 *                                   nwin[b]; waits for the pass like nbls_fetch. */
int nbls_set_uncertainty(nbls_handle* h, const double* eig6);
int nbls_fetch_uncertainty(nbls_handle* h, double* vel_uncert, double* baz_uncert);

/* Beam power and Fisher F-statistic of the delay-and-sum beam at the solved slowness, computed on
 * the GPU behind every unit's solve when wanted — per estimator, with that estimator's N elements (estimator 0: every
 * element of the row's recording; a further one: the trace rows kept[]) and its own slowness z.  For the unit of result
 * row r, window w (start s0 = w * wininc, length W):
 *   delays   d_0 = 0, d_i = rint(fs * (xij[k][0] z0 + xij[k][1] z1)), ties to even, k = i - 1 the index of pair (0, i) in
 *            the estimator's own pair list: the modelled lag of pair (0, i) in samples, in the sign convention of the
 *            measured lag of nbls_fetch (lag = W-1-argmax, tau = xij . z) — element i lags element 0 by d_i samples
 *   samples  x_i[t] = filt[row of element i][s0 + t + d_i] for t in [0, W), 0.0 where the index is outside [0, npts)
 *   sums     b[t] = sum_i x_i[t], S_b = sum_t b[t]^2, S_t = sum_t sum_i x_i[t]^2, D = N S_t - S_b
 *   outputs  beam_power = S_b / (N^2 W), fstat = (N - 1) S_b / D; fstat = +inf if D <= 0 and S_b > 0; fstat = NaN and
 *            beam_power = 0 if S_t == 0; both NaN if z is not finite, some |fs xij . z| is at least 2^30, or a sample
 *            read is NaN.  Cells beyond nwin[r] (and outside a window slice) are zeros.
 * The order of every sum is fixed per (N, W) and no floating-point atomics are used: single, batched and streamed passes
 * agree bit for bit.
 *   nbls_set_beam(h, on)     read by the next nbls_plan; a plan without it is launch for launch the plain pass.
 *                            NBLS_ERR_UNSUPPORTED from nbls_plan with an RCCL communicator (the gathered block does
 *                            not carry the two grids).
 *   nbls_fetch_beam(h, beam_power, fstat)   [rows][vector_len] each (either may be NULL), rows as for nbls_fetch; waits for
 *                            the pass like nbls_fetch_uncertainty.  NBLS_ERR_STATE if the plan did not ask for beam results.
 *                            The grids are written by the solve stage alone: zeros until a pass of the plan has run it,
 *                            and nbls_execute_stages without the solve bit leaves them as they are.
 * nbls_timings is unchanged: the kernel's time falls inside the solve interval. */
int nbls_set_beam(nbls_handle* h, int32_t on);
int nbls_fetch_beam(nbls_handle* h, double* beam_power, double* fstat);

/* Sub-sample refinement of the picked lags, computed on the GPU in the correlation stage behind
 * the verifier of each unit batch when wanted.  For one unit and one pair (i, j) with picked lag l = W-1-argmax, which stays
 * exactly what it is today, let a, b be the unit's windows of elements i and j as the correlator saw them.  Define
 *   R(m) = sum_n a[n-m] b[n]  over the n for which both indices are in [0, W): np.correlate(a, b, 'full')[W-1-m], raw and
 *            not normalised
 *   Nn   = R(l-1) - R(l+1)
 *   D    = R(l-1) - 2 R(l) + R(l+1)
 *   frac = 1/2 Nn / D, clamped to [-1/2, 1/2]
 *   frac = 0.0 in each of these cases: |l| >= W-1; D >= 0 (no strict maximum: dead channel, plateau); any of the three
 *            values or the quotient is not finite (NaN / Inf windows keep today's behaviour)
 *   tau  = ((double)lag + frac) / fs, in un-fused IEEE double, in exactly this form at every site that reads a lag
 * All three R are computed by the refinement kernel itself, in one summation order (R(l) is not cmax * norm).  The
 * summation order depends on (W, l) alone; no atomics are used, and nothing depends on the launch's unit range: single,
 * streamed, batched, window-sliced and multi-estimator passes agree bit for bit, and a sub-array estimator agrees with a
 * separate call on the sub-array.  cmax, MdCCM, nbls_fetch's lag, the key text of stdict and the MAD(tau) == 0 -> NaN rule
 * are unchanged.  Cells beyond nwin are zeros.
 *   nbls_set_lag_refinement(h, on)   read by the next nbls_plan, like nbls_set_beam; a plan without it is launch for launch
 *                            the plain pass.  An RCCL communicator is not refused: the gathered block carries everything
 *                            that changes; the fractions themselves are fetched locally only.
 *   nbls_fetch_lag_fraction(h, frac)   [rows][vector_len][npairs]; waits for the pass like nbls_fetch.
 *   nbls_est_fetch_lag_fraction(h, e, frac)   the same for estimator e, [rows][vector_len][P'] (nbls_set_estimators).
 *                            Both return NBLS_ERR_STATE if the plan did not ask for refinement.  The fractions are written by
 *                            the correlation stage alone: zeros until a pass of the plan has run it, and
 *                            nbls_execute_stages without that bit keeps the fractions it has (the solve goes on using them).
 * nbls_timings is unchanged: the kernel's time falls inside the correlation interval (on the screening path inside
 * verify_ms). */
int nbls_set_lag_refinement(nbls_handle* h, int32_t on);
/* Which of its two forms the refinement kernel takes for windows of W samples of an array of nelem elements (a pure host
 * function, like nbls_route_xcorr): the dynamic LDS bytes of the form that stages the unit's nelem windows in LDS
 * (nelem * W * 8, up to 80 KiB), or 0 for the form that reads them from global memory.  Both give the same bits.
 * NBLS_ERR_ARG for nelem < 1 or W < 1. */
int nbls_refine_lds_bytes(int32_t nelem, int32_t W);
int nbls_fetch_lag_fraction(nbls_handle* h, double* frac);
int nbls_est_fetch_lag_fraction(nbls_handle* h, int32_t e, double* frac);

/* Per-pair lag limits: the lag pick of pair k searched only within |lag| <= max_lag[k] samples, the
 * range a plane wave no slower than v_min can delay that pair (|tau_k| <= |xij_k| / v_min), instead of over all 2W-1 lags —
 * in a narrow band the correlation is nearly periodic and noise lifts a neighbouring cycle above the true one.  For one unit
 * and pair k = (i, j), a, b the unit's windows of elements i and j, R(m) = sum_n a[n-m] b[n] over the indices inside [0, W)
 * (np.correlate(a, b, 'full')[W-1-m], the definition of nbls_set_lag_refinement), max_lag[k] >= 0 and L = min(max_lag[k], W-1):
 *   lag  = L - np.argmax(cij[W-1-L : W+L]),  cij = np.correlate(a, b, 'full') / sqrt(sum a^2 * sum b^2); quotients are
 *          compared as the plain pass compares them, and the first maximum in np.correlate index order wins: among equal
 *          maxima the LARGEST lag
 *   cmax = R(lag) / sqrt(sum a^2 * sum b^2)
 *   an all-zero range gives lag = +L, cmax = 0; a dead channel lag = +L, cmax = NaN; windows whose sum of squares is not
 *          finite (NaN or +-Inf samples) give cmax = NaN and lag = min(the plain pass's lag, L) — NumPy's first NaN of the slice
 *   max_lag[k] >= W-1 is the full search for that pair: the plain pass's lag
 * MdCCM, the solve, the uncertainty, beam and refinement kernels read these picks as they read the plain pass's.  The order
 * of every sum depends on (number of elements, W, the limit table, lag) alone, no atomics are used and nothing depends on
 * the launch's unit range: single, streamed, batched (nbls_set_segments) and window-sliced passes agree bit for bit.  A
 * sub-array estimator reads the full array's picks; against a separate call on the sub-array it agrees in lags and weights
 * exactly and in cmax to 1e-12 (the tile origins differ with the element count).
 *   nbls_set_lag_limits(h, max_lag, npairs)   the table is copied and read by the next nbls_plan, like nbls_set_beam; max_lag
 *                            NULL switches it off (the default: a plan without it is launch for launch the plain pass).
 *                            NBLS_ERR_ARG for a negative entry or npairs < 1, and the handle is then unchanged.  nbls_plan
 *                            returns NBLS_ERR_ARG if npairs differs from the geometry's, NBLS_ERR_UNSUPPORTED if limits are
 *                            set and xcorr_impl != 0.  An RCCL communicator, segments, window ranges and estimators are not
 *                            refused: the result block carries everything that changes.
 *   nbls_lag_limit_form(nelem, W, min_limit)   a pure host function, like nbls_refine_lds_bytes: the form a window group of
 *                            W-sample windows of nelem elements takes when the SMALLEST limit of the table is min_limit
 *                            (values above W-1 count as W-1): 0 the plan's ordinary route — every pair's limit reaches
 *                            W-1, the full search is the bounded one; 1 the matrix-core form (3..16 elements whose
 *                            zero-padded windows fit a CU's LDS: the fit rule of NBLS_ROUTE_MFMA); 2 the general form
 *                            (everything else).  NBLS_ERR_ARG for nelem outside 3..32, W < 2 or min_limit < 0.  The
 *                            launcher decides through the same function.
 * A group in form 1 or 2 takes the place a general correlator has in the pass: one launch over the group's units (and one
 * result batch of a streamed pass), refinement behind it when the plan refines.  nbls_timings.xcorr_impl is 4 for a pass in
 * which at least one window group ran the bounded-lag correlator; its time falls inside xcorr_ms. */
int nbls_set_lag_limits(nbls_handle* h, const int32_t* max_lag, int32_t npairs);
int nbls_lag_limit_form(int32_t nelem, int32_t W, int32_t min_limit);

/* Slowness-grid search of the beam F-statistic: per window, the delay-and-sum beam of the plan's full
 * array steered over G caller-given slowness vectors, and the vector with the largest Fisher ratio — the estimate that does
 * not rest on pairwise lag picks.  grid[G][2] is in s/km, in the (z0, z1) convention of the solved z of nbls_fetch,
 * 1 <= G <= 65536 (NBLS_BEAM_GRID_MAX).  N = nelem, every element of the row's recording; the geometry's first N-1 pairs are
 * the pairs (0, i).
 *   delays   once per plan: d[g][0] = 0, d[g][i] = rint(fs * (xij[i-1][0] s_g0 + xij[i-1][1] s_g1)), un-fused IEEE double,
 *            ties to even; the sign is nbls_set_beam's: element i is read at +d_i.  H = max |d[g][i]| is the plan's halo.
 *   samples  for the unit of result row r, window w (start s0 = w * wininc, length W) and grid point g:
 *            x_i[t] = filt[row of element i][s0 + t + d[g][i]] for t in [0, W), 0.0 where the index is outside [0, npts)
 *   sums     b[t] = sum_i x_i[t], S_b = sum_t b[t]^2, S_t = sum_t sum_i x_i[t]^2, D = N S_t - S_b
 *   values   F(g) = (N - 1) S_b / D; F(g) = +inf if D <= 0 and S_b > 0; F(g) = NaN if S_t == 0 or a NaN sample was read;
 *            P(g) = S_b / (N^2 W)
 *   outputs  grid_index (int32): the g with the largest F under the total order "F descending (+inf first), g ascending";
 *            NaN values of F are not candidates; -1 if no g has a non-NaN F.  grid_fstat = F(grid_index), grid_power =
 *            P(grid_index), both NaN when the index is -1.  The map, if the plan asked: every F(g); grid_fstat is bit-equal
 *            to the map's entry at grid_index.  Cells beyond nwin[r] (and outside a window slice) are zeros.
 * One wave sums one (unit, grid point): the order of every sum depends on (N, W) alone, the arg-max is a total order, no
 * atomics are used and nothing depends on the launch's unit range: single, streamed, batched (nbls_set_segments) and
 * window-sliced passes agree bit for bit, and grid points with identical delay rows give identical bits.
 *   nbls_set_beam_grid(h, grid, G, want_map)   the grid is copied and read by the next nbls_plan, like nbls_set_beam; grid
 *                            NULL switches the search off (the default: a plan without it is launch for launch the plain
 *                            pass).  NBLS_ERR_ARG for G outside 1..65536 or an entry that is not finite, and the handle is
 *                            then unchanged.  nbls_plan returns NBLS_ERR_ARG if some |fs xij . s_g| is at least 2^30,
 *                            NBLS_ERR_STATE without the geometry, NBLS_ERR_UNSUPPORTED with an RCCL communicator (the
 *                            gathered block does not carry the grids).  Further estimators (nbls_set_estimators) get no
 *                            grid results: the search is over the full array, behind estimator 0's solve.
 *   nbls_fetch_beam_grid(h, index, fstat, power)   [rows][vector_len] each (any may be NULL), rows as for nbls_fetch; waits
 *                            for the pass like nbls_fetch_beam.  NBLS_ERR_STATE if the plan did not ask for the search.
 *   nbls_fetch_beam_grid_map(h, map)   [rows][vector_len][G]; NBLS_ERR_STATE if the plan did not ask for the map.
 *   nbls_fetch_beam_grid_delays(h, d)  [G][nelem] int32, the plan's own delay table.
 *                            The grids and the map are written by the solve stage alone: zeros until a pass of the plan
 *                            has run it, and nbls_execute_stages without the solve bit leaves them as they are.
 *   nbls_beam_grid_lds_bytes(nelem, W, halo)   a pure host function, like nbls_refine_lds_bytes: which of its two forms the
 *                            kernel takes for windows of up to W samples of nelem elements under a halo of `halo` samples:
 *                            the dynamic LDS bytes of the form that stages the unit's rows over [s0 - H, s0 + W + H) in LDS
 *                            (nelem * (W + 2 halo) * 8, up to 156 KiB), or 0 for the form that reads them from global
 *                            memory.  Both give the same bits.  NBLS_ERR_ARG for nelem < 1, W < 1 or halo < 0.  A workgroup
 *                            has NBLS_BEAM_GRID_WAVES waves; wave j takes the grid points j, j + NBLS_BEAM_GRID_WAVES, ...
 * nbls_timings is unchanged: the kernel's time falls inside the solve interval. */
#define NBLS_BEAM_GRID_MAX 65536
#define NBLS_BEAM_GRID_WAVES 16
int nbls_set_beam_grid(nbls_handle* h, const double* grid, int32_t G, int32_t want_map);
int nbls_beam_grid_lds_bytes(int32_t nelem, int32_t W, int32_t halo);
int nbls_fetch_beam_grid(nbls_handle* h, int32_t* index, double* fstat, double* power);
int nbls_fetch_beam_grid_map(nbls_handle* h, double* map);
int nbls_fetch_beam_grid_delays(nbls_handle* h, int32_t* d);

/* Seeded lag search: a plan with a slowness grid (nbls_set_beam_grid) and a seed table searches every
 * pair's lag only near the delay the unit's grid maximum predicts — the whole-array beam chooses the cycle, the pairwise
 * correlation is searched within half a period of it, and the existing solve runs on those picks.  For the unit of result
 * row r, window w, band b of row r, g = grid_index[r][w], and pair k = (i, j), i < j, a, b the unit's windows of elements i
 * and j, R(m) = sum_n a[n-m] b[n] (np.correlate(a, b, 'full')[W-1-m], as for nbls_set_lag_limits),
 * cij = np.correlate(a, b, 'full') / sqrt(sum a^2 * sum b^2) and K = halfwidth[b] >= 0:
 *   centre  c  = d[g][j] - d[g][i]   (int32 arithmetic on the plan's delay table, nbls_fetch_beam_grid_delays);  c = 0 if g == -1
 *           c' = min(max(c, -(W-1)), W-1)
 *   range   lo = max(c' - K, -(W-1)),  hi = min(c' + K, W-1)          (never empty)
 *   lag     = hi - np.argmax(cij[W-1-hi : W-lo]);  quotients are compared as the plain pass compares them, with "no lag seen
 *           yet" as the least element, and the first maximum in np.correlate index order wins: among equal maxima the LARGEST lag
 *   cmax    = R(lag) / sqrt(sum a^2 * sum b^2)
 *   an all-zero range gives lag = hi, cmax = 0; a dead channel lag = hi, cmax = NaN; a pair whose sum of squares of either
 *           window is not finite (NaN or +-Inf samples) lag = hi, cmax = NaN — NumPy's answer for NaN samples, a deliberate
 *           simplification for Inf samples (the reference has no seeded search: the contract is this library's)
 *   K >= 2 (W-1) is the full search: the plain pass's lag
 * The centre is d_j - d_i, the steering the beam used, not rint(fs xij_k . s): integer arithmetic on a table the caller can
 * fetch.  MdCCM, the solve, the uncertainty, beam and refinement kernels and the gather of sub-array estimators read these
 * picks as they read the plain pass's.  The order of every sum depends on (number of elements, W, range, lag) alone, no
 * atomics are used and nothing depends on the launch's unit range: single, streamed, batched (nbls_set_segments) and
 * window-sliced passes agree bit for bit.
 *   nbls_set_lag_seed(h, halfwidth, nbands)   the table is copied and read by the next nbls_plan, like nbls_set_lag_limits;
 *                            halfwidth NULL switches it off (the default: a plan without it queues the launches it queued
 *                            before).  NBLS_ERR_ARG for a negative entry or nbands < 1, and the handle is then unchanged.
 *                            nbls_plan returns NBLS_ERR_ARG if nbands differs from the plan's, NBLS_ERR_STATE if no grid is
 *                            set, NBLS_ERR_UNSUPPORTED together with nbls_set_lag_limits (the grid's own extent bounds the
 *                            slowness: one restriction at a time) or with xcorr_impl != 0.  Segments, window ranges and
 *                            estimators are not refused: with segments halfwidth is indexed by band b of row r = b nseg + s,
 *                            and a sub-array estimator reads the full array's picks.
 *   nbls_lag_seed_form(nelem, W, max_halfwidth, halo)   a pure host function, like nbls_lag_limit_form: the form a window
 *                            group of W-sample windows of nelem elements takes: 1 the staged form (3..16 elements whose
 *                            windows and sums of squares, nelem (W + 1) doubles, fit 156 KiB of a CU's LDS; the staged block
 *                            has no padding, so max_halfwidth and halo do not enter the rule), 2 the general form
 *                            (everything else).  Never 0: every window group of a seeded plan takes the seeded correlator.
 *                            NBLS_ERR_ARG for nelem outside 3..32, W < 2, max_halfwidth < 0 or halo < 0.  The launcher
 *                            decides through the same function.  The two forms give the same bits.
 * Stage order.  In a seeded plan the grid search belongs to the CORRELATION stage: per window group, on the handle's stream,
 * the grid kernel over the group's units, then the seeded correlator, then refinement if the plan refines (and, when a pass
 * solves per batch, the group's solve and result batch: a seeded group is one result batch of a streamed pass).  The solve
 * stage does not run the grid kernel for such a plan.  The grid kernel and its outputs are those of the same plan without a
 * seed, bit for bit, but they are written by stage bit 2 (the correlation stage) — zeros until a pass of the plan has run
 * it, and nbls_execute_stages with only the solve bit leaves picks and grid results as they are — and the grid kernel's time
 * falls inside xcorr_ms.  nbls_timings.xcorr_impl is 5 for a pass of a seeded plan. */
int nbls_set_lag_seed(nbls_handle* h, const int32_t* halfwidth, int32_t nbands);
int nbls_lag_seed_form(int32_t nelem, int32_t W, int32_t max_halfwidth, int32_t halo);

/* Closure (consistency) of the picked lags, computed on the GPU behind every unit's solve when
 * wanted: for three elements i < j < k the lags of any single coherent arrival satisfy l_ij + l_jk - l_ik = 0, whatever its
 * slowness, its wavefront's curvature or the elements' clock offsets (Cansi 1995); only noise, cycle skips and several
 * arrivals break it.  The definition is per estimator: N is that estimator's element count (estimator 0: every element; a
 * further one: its nkept elements), its pair list the lexicographic one of P' = N (N-1) / 2 pairs, k(i,j) the index of pair
 * (i, j), i < j, in that list.  For the unit of result row r, window w:
 *   t_ij     plan without lag refinement:  t_ij = lag[k(i,j)]                     (int32, exactly the lag of nbls_fetch / nbls_est_fetch)
 *            plan with lag refinement:     t_ij = (double)lag[k(i,j)] + frac[k(i,j)]   (the sum every other site forms, un-fused double)
 *   closure  c_ijk = (t_ij + t_jk) − t_ik           for i < j < k;  T = N (N−1)(N−2) / 6 triplets
 *   sums     Q = Σ_{i<j<k} c_ijk²,   E_m = Σ_{triplets that contain element m} c_ijk²,   T_m = (N−1)(N−2) / 2
 *   outputs  consistency            = sqrt(Q / T) / fs                          seconds, [rows][VL]
 *            closure_max            = max_{i<j<k} |c_ijk| / fs                  seconds, [rows][VL]
 *            element_consistency[m] = sqrt(E_m / T_m) / fs                      seconds, [rows][VL][N]
 * Without refinement c, Q and E_m are computed exactly in integers (int64: |c| <= 3 (W-1)), converted to double once, and
 * the three double operations are done in that order.  With refinement everything is un-fused IEEE double and the order of
 * every sum depends on N alone; no floating-point atomics are used and nothing depends on the launch's unit range: single,
 * streamed, batched (nbls_set_segments) and window-sliced passes agree bit for bit, and a sub-array estimator agrees bit
 * for bit with a separate call on the sub-array.  Cells beyond nwin[r] (and outside a window slice) are zeros, and so is
 * everything for an array of fewer than three elements.  The results follow whatever picks the plan made: full, bounded
 * (nbls_set_lag_limits) or seeded (nbls_set_lag_seed).  Lags are finite integers and fractions are finite: no NaN rule.
 *   nbls_set_closure(h, on)  read by the next nbls_plan, like nbls_set_beam; a plan without it is launch for launch the
 *                            plain pass.  nbls_plan returns NBLS_ERR_UNSUPPORTED with an RCCL communicator (the gathered
 *                            block does not carry the grids) and NBLS_ERR_STATE without the geometry of the trace's array
 *                            (every pair, in lexicographic order).  Segments, window ranges, estimators, lag limits, grid,
 *                            seed and refinement are not refused.
 *   nbls_fetch_closure(h, consistency, closure_max, element_consistency)   [rows][vector_len], [rows][vector_len] and
 *                            [rows][vector_len][nelem] (any may be NULL), rows as for nbls_fetch; waits for the pass like
 *                            nbls_fetch_beam.  NBLS_ERR_STATE if the plan did not ask for closure results.  The grids are
 *                            written by the solve stage alone: zeros until a pass of the plan has run it, and
 *                            nbls_execute_stages without the solve bit leaves them as they are.
 *   nbls_est_fetch_closure(h, e, ...)   the same for estimator e, element rows [rows][vector_len][nkept_e]
 *                            (nbls_set_estimators).
 * nbls_timings is unchanged: the kernel's time falls inside the solve interval. */
int nbls_set_closure(nbls_handle* h, int32_t on);
int nbls_fetch_closure(nbls_handle* h, double* consistency, double* closure_max, double* element_consistency);

/* Capon (MVDR) and Bartlett slowness spectra of the narrow band's cross-spectral matrix: per window,
 * the adaptive beamformer that separates two arrivals closer than the array's beam width, where the delay-and-sum search of
 * nbls_set_beam_grid merges them.  grid[G][2] is in s/km, the convention of nbls_set_beam_grid, 1 <= G <= 65536
 * (NBLS_CAPON_GRID_MAX); per band b a frequency f_b > 0 (Hz), a snapshot length Ls_b >= 1 and a hop Hs_b >= 1 (samples); one
 * diagonal loading delta >= 0.  N = nelem (3..32, NBLS_CAPON_MAX_ELEMENTS), W_b the band's window length, xij the geometry's
 * first N-1 pairs (0, i).
 *   tables   once per plan, host, un-fused IEEE double:
 *            c_b[n]    = (0.5 - 0.5 cos((2 pi (n + 0.5)) / Ls_b)) (cos p, sin p),  p = -(((2 pi f_b) n) / fs),  n < Ls_b
 *            a_b[g][0] = 1,  a_b[g][i] = (cos q, sin q),  q = -((2 pi f_b) tau_i(g)),
 *            tau_i(g)  = xij[i-1][0] s_g0 + xij[i-1][1] s_g1   (seconds: what the delay table of nbls_set_beam_grid rounds
 *                        after multiplying by fs)
 *            K_b       = 1 + (W_b - Ls_b) div Hs_b   snapshots
 *   matrix   for the unit of result row r (band b), window w (start s0 = w * wininc):
 *            X_i[k] = sum_{n < Ls} c[n] filt[row of element i][s0 + k Hs + n];  R = (1 / K) sum_k X[k] X[k]^H  (N x N)
 *            every index lies inside the window: no halo, no read outside the trace
 *   loading  t = sum_i Re R_ii;  R' = R + delta (t / N) I
 *   values   P_B(g) = Re(a^H R a) / N^2  on the unloaded R;  R' = L L^H (Cholesky), L y = a, P_C(g) = 1 / |y|^2.  For one
 *            wave of power sigma^2 both read about sigma^2 at its slowness.
 *   outputs  capon_index (int32): the g with the largest P_C under the total order "P descending, g ascending"; NaN is no
 *            candidate; -1 if there is none.  capon_power = P_C there (NaN for -1).  bartlett_index / bartlett_power: the
 *            same for P_B.  On request both maps [G] and R [N][N] complex (re, im interleaved).
 *   degenerate  t == 0, t NaN or a NaN entry of R: every result NaN / -1 (R itself is returned as computed).  A Cholesky
 *            pivot that is not > 0: the Capon results NaN / -1, the Bartlett results stay.
 * With delta > 0 the condition number of R' is at most (N + delta) / delta.  The order of every sum depends on (N, W, Ls, Hs,
 * G) alone, the arg-max is a total order and no atomics are used: single, streamed, batched (nbls_set_segments) and
 * window-sliced passes agree bit for bit.
 *   nbls_set_capon(h, grid, G, freq, snap_len, snap_hop, nbands, loading, flags)   copied and read by the next nbls_plan;
 *                            G = 0 (or grid NULL) switches it off (the default: a plan without it is launch for launch the
 *                            plain pass).  flags: NBLS_CAPON_MAPS, NBLS_CAPON_CSDM.  NBLS_ERR_ARG, the handle unchanged, for
 *                            G outside 1..65536, an entry of the grid that is not finite, a frequency not in (0, inf), a
 *                            length or hop < 1, a loading < 0 or not finite, nbands < 1.  nbls_plan returns NBLS_ERR_ARG if
 *                            nbands differs from the plan's, if some Ls_b > W_b, or if delta = 0 with some K_b < N (singular
 *                            by construction); NBLS_ERR_STATE without the geometry of the trace's array;
 *                            NBLS_ERR_UNSUPPORTED with an RCCL communicator, for more than 32 elements, and if the steering
 *                            table nbands * G * N * 16 bytes exceeds 1 GiB.  The search is over the full array, behind
 *                            estimator 0's solve; it is independent of nbls_set_beam_grid / nbls_set_lag_seed and combines
 *                            with them, with segments, streamed results and window ranges.
 *   nbls_fetch_capon(h, capon_index, capon_power, bartlett_index, bartlett_power)   [rows][vector_len] each (any may be NULL),
 *                            rows as for nbls_fetch; waits for the pass like nbls_fetch_beam_grid.
 *   nbls_fetch_capon_maps(h, capon_map, bartlett_map)   [rows][vector_len][G] each (either may be NULL).
 *   nbls_fetch_capon_csdm(h, R)   [rows][vector_len][N][N][2].
 *   nbls_fetch_capon_tables(h, band, coef, steer)   the plan's own tables of band `band`: coef [Ls_b][2], steer [G][N][2]
 *                            (either may be NULL).
 *                            Each returns NBLS_ERR_STATE where the plan did not ask for the result.  The results are
 *                            written by the solve stage alone: zeros until a pass of the plan has run it; cells beyond
 *                            nwin[r] (and outside a window slice) are zeros.
 * A workgroup of NBLS_CAPON_THREADS threads takes one unit; the snapshots go through LDS NBLS_CAPON_CHUNK at a time.
 * nbls_timings is unchanged: the kernel's time falls inside the solve interval. */
#define NBLS_CAPON_GRID_MAX 65536
#define NBLS_CAPON_MAX_ELEMENTS 32
#define NBLS_CAPON_THREADS 128
#define NBLS_CAPON_CHUNK 32
#define NBLS_CAPON_MAPS 1
#define NBLS_CAPON_CSDM 2
int nbls_set_capon(nbls_handle* h, const double* grid, int32_t G, const double* freq, const int32_t* snap_len,
                   const int32_t* snap_hop, int32_t nbands, double loading, int32_t flags);
int nbls_fetch_capon(nbls_handle* h, int32_t* capon_index, double* capon_power, int32_t* bartlett_index, double* bartlett_power);
int nbls_fetch_capon_maps(nbls_handle* h, double* capon_map, double* bartlett_map);
int nbls_fetch_capon_csdm(nbls_handle* h, double* R);
int nbls_fetch_capon_tables(nbls_handle* h, int32_t band, double* coef, double* steer);

/* The K strongest arrivals of either spectrum: a plan with Capon spectra may also carry a peak
 * request, and its kernel then picks the local maxima of both maps where they are complete, instead of the caller
 * fetching [rows][vector_len][G] doubles per map to do it on the host.
 *   request  cell[G][2] (int32): the lattice coordinates of the G grid points, distinct, 0 <= c < 32768, G that of
 *            nbls_set_capon when the plan is made; a count 1 <= K <= 8 (NBLS_CAPON_PEAKS_MAX); a relative floor in [0, 1].
 *            The library builds the neighbour table once per request, [8][G] on the device: the neighbours of g are the
 *            points at cell(g) + (di, dj) in the fixed order (-1,0), (+1,0), (0,-1), (0,+1), (-1,-1), (-1,+1), (+1,-1),
 *            (+1,+1); an absent neighbour is -1.
 * For one unit and one spectrum P, each of the two on its own:
 *   order    better(p, g; q, n): P descending, g ascending (the order of capon_index).
 *   peak     g is a peak iff P[g] is not NaN and better(P[g], g; P[n], n) holds for every neighbour n >= 0 with P[n] not
 *            NaN.  A NaN or absent neighbour does not compete; of equal neighbours the one with the smaller index wins.
 *            The spectrum's arg-max is always a peak.
 *   kept     the arg-max is kept; another peak iff floor == 0 or P[g] >= floor * P[argmax] (one double multiplication).
 *            count is the number of kept peaks; it is not capped at K.
 *   ranks    ranks k < min(count, K) hold the kept peaks in that order: index[k], power[k] = P[index[k]].  Rank 0 equals
 *            capon_index / capon_power (bartlett_*) bit for bit.  Further ranks: index -1, power NaN, offset NaN.
 *   offset   offset[k][axis] in lattice steps, positive towards the +1 neighbour: with m and p the -1 and +1 neighbours of
 *            index[k] on that axis, 0.5 (P[m] - P[p]) / ((P[m] - 2 P[g]) + P[p]); 0 unless all three values are finite,
 *            the denominator is < 0 and the quotient is finite; clamped to +-0.5, -0.0 becomes 0.0; 0 where m or p is
 *            absent.  It is the rule of the lag refinement (nbls_set_lag_refinement).
 *   degenerate  every Capon and Bartlett result NaN / -1: count 0, nothing kept.  A Cholesky pivot not > 0: the Capon peaks
 *            are empty, the Bartlett peaks stay.
 * No atomics, every order total, nothing depends on the launch's unit range: single, streamed, batched and window-sliced
 * passes, and both routes below, give the same bits.
 *   nbls_set_capon_peaks(h, cell, G, K, floor)   copied and read by the next nbls_plan; cell NULL or K = 0 switches it off
 *                            (the default: such a plan launches exactly what it launched before).  NBLS_ERR_ARG, the handle
 *                            unchanged, for K outside 1..8, G outside 1..65536, a floor outside [0, 1] or NaN, a coordinate
 *                            out of range, two equal cells.  nbls_plan returns NBLS_ERR_ARG for a peak request without Capon
 *                            spectra or with another G.
 *   nbls_fetch_capon_peaks(h, which, count, index, power, offset)   which: 0 Capon, 1 Bartlett.  count [rows][vector_len],
 *                            index and power [rows][vector_len][K], offset [rows][vector_len][K][2]; any may be NULL.  Rows,
 *                            waiting, NBLS_ERR_STATE and the zeros beyond nwin[r] as for nbls_fetch_capon.
 * The unit's two maps wait for the pick either in LDS behind the kernel's own (the LDS route; [2][G] doubles must fit a
 * workgroup's 160 KiB) or in HBM (the HBM route): in the unit's rows of the maps if the plan keeps them (NBLS_CAPON_MAPS), else
 * in one of S slabs of a scratch buffer the handle owns, the units issued in launches of at most S.  Both routes run the same
 * code on the same values.  nbls_set_option keys, read by the next plan:
 *   "capon_peak_route" 0 automatic (LDS where the maps fit without lowering the workgroups per CU, else HBM), 1 LDS
 *                      (NBLS_ERR_UNSUPPORTED from nbls_plan where it does not fit), 2 HBM;
 *   "capon_peak_slabs" S = 1..4096; 0, the default: as many as 256 MiB hold, at least 256 (256 MiB at G = 65536), at most 4096. */
#define NBLS_CAPON_PEAKS_MAX 8
int nbls_set_capon_peaks(nbls_handle* h, const int32_t* cell, int32_t G, int32_t K, double floor);
int nbls_fetch_capon_peaks(nbls_handle* h, int32_t which /* 0 Capon, 1 Bartlett */,
                           int32_t* count, int32_t* index, double* power, double* offset);

/* ---- Beam and Capon results on the elements LTS kept ----
 * FAST-LTS finds the mistimed or noisy element of a window and takes the weight of its pairs; the beam of nbls_set_beam and
 * the spectra of nbls_set_capon still sum over the whole array.  On request the plan works out, per window, which elements
 * LTS has dropped, and those results are formed over the elements it kept.  The geometry must be the full lexicographic
 * pair list of the trace's array (as for nbls_set_closure); k(a, b) is the index of pair (a, b), a < b, in it.  For
 * estimator 0, the unit of result row r and window w, N elements and the weights w_k exactly as nbls_fetch returns them:
 *   count    c_m = the number of pairs k that hold element m and have w_k == 0.
 *   dropped  element m is dropped iff c_m >= q, q the request's min_pairs, 1 <= q <= N - 1 (N - 1: every pair of the
 *            element has lost its weight).
 *   outputs  dropped_mask uint32 [rows][vector_len], bit m set iff m is dropped; kept_count int32 [rows][vector_len] = M.
 *   kept set e_0 < ... < e_{M-1}, the complement of the dropped set; if fewer than 3 elements would remain, the kept set
 *            is the whole array (M = N) and dropped_mask still shows what the rule found.
 *   An OLS plan has every weight 1: its mask is 0 and M = N.  Cells beyond nwin[r] and outside a window slice are zeros.
 * NBLS_KEPT_BEAM: beam_power and fstat are nbls_set_beam's definition with N -> M, the elements e_i in ascending order,
 *   d_0 = 0 and d_i = rint(fs * (xij[k(e_0, e_i)] . z)): the reference element is the first kept one, z the solved slowness.
 * NBLS_KEPT_CAPON: R is formed, and with NBLS_CAPON_CSDM returned, for all N elements as before.  The spectra use
 *   R_K = R[e_i][e_j], t = sum_i Re R_K,ii, R' = R_K + delta (t / M) I, a_K[g][i] = a[g][e_i] (the plan's steering table,
 *   not re-referenced: both spectra are invariant to a common phase), P_B = Re(a_K^H R_K a_K) / M^2, and the M x M Cholesky
 *   factor and substitution with every loop in ascending i, j.  The degenerate rules of nbls_set_capon apply to R_K and t.
 *   The maps, the arg-max and the peak pick (nbls_set_capon_peaks, both routes) work on these spectra unchanged.
 * Where no element is dropped both are the plain plan's results bit for bit.  No atomics; every order depends on (N, the
 * kept set, W, ...) alone: single, streamed, batched and window-sliced passes give the same bits; full, bounded and seeded
 * lag picks are all accepted.
 *   nbls_set_kept_elements(h, min_pairs, flags)   read by the next nbls_plan; min_pairs = 0 switches it off (the default:
 *                            such a plan launches exactly what it launched before).  flags: NBLS_KEPT_BEAM, NBLS_KEPT_CAPON.
 *                            NBLS_ERR_ARG, the handle unchanged, for a negative min_pairs or unknown flags.  nbls_plan
 *                            returns NBLS_ERR_ARG for min_pairs > N - 1 (or N > 32), NBLS_ERR_STATE for a flag whose feature
 *                            the plan lacks (nbls_set_beam, nbls_set_capon) or a geometry that is not the full pair list,
 *                            NBLS_ERR_UNSUPPORTED with nbls_set_estimators (further estimators have kept sets of their
 *                            own: out of scope) and with an RCCL communicator.
 *   nbls_fetch_kept_elements(h, dropped_mask, kept_count)   either may be NULL.  Rows, waiting and zeros as for
 *                            nbls_fetch_closure; NBLS_ERR_STATE if the plan did not ask.  Written by the solve stage alone. */
#define NBLS_KEPT_BEAM 1
#define NBLS_KEPT_CAPON 2
int nbls_set_kept_elements(nbls_handle* h, int32_t min_pairs, int32_t flags);
int nbls_fetch_kept_elements(nbls_handle* h, uint32_t* dropped_mask, int32_t* kept_count);

/* ---- The beam trace at the windows' solved slowness ----
 * The pass describes every window (slowness, MdCCM, beam power, F ...); on request it also returns the waveform those
 * numbers describe: per result row one trace [npts], the delay-and-sum beam steered window by window at the slowness the
 * window solved, the overlapping windows stitched with a synthesis window.  For estimator 0, result row r (band b; with
 * segments r = b * nseg + s), N elements, window length W, hop inc, nwin[r] windows, the synthesis window g_b[0..W) of the
 * request's table, and M_w the kept count of window w (N without NBLS_BEAM_TRACE_KEPT).  For window w, s0 = w * inc, z the
 * solved slowness of its cell:
 *   delays   d_0 = 0, d_m = rint(fs * (xij[m-1][0] * z0 + xij[m-1][1] * z1)) for m > 0, ties to even; row m - 1 of the
 *            geometry is pair (0, m).  The delays are ALWAYS those against element 0's position, also where the kept set
 *            does not hold element 0: that takes the geometry alone, not element 0's samples.  NBLS_KEPT_BEAM re-references
 *            to the first kept element e_0; the trace does not, on purpose: consecutive windows of a stitched trace must
 *            share one time base.
 *   usable   window w is usable iff w < nwin[r], z0 and z1 are finite, |fs * (xij[m-1] . z)| < 2^30 for every m in 1..N-1
 *            (of the whole array) and, with the gate on, mdccm[cell] >= mdccm_min (a NaN MdCCM fails the gate).  The gate
 *            is off iff mdccm_min is NaN.
 *   elements all N; with NBLS_BEAM_TRACE_KEPT the kept set of nbls_set_kept_elements (bit m of dropped_mask[cell] clear,
 *            the whole array where fewer than 3 would remain), M_w = kept_count[cell].
 *   sum      s_w[t] = ((0.0 + x_a) + x_b) + ... over the set's elements in ascending m, x_m = filt[row of m][s0 + t + d_m],
 *            0.0 where the index is outside [0, npts): the padding up to npts_pad is never read as data.
 *   sample   n in [0, npts), over the usable windows with 0 <= n - s0 < W in ascending w, both sums from 0.0:
 *            acc = sum_w g_b[n - s0] * s_w[n - s0],  den = sum_w g_b[n - s0] * M_w,
 *            trace[r][n] = acc / den if den > 0, else 0.0.  One division per sample; a NaN sample read propagates.
 * Built without FMA contraction, no atomics; every order depends on (N, the kept set, W, inc) alone: single, streamed,
 * batched (nbls_set_segments) and band-round passes give the same bits, and the expression is a fixed sequence of IEEE
 * operations that NumPy float64 restates (tests/beam_trace_truth.py).  Full, bounded, seeded, refined, grid, Capon and
 * closure plans are accepted; the delays are the whole-sample ones of z in every case.
 *   nbls_set_beam_trace(h, window, nwindow, mdccm_min, flags)   read by the next nbls_plan.  window: the synthesis windows
 *                            of the plan's bands one after the other, sum_b W_b = nwindow doubles; NULL switches it off (the
 *                            default: such a plan launches exactly what it launched before).  flags: NBLS_BEAM_TRACE_KEPT.
 *                            NBLS_ERR_ARG, the handle unchanged, for a negative nwindow or unknown flags.  nbls_plan returns
 *                            NBLS_ERR_ARG if nwindow != sum_b W_b, an entry is negative or not finite or a band's window
 *                            is all zero, NBLS_ERR_STATE for NBLS_BEAM_TRACE_KEPT without nbls_set_kept_elements or a
 *                            geometry whose rows 0..N-2 are not the pairs (0, m), NBLS_ERR_UNSUPPORTED with
 *                            nbls_set_window_ranges, nbls_set_estimators or an RCCL communicator.
 *   nbls_fetch_beam_trace(h, row, out)   out[npts] of result row `row`; waits for the pass as nbls_fetch_beam does.
 *                            NBLS_ERR_STATE if the plan did not ask, NBLS_ERR_ARG for a bad row.  Zeros until a pass of
 *                            this plan has run the solve stage; a later pass without it leaves the trace as it is.
 * One launch per pass, behind the last solve; streamed result batches do not carry the trace. */
#define NBLS_BEAM_TRACE_KEPT 1
int nbls_set_beam_trace(nbls_handle* h, const double* window /* concatenated per band; NULL = off */, int64_t nwindow,
                        double mdccm_min, int32_t flags);
int nbls_fetch_beam_trace(nbls_handle* h, int32_t row, double* out /* [npts] */);

/* ---- Steering at fractional-sample delays ----
 * The beam at the solved slowness (nbls_set_beam, section 12) and the slowness-grid search (nbls_set_beam_grid, section 15)
 * shift the elements by whole samples, d = rint(tau).  On request they read every element at the delay tau itself through a
 * Lagrange interpolator of L = taps samples.  K = L / 2, k runs over -K+1 .. K:
 *   tau_i    fs * (xij[row][0] * z0 + xij[row][1] * z1), un-fused, the expression and the pair row of sections 12 / 15 / 20
 *            (the kept-elements beam re-references as it does today); the reference element has tau = 0.  |tau| >= 2^30 or
 *            NaN: the unit's beam results are NaN, a grid plan is refused, as without interpolation.
 *   n_i, mu  n_i = floor(tau_i), mu_i = tau_i - n_i in [0, 1) (exact below 2^30).
 *   c_k(mu)  (((1.0 * (mu - j_1)) * (mu - j_2)) * ...) / D_k, the j ascending over -K+1 .. K without k, D_k = prod_{j != k}
 *            (k - j) an exact integer: L - 1 subtractions, L - 1 products, one division.  mu = 0: c_0 = 1.0, every other
 *            coefficient exactly +-0.
 *   x_i[t]   ((0.0 + c_{-K+1} * y_{-K+1}) + ...) + c_K * y_K,  y_k = filt[e_i][s0 + t + n_i + k], 0.0 where the index is
 *            outside [0, npts).  Every product is rounded before its addition (no contraction); a zero coefficient is still
 *            multiplied, so a NaN sample propagates.
 * b[t], S_b, S_t, D, F, P, the +-inf / NaN rules, the arg-max order and every reduction order are those of sections 12 and
 * 15.  Where every tau is an integer an interpolated plan returns the whole-sample plan's bits.  A fixed sequence of IEEE
 * operations that NumPy float64 restates (tests/steer_truth.py).  The beam trace (section 21) keeps whole-sample delays.
 *   nbls_set_beam_interpolation(h, taps)   read by the next nbls_plan; 0 switches it off (the default: such a plan launches
 *                            exactly what it launched before), 4, 6 or 8 taps.  NBLS_ERR_ARG, the handle unchanged, for
 *                            anything else.  nbls_plan returns NBLS_ERR_STATE if it is on and the plan asks for neither
 *                            nbls_set_beam nor nbls_set_beam_grid.  Every estimator's beam (nbls_est_fetch_beam), the
 *                            kept-elements beam and the grid of a seeded plan follow it.
 *   nbls_fetch_beam_grid_delays   of an interpolated grid plan returns n[G][N] (floor, not rint).
 *   nbls_fetch_beam_grid_coefficients(h, c)   the plan's table c[G][N][taps], k ascending; NBLS_ERR_STATE without an
 *                            interpolated grid plan. */
int nbls_set_beam_interpolation(nbls_handle* h, int32_t taps);
int nbls_fetch_beam_grid_coefficients(nbls_handle* h, double* c /* [G][N][taps] */);

/* ---- Each element's delay against the beam of the others ----
 * The pass can say that an element is wrong (its pairs lose their weight, nbls_set_kept_elements names it); on request it
 * also says by how much: per window and element the whole-sample shift, within +-K of the modelled delay, at which the
 * element correlates best with the beam of the other elements, the correlation there and the delay in seconds with a
 * parabola fraction.  For estimator 0, the unit of result row r (band b; with segments r = b * nseg + s) and window w,
 * s0 = w * inc, window length W, N = nelem, z the cell's solved slowness as nbls_fetch returns it, K = max_shift[b]:
 *   model    tau_0 = 0, tau_m = fs * (xij[m-1][0] * z0 + xij[m-1][1] * z1), un-fused; d_m = rint(tau_m), ties to even.  The
 *            delays are always those against element 0's position, as in the beam trace: row m - 1 of the geometry is pair
 *            (0, m).  The sign is nbls_set_beam's: element m is read at +d_m.
 *   bad unit z0 or z1 not finite, or some |tau_m| >= 2^30 over the whole array: delay and cc are NaN and shift is 0 for
 *            every element.
 *   samples  y_m(k)[t] = filt[row of m][s0 + t + d_m + k] for t in [0, W), k in [-K, K]; 0.0 where the index is outside
 *            [0, npts).  The +-K samples beside the window are real trace samples, not zero padding.
 *   set S    all N elements; with NBLS_ELEMENT_DELAY_KEPT the kept set of nbls_set_kept_elements: the clear bits of
 *            dropped_mask[cell], the whole array where fewer than 3 elements would remain.
 *   beam     b[t] = ((0.0 + y_a(0)[t]) + y_b(0)[t]) + ... over S in ascending element order;
 *            b_m[t] = b[t] - y_m(0)[t] if m is in S, b[t] otherwise: a dropped element is measured against the clean beam
 *            of the others, and every element, dropped or not, gets results.
 *   sums     E_b,m = sum_t b_m[t]^2,  E_m(k) = sum_t y_m(k)[t]^2,  C_m(k) = sum_t y_m(k)[t] * b_m[t],
 *            c_m(k) = C_m(k) / sqrt(E_m(k) * E_b,m).  Plain IEEE: a dead channel or an all-zero beam gives 0/0 = NaN, a NaN
 *            sample propagates.
 *   pick     k* = the k with the largest c_m(k) under the total order "c descending, |k| ascending, k ascending"; NaN is
 *            no candidate; with no candidate shift = 0, cc = NaN, delay = NaN.
 *   fraction frac = the rule of refine_fraction.h on (c_m(k*-1), c_m(k*), c_m(k*+1)): 0.5 (rm - rp) / ((rm - 2 r0) + rp)
 *            clamped to [-1/2, 1/2], 0 unless the three are finite and the denominator < 0; 0 where |k*| == K (so K = 0
 *            always gives 0).
 *   outputs  shift[m] = k*, cc[m] = c_m(k*), delay[m] = ((((double)(d_m + k*)) + frac) - tau_m) / fs in seconds: positive
 *            when element m records the beam's waveform later than a plane wave of slowness z predicts.  Subtracting tau_m
 *            rather than d_m takes the half-sample rounding of the steering out of the result.  Cells beyond nwin[r] and
 *            outside a window slice are zeros.
 * Built without FMA contraction, no atomics; the order of every sum depends on (N, S, W, K) alone and nothing on the
 * launch's unit range: single, streamed (overlap on and off), batched, window-sliced and band-round passes give the same
 * bits, and so do the two forms of the kernel (staged in LDS / global memory; option "element_delay_form": 0 automatic,
 * 1 staged — NBLS_ERR_UNSUPPORTED from nbls_plan where a row's block does not fit —, 2 global).
 *   nbls_set_element_delays(h, max_shift, nbands, flags)   copies the table; read by the next nbls_plan.  max_shift NULL
 *                            switches it off (the default: such a plan launches exactly what it launched before).
 *                            NBLS_ERR_ARG, the handle unchanged, for nbands < 1, an entry outside
 *                            0..NBLS_ELEMENT_DELAY_MAX_SHIFT or unknown flags.  nbls_plan returns NBLS_ERR_ARG if nbands
 *                            differs from the plan's or N > 32, NBLS_ERR_STATE without a geometry whose rows 0..N-2 are
 *                            the pairs (0, m) or for NBLS_ELEMENT_DELAY_KEPT without nbls_set_kept_elements,
 *                            NBLS_ERR_UNSUPPORTED with nbls_set_estimators or an RCCL communicator.  Segments, window
 *                            ranges, streamed results, bounded, seeded and refined picks, beam, grid, Capon, closure and
 *                            beam trace are accepted, and so is nbls_set_beam_interpolation: this feature keeps the
 *                            whole-sample d_m whatever the taps are, the fraction is its own.
 *   nbls_fetch_element_delays(h, delay, cc, shift)   [rows][vector_len][nelem] each, any may be NULL; waits for the pass as
 *                            nbls_fetch_beam does.  NBLS_ERR_STATE if the plan did not ask; zeros until a pass of this plan
 *                            has run the solve stage.
 *   nbls_element_delay_lds_bytes(nelem, W, max_shift)   pure host function: (nelem * (W + 2 max_shift) + W) * 8, the
 *                            staged form's rows and b[W], where that is at most 156 KiB; 0: the global form.
 *                            NBLS_ERR_ARG for nelem < 1, W < 1 or max_shift outside 0..NBLS_ELEMENT_DELAY_MAX_SHIFT.
 * The kernel runs behind every solve of estimator 0 (behind the kept elements' mask), over the solve's unit range. */
#define NBLS_ELEMENT_DELAY_KEPT 1          /* beam over the elements LTS kept */
#define NBLS_ELEMENT_DELAY_MAX_SHIFT 256
int nbls_set_element_delays(nbls_handle* h, const int32_t* max_shift /* [nbands]; NULL = off */, int32_t nbands, int32_t flags);
int nbls_fetch_element_delays(nbls_handle* h, double* delay, double* cc, int32_t* shift);   /* [rows][vector_len][nelem] each; any may be NULL */
int nbls_element_delay_lds_bytes(int32_t nelem, int32_t W, int32_t max_shift);              /* pure host function, like nbls_beam_grid_lds_bytes */

/* ---- A window's arrivals and their powers by CLEAN-SC ----
 * A Bartlett peak list is mostly sidelobes and a Capon power depends on the loading.  CLEAN-SC (Sijtsma 2007) takes the
 * Bartlett maximum of R, removes from R everything coherent with that beam, and repeats on the residual; it needs no
 * loading, no factor and no point-spread model, and the residual stays positive semidefinite.  A plan with nbls_set_capon
 * may carry a CLEAN request: iterations 1 <= I <= 32 (NBLS_CAPON_CLEAN_MAX), a gain phi in (0, 1], a floor f in [0, 1),
 * flags (NBLS_CLEAN_RESIDUAL).  It applies to estimator 0 and uses the grid, the steering table a[g], R and the units of
 * nbls_set_capon; with NBLS_KEPT_CAPON it uses R_K and the kept rows of a exactly as the spectra do, M in the place of N.
 * Per unit, R_0 = R:
 *   degenerate  (t = 0, t NaN or a NaN entry, as for the spectra) count = 0, every rank -1 / NaN, total and residual NaN.
 *   total    t_0 / N,  t_0 = sum_i Re R_0,ii in ascending i.
 *   scan     iteration i = 0 .. I-1: P_i(g) is the Bartlett spectrum of nbls_set_capon on R_i, the same operations in the
 *            same order as the spectra's kernel; g_i its arg-max under "P descending, g ascending" (NaN is no candidate),
 *            p_i = P_i(g_i).
 *   stop     count = i if there is no candidate, if p_i > 0 is not true, or if i > 0 and p_i < f * p_0 (one
 *            multiplication).
 *   update   with a = a[g_i], every sum from 0 in ascending index, fma(x, y, z) = x * y + z rounded once:
 *            v_j:  vr = fma(Rr_jk, ar_k, vr); vr = fma(-Ri_jk, ai_k, vr); vi = fma(Rr_jk, ai_k, vi); vi = fma(Ri_jk, ar_k, vi)
 *                  over k  (v = R_i a)
 *            q:    q = fma(ar_j, vr_j, q); q = fma(ai_j, vi_j, q)  over j  (q = Re(a^H v))
 *            count = i if q > 0 is not true or q is not finite;  s = phi / q
 *            for j >= k:  wr = fma(vi_j, vi_k, vr_j * vr_k);  wi = fma(vi_j, vr_k, -(vr_j * vi_k))   (w = v_j conj(v_k))
 *                  Re R_{i+1},jk = fma(-wr, s, Re R_i,jk);  Im R_{i+1},jk = fma(-wi, s, Im R_i,jk)
 *            the imaginary part of the diagonal is 0.0 and the upper triangle the conjugate, bit for bit
 *            index[i] = g_i, power[i] = phi * p_i
 *   count    I where no rule fired; ranks at or beyond count are -1 / NaN.
 *   residual sum_i Re R_count,ii / N (M with the kept elements), ascending i.
 *   NBLS_CLEAN_RESIDUAL  R_count is kept, [N][N][2]; with the kept elements it is scattered back to the elements' own rows
 *            and columns, zeros for the dropped ones.  A degenerate unit returns its R_0.
 * Rank 0 is bartlett_index, and power[0] == phi * bartlett_power, bit for bit.  The results of a plan with I' < I are the
 * first I' ranks of the plan with I, count = min(count, I').  In exact arithmetic R_i stays positive semidefinite and its
 * trace does not grow.  No atomics, every order total, nothing depends on the launch's unit range: single, streamed,
 * batched, window-sliced and round-split passes give the same bits.
 *   nbls_set_capon_clean(h, iterations, gain, floor, flags)   read by the next nbls_plan; 0 iterations switches it off (the
 *                            default: such a plan launches exactly what it launched before).  NBLS_ERR_ARG, the handle
 *                            unchanged, for iterations outside 0..32, a gain outside (0, 1], a floor outside [0, 1), NaN, or
 *                            unknown flags.  nbls_plan returns NBLS_ERR_STATE without nbls_set_capon; whatever nbls_set_capon
 *                            refuses stays refused.  It combines with the maps, the peaks on either route, the kept
 *                            elements, segments, window ranges and streamed results.
 *   nbls_fetch_capon_clean(h, count, index, power, total, residual)   count, total, residual [rows][vector_len]; index and
 *                            power [rows][vector_len][I]; any may be NULL.  Rows, waiting, NBLS_ERR_STATE and zeros as for
 *                            nbls_fetch_capon.
 *   nbls_fetch_capon_clean_csdm(h, R)   [rows][vector_len][N][N][2]; NBLS_ERR_STATE without NBLS_CLEAN_RESIDUAL.
 *   nbls_capon_clean_lds_bytes(nelem)   pure host function: (2 N^2 + 2 N + 2 * 128 * N) * 8, the kernel's dynamic LDS (R, v
 *                            and a column of a per lane); NBLS_ERR_ARG for nelem outside 1..32.
 * capon_clean_kernel (csrc/capon_clean.hip) runs behind the spectra's kernel on the same stream over the same units, one
 * workgroup of NBLS_CAPON_THREADS per unit; it reads R from the plan's matrix buffer, which such a plan holds on the device
 * whether or not NBLS_CAPON_CSDM was asked.  nbls_timings is unchanged. */
#define NBLS_CAPON_CLEAN_MAX 32
#define NBLS_CLEAN_RESIDUAL 1
int nbls_set_capon_clean(nbls_handle* h, int32_t iterations, double gain, double floor, int32_t flags);
int nbls_fetch_capon_clean(nbls_handle* h, int32_t* count, int32_t* index, double* power, double* total, double* residual);
int nbls_fetch_capon_clean_csdm(nbls_handle* h, double* R);
int nbls_capon_clean_lds_bytes(int32_t nelem);

/* ---- A window's eigenvalues and its MUSIC slowness spectrum ----
 * The eigenvalues of R say whether a window holds one arrival or several; the MUSIC pseudo-spectrum (Schmidt 1986)
 * separates them with one scan of the grid.  A plan with nbls_set_capon may carry a MUSIC request: sources, an eigenvalue
 * floor rho, a peak floor, flags (NBLS_MUSIC_MAP, NBLS_MUSIC_VECTORS, NBLS_MUSIC_PEAKS).  It applies to estimator 0 and uses the grid, the
 * steering table a[g], the units and the unloaded R of nbls_set_capon, the matrix NBLS_CAPON_CSDM returns; the loading plays
 * no part.  N is the full array, 3 <= N <= 32.  fma(x, y, z) = x * y + z rounded once.  Per unit, A = R, E = I:
 *   degenerate  (t = 0, t NaN or a NaN entry of R, as for the spectra) every eigenvalue NaN, sources -1, sweeps 0, index
 *            -1, power NaN, the map and the vectors NaN.
 *   order    cyclic Jacobi in the round-robin tournament order: with H = ceil(N / 2) and m = 2 H - 1, step k = 0 .. m - 1
 *            rotates the disjoint pairs {m, k} and {(k + r) mod m, (k - r) mod m}, r = 1 .. H - 1, p the smaller and q
 *            the larger index; a pair with the player N of an odd array is the other's bye.  m steps are one sweep: every
 *            pair once, the order independent of the data.
 *   rotation of the pair (p, q) from x = A_pq, g = sqrt(fma(Im x, Im x, Re x * Re x)):  g = 0: none.  Otherwise
 *            tau = (A_qq - A_pp) / (2 g);  t = sign(tau) / (|tau| + sqrt(fma(tau, tau, 1)))  (sign(+-0) = +-1);
 *            c = 1 / sqrt(fma(t, t, 1));  s = t * c;  sigma = s * (x / g)  (each part divided, then multiplied).
 *            J is the identity but for J_pp = J_qq = c, J_pq = sigma, J_qp = -conj(sigma).
 *   step     A <- J^H A J and E <- E J with J the product of the step's rotations, all formed from the A before the step.
 *            A_pp <- A_pp - t g, A_qq <- A_qq + t g, A_pq = A_qp = 0, the imaginary part of the diagonal 0.0.  Of the other
 *            entries the 2 x 2 blocks X = A[{p, q}][{p', q'}] of the pairs r < r' are computed, X J' first and J^H (X J')
 *            second, each product a chain of fma from the product with c; the entries below are their conjugates, bit
 *            for bit.
 *   stop     before every sweep:  off^2 = sum_{i > j} |A_ij|^2 (fma chain, rows ascending) and n^2 = sum_ij |R_ij|^2
 *            (likewise, storage order);  stop if 2 off^2 <= 2^-92 n^2, that is off(A) <= 2^-46 ||R||_F, or after
 *            NBLS_MUSIC_SWEEP_CAP = 24 sweeps.  sweeps is the number of sweeps made; a diagonal R takes 0.  Fewer than
 *            the cap means the rule fired.
 *   eigenvalues  lambda_1 >= ... >= lambda_N: the diagonal of A under the total order "value descending, then the
 *            column's index before sorting ascending"; e_k is the column of E that belongs to lambda_k.
 *   sources  M = sources where 1 <= sources <= N - 1;  sources = 0:  M = clamp(#{k : lambda_k >= rho * lambda_1}, 1, N - 1),
 *            one multiplication, decided from the returned eigenvalues: the returned M is reproducible from them bit for bit.
 *   spectrum D(g) = (1 / N) sum_{k > M} |e_k^H a(g)|^2, k ascending and inside each k the elements ascending:
 *            zr = fma(Re e_ik, Re a_i, zr); zr = fma(Im e_ik, Im a_i, zr); zi = fma(Re e_ik, Im a_i, zi);
 *            zi = fma(-Im e_ik, Re a_i, zi);  then d = fma(zr, zr, d); d = fma(zi, zi, d);  P(g) = 1 / (d / N).  The noise
 *            subspace is summed, not N minus the signal subspace: nothing cancels where D -> 0.  D = 0 gives +inf, which
 *            is a candidate.
 *   arg-max  music_index / music_power under "P descending, g ascending", NaN no candidate, as for the spectra.
 *   NBLS_MUSIC_MAP      the plan keeps P, [G] per unit.
 *   NBLS_MUSIC_VECTORS  the plan keeps E, [N][N][2] per unit, entry [i][k] element i of e_k; its phase is unspecified.
 *   NBLS_MUSIC_PEAKS    the K strongest local maxima of P as nbls_set_capon_peaks defines them for a spectrum: K and the
 *            neighbour table are that request's, which the plan must carry (NBLS_ERR_STATE without it); the floor is this
 *            request's own peak_floor, since a pseudo-spectrum's heights are not powers; count, index, power and offset as
 *            there.  +inf is a local maximum like any other value; a degenerate unit has count 0 and every rank -1 / NaN.
 * No atomics, every order total, nothing depends on the launch's unit range: single, streamed, batched, window-sliced and
 * round-split passes give the same bits.
 *   nbls_set_capon_music(h, sources, eig_floor, peak_floor, flags)   read by the next nbls_plan; sources = -1 switches it
 *                            off (the default: such a plan launches exactly what it launched before).  NBLS_ERR_ARG, the
 *                            handle unchanged, for sources outside -1..31, with sources = 0 an eig_floor outside (0, 1), a
 *                            peak_floor outside [0, 1), NaN, or unknown flags.  nbls_plan returns NBLS_ERR_STATE without nbls_set_capon,
 *                            NBLS_ERR_ARG for sources > N - 1, and NBLS_ERR_UNSUPPORTED for fewer than 3 elements, with an
 *                            RCCL communicator, with further estimators (nbls_set_estimators) and with NBLS_KEPT_CAPON.
 *                            It combines with the maps, the peaks, CLEAN-SC, segments, window ranges and streamed results.
 *   nbls_fetch_capon_music(h, eigenvalues, sources, sweeps, index, power)   eigenvalues [rows][vector_len][N]; the others
 *                            [rows][vector_len]; any may be NULL.  Rows, waiting, NBLS_ERR_STATE and zeros as for
 *                            nbls_fetch_capon.
 *   nbls_fetch_capon_music_map(h, map)   [rows][vector_len][G]; NBLS_ERR_STATE without NBLS_MUSIC_MAP.
 *   nbls_fetch_capon_music_vectors(h, E)   [rows][vector_len][N][N][2]; NBLS_ERR_STATE without NBLS_MUSIC_VECTORS.
 *   nbls_fetch_capon_music_peaks(h, count, index, power, offset)   count [rows][vector_len], index and power [..][K], offset
 *                            [..][K][2]; any may be NULL; NBLS_ERR_STATE without NBLS_MUSIC_PEAKS.  nbls_fetch_capon_peaks
 *                            keeps its `which` of 0 and 1.
 *   nbls_capon_music_lds_bytes(nelem)   pure host function: (4 N^2 + 2 * 128 * N + 4 N + 4) * 8, the kernel's dynamic LDS (A,
 *                            E, a column of a per lane, the step's rotations, the eigenvalues and their order);
 *                            NBLS_ERR_ARG for nelem outside 3..32.
 * capon_music_kernel (csrc/capon_music.hip) runs behind the spectra's kernel on the same stream over the same units, one
 * workgroup of NBLS_CAPON_THREADS per unit; it reads R from the plan's matrix buffer, which such a plan holds on the device
 * whether or not NBLS_CAPON_CSDM was asked.  nbls_timings is unchanged. */
#define NBLS_MUSIC_SWEEP_CAP 24
#define NBLS_MUSIC_STOP_SQUARED 0x1p-92
#define NBLS_MUSIC_MAP 1
#define NBLS_MUSIC_VECTORS 2
#define NBLS_MUSIC_PEAKS 4
int nbls_set_capon_music(nbls_handle* h, int32_t sources, double eig_floor, double peak_floor, int32_t flags);
int nbls_fetch_capon_music(nbls_handle* h, double* eigenvalues, int32_t* sources, int32_t* sweeps, int32_t* index, double* power);
int nbls_fetch_capon_music_map(nbls_handle* h, double* map);
int nbls_fetch_capon_music_vectors(nbls_handle* h, double* E);
int nbls_fetch_capon_music_peaks(nbls_handle* h, int32_t* count, int32_t* index, double* power, double* offset);
int nbls_capon_music_lds_bytes(int32_t nelem);

/* ---- A pass's windows grouped into detections: families ----
 * Every other result describes one (band, window) cell.  A family (after PMCC, Cansi 1995) is a set of cells of one recording
 * that neighbour each other in band and time and agree in back-azimuth and velocity: "this source, from about this
 * back-azimuth, between these times, in these bands".  Pure integer logic and a handful of IEEE compares.
 *   lattice   B bands, nseg recordings, result rows r = b * nseg + s, each a grid row of vector_len cells,
 *             cell = r * vector_len + w.  Band b has window length W_b and hop inc_b; window w starts at sample
 *             s0 = w * inc_b; its doubled centre is c2 = 2 * s0 + W_b (int64).
 *   request   nbls_family_params.  mdccm_min finite; vel_min <= vel_max, both finite; sigma_tau_max (NaN: that gate is off);
 *             baz_tol in [0, 180] degrees; vel_tol >= 0 km/s; band_reach in [0, 8]; time_reach in [1, 8]; min_pixels >= 1;
 *             flags 0.  Anything else is NBLS_ERR_ARG and leaves the handle unchanged.
 *   eligible  a cell with w < nwin[r]; vel, baz and mdccm finite; mdccm >= mdccm_min; vel_min <= vel <= vel_max; and, with
 *             the gate on, sigma_tau <= sigma_tau_max (a NaN fails the gate).
 *   link      two distinct eligible cells p = (b, s, w) and p' = (b', s', w') are linked iff
 *             1. s == s' (recordings never link);
 *             2. |b - b'| <= band_reach (band index of the plan);
 *             3. |c2 - c2'| <= 2 * time_reach * max(inc_b, inc_b') in integer arithmetic: within one band |w - w'| <= time_reach;
 *             4. d = |baz - baz'|, d = 360.0 - d if d > 180.0, then d <= baz_tol;  and |vel - vel'| <= vel_tol: plain
 *                float64 subtract, abs and compare (built without contraction).
 *   family    a connected component of the link graph with at least min_pixels cells; families are numbered 0 .. F - 1 in
 *             ascending order of their smallest cell.
 *   results   family [rows][vector_len] int32: the family id, -2 for an eligible cell whose component is too small, -1 for
 *             everything else;  nfamilies = F;  table int64 [F][8]: count | first_cell (the smallest cell) | peak_cell (the
 *             cell of the largest MdCCM, ties to the smallest cell; -0.0 == +0.0) | band_lo | band_hi | segment |
 *             sample_first (min s0) | sample_end (max s0 + W_b).
 * Everything is a function of the inputs alone: launch shape, batch seams and arrival order never change a bit.
 *   nbls_set_families(h, params)   read by the next nbls_plan; NULL switches it off (the default: such a plan launches exactly
 *                            what it launched before).  One launch sequence per pass, behind the last solve, on estimator 0's
 *                            result grids.  nbls_plan returns NBLS_ERR_UNSUPPORTED with window ranges (nbls_set_window_ranges),
 *                            with further estimators (nbls_set_estimators) and with an RCCL communicator; segments are
 *                            supported; streamed result batches do not carry families.
 *   nbls_fetch_families(h, family, nfamilies, table, capacity)   any pointer may be NULL; min(F, capacity) table rows are
 *                            filled.  Waits for the pass as nbls_fetch_beam does; NBLS_ERR_STATE without the request; -1
 *                            everywhere and F = 0 until a pass of the plan has run the solve stage.
 *   nbls_label_families(h, params, nbands, nseg, vector_len, winlen, wininc, nwin, vel, baz, mdccm, sigma_tau, family,
 *                            nfamilies, table, capacity)   the same kernels on grids the caller supplies (host pointers):
 *                            winlen and wininc [nbands], nwin [nbands * nseg], the grids [nbands * nseg][vector_len],
 *                            sigma_tau NULL iff the gate is off.  Uploads, labels and downloads synchronously on the handle's
 *                            device; needs no plan and changes none.  NBLS_ERR_ARG for rows * vector_len >= 2^31, a
 *                            non-positive winlen or wininc, nwin outside [0, vector_len], a sigma_tau that does not match
 *                            the gate.
 * families.hip: one thread per cell; a lock-free union-find (path halving, one compare-and-swap that hooks the larger root
 * under the smaller) whose every access to the parent array is an agent-scope relaxed atomic; integer add / min / max on the
 * root for the table; a three-kernel device-wide scan for the ids.  No wave waits for another.  nbls_timings is unchanged. */
typedef struct {
    double mdccm_min, vel_min, vel_max, sigma_tau_max, baz_tol, vel_tol;
    int32_t band_reach, time_reach, min_pixels, flags;
} nbls_family_params;
#define NBLS_FAMILY_COLUMNS 8
#define NBLS_FAMILY_MAX_REACH 8
int nbls_set_families(nbls_handle* h, const nbls_family_params* params /* NULL = off */);
int nbls_fetch_families(nbls_handle* h, int32_t* family, int32_t* nfamilies, int64_t* table, int64_t capacity);
int nbls_label_families(nbls_handle* h, const nbls_family_params* params, int32_t nbands, int32_t nseg, int32_t vector_len,
                        const int32_t* winlen, const int32_t* wininc, const int32_t* nwin, const double* vel, const double* baz,
                        const double* mdccm, const double* sigma_tau /* NULL iff the gate is off */, int32_t* family,
                        int32_t* nfamilies, int64_t* table, int64_t capacity);

/* ---- The grid maximum refined between grid points ----
 * The slowness-grid search (section 15) returns an index; steered at fractional-sample delays (section 22) F is a continuous
 * function of the slowness, so a coarse grid can find the lobe and a local search climb it.  The request needs a plan with a
 * beam grid and fractional-sample steering (taps L in {4, 6, 8}) and holds `levels` R in 1..12 and `step` (h0, h1) in s/km,
 * both finite and > 0; the usual step is the grid's lattice step.  For the unit of result row r and window w, over the full
 * array exactly as section 15 takes it:
 *   start    g* = grid_index.  g* = -1: slowness, fstat, power and stencil are NaN, every path entry is -1.
 *            Otherwise c = (grid[g*][0], grid[g*][1]), Fc = grid_fstat, Pc = grid_power (the grid kernel's own bits).
 *   level    l = 1 .. R:   e = (ldexp(h0, -l), ldexp(h1, -l))                  (exact: step * 2^-l)
 *            candidates j = 0 .. 8:  a = j / 3 - 1,  b = j % 3 - 1  (integer division)
 *                                    s_j = (c0 + a * e0,  c1 + b * e1)         (a * e exact, one rounded addition)
 *            j = 4 is the centre and is not evaluated again: F_4 = Fc, P_4 = Pc.
 *            j != 4: F_j, P_j = F and P of section 22 with z = s_j:
 *                    tau_i = fs * (xij[i-1][0] * s_j0 + xij[i-1][1] * s_j1) un-fused, tau_0 = 0, n = floor(tau), mu = tau - n,
 *                    the coefficients of section 22, the taps ascending, every product rounded before its addition.
 *                    b[t], S_b, S_t, D, the +inf and NaN rules, the mapping of t to lanes, and every reduction order
 *                    are those of the grid kernel for a grid point of that slowness.
 *            choose  j* = the best candidate under the order "F descending (+inf first); the centre before any other
 *                    candidate; then j ascending".  A NaN F is no candidate.  (Fc is never NaN when g* >= 0.)
 *            record  path[l-1] = j*.  On the last level stencil[j] = F_j for j = 0 .. 8, taken before the move.
 *            move    c = s_j*, Fc = F_j*, Pc = P_j*.  (j* = 4 leaves all three unchanged.)
 *   outputs  grid_refined_slowness (2 doubles) = c,  grid_refined_fstat = Fc,  grid_refined_power = Pc,
 *            grid_refined_path (R int32),  grid_refined_stencil (9 doubles).
 *            Cells beyond nwin[r] and outside a window slice are zeros.
 * So grid_refined_fstat >= grid_fstat, with equal bits where every path entry is 4; the slowness is what float64 gives when
 * it replays the path from grid[g*]; |c - grid[g*]| <= step (1 - 2^-R) on each axis; the first l entries of the path of an
 * R-level plan are the path of an l-level plan.  A candidate's F depends on (N, W, taps, s_j) alone: single, streamed, batched,
 * window-sliced and HBM-round passes agree bit for bit.  Estimator 0 only, as for the grid.  The coarse step must not exceed
 * the width of the main lobe: a grid that misses the lobe gives the search nothing to climb.
 *   nbls_set_beam_grid_refinement(h, levels, step)   read by the next nbls_plan; levels = 0 or step = NULL switches it off (the
 *                            default: such a plan launches exactly what it launched before).  NBLS_ERR_ARG, the handle
 *                            unchanged, for levels outside 0..12 or a step that is not finite and > 0.  The plan derives one
 *                            halo H_r = grid_halo + ceil(fs max_i(|xij[i][0]| h0 + |xij[i][1]| h1)) + 1 over the pairs (0, i)
 *                            and uses it everywhere; nbls_plan returns NBLS_ERR_ARG if H_r reaches 2^30, NBLS_ERR_STATE if
 *                            the refinement is on without a grid or without interpolation, NBLS_ERR_UNSUPPORTED with a lag
 *                            seed (nbls_set_lag_seed: the seed keeps the unrefined maximum) and with an RCCL communicator.
 *                            One launch behind the grid search of every unit batch.
 *   nbls_fetch_beam_grid_refined(h, slowness, fstat, power, path, stencil)   [rows][vector_len][2] | [rows][vector_len] twice |
 *                            [rows][vector_len][R] int32 | [rows][vector_len][9]; any may be NULL.  Waits for the pass like
 *                            nbls_fetch_beam; NBLS_ERR_STATE if the plan did not ask; zeros until a pass of the plan has run
 *                            the solve stage.
 *   nbls_beam_grid_refine_lds_bytes(nelem, W, halo)   a pure host function, like nbls_beam_grid_lds_bytes: the dynamic LDS
 *                            of the staged form, nelem * (W + 2 halo) * 8 bytes where that is at most 156 KiB, else 0: the
 *                            form that reads the filtered band from global memory.  Both give the same bits.  NBLS_ERR_ARG
 *                            for nelem < 1, W < 1 or halo < 0. */
#define NBLS_BEAM_GRID_REFINE_MAX_LEVELS 12
int nbls_set_beam_grid_refinement(nbls_handle* h, int32_t levels /* 0 = off */, const double* step /* [2]; NULL = off */);
int nbls_fetch_beam_grid_refined(nbls_handle* h, double* slowness, double* fstat, double* power, int32_t* path, double* stencil);
int nbls_beam_grid_refine_lds_bytes(int32_t nelem, int32_t W, int32_t halo);

/* Copy the filtered+tapered trace of planned band `band` to host: out[nchans][npts]. */
int nbls_fetch_filtered(nbls_handle* h, int32_t band, double* out);

/* ---- time-segmented filtering (a band whose filtered trace does not fit the HBM budget) ----
 * The trace is fed in consecutive time segments (nbls_set_trace per segment, nbls_plan for its length); the IIR state
 * is handed from segment to segment, so the output equals the whole-trace filter (helpers.py:124-139) up to the
 * rounding of the carried states.
 *   nbls_filter_segment(h, reverse, state_in, state_out)
 *       reverse = 0: ONE causal pass over the resident raw segment, forward in time, into the filtered buffer;
 *       reverse = 1: one causal pass over the filtered buffer IN PLACE, backward in time (the second half of a
 *       zero-phase filter: feed the forward outputs back with nbls_set_filtered, last segment first).
 *       state_in / state_out: [nbands][nchans][2 * nsections] DF2T states entering the segment / leaving its last
 *       whole 512-sample chunk (NULL = zero state / not wanted).  A segment that hands a state on must be a multiple
 *       of 512 samples long (every segment but the last in time).  No taper is applied: the caller multiplies the
 *       whole-trace taper in at global sample positions.
 *   nbls_set_filtered(h, band, data[nchans][npts])   write one band of the filtered buffer (the forward outputs of a
 *       segment, before the backward pass). */
int nbls_filter_segment(nbls_handle* h, int32_t reverse, const double* state_in, double* state_out);
int nbls_set_filtered(nbls_handle* h, int32_t band, const double* data);

/* Device pointers of the result grids (for an RCCL gather straight from HBM):
 * ptrs[0..3] = vel, baz, mdccm, sigma_tau (double[nbands][vector_len]); ptrs[4] = nwin (int32).
 * The four grids are the head of the result block (see nbls_result_layout): always contiguous,
 * ptrs[i+1] - ptrs[i] == *bytes_per_grid. */
int nbls_device_results(nbls_handle* h, void** ptrs, int64_t* bytes_per_grid);

/* The result block: ONE device allocation holding, back to back,
 *     double vel[B][VL], baz[B][VL], mdccm[B][VL], sigma_tau[B][VL], uint8 mask[B][VL][MB]
 * MB = ceil(npairs / 8); bit (k & 7) of mask byte (k >> 3) is the LTS weight of pair k (1 = kept; all
 * 1 for OLS; rows beyond nwin[b] are zero).  This is what narrow_band_least_squares() needs back from
 * the GPU (rows written at narrow_band_least_squares.py:104-113 + the weights behind `stdict`, :114-124).
 *   nbls_result_layout: out4 = {cells = B*VL, MB, total bytes, byte offset of the mask}
 *   nbls_fetch_packed : one D2H copy of the whole block into out[nbytes] (nbytes = total bytes) */
int nbls_result_layout(nbls_handle* h, int64_t* out4);
int nbls_fetch_packed(nbls_handle* h, void* out, int64_t nbytes);

/* ---- streamed results: the rows of a pass reach the host batch by batch, while the pass is still running --------
 * Replaces "wait for the whole pass, then build the result rows and the dropped-element dictionary"
 * (narrow_band_least_squares.py:104-124 runs once per band, as each band's ltsva() returns; here a pass covers all
 * bands, and its units are processed in batches of consecutive (band, window) units):
 *   nbls_stream_results(h, 1)     the NEXT nbls_execute* run every unit batch as a complete chain
 *                                 (correlation -> solve -> weight mask) and queue, behind it, a copy of that batch's
 *                                 rows of the result block into a PINNED host mirror of the block owned by the
 *                                 library (same layout as nbls_result_layout / nbls_fetch_packed)
 *   nbls_result_batches(h, &n)    after nbls_execute*: how many batches the pass was cut into (>= 1)
 *   nbls_wait_result_batch(h, k, out4, &block)
 *                                 wait until batch k has landed; out4 = {u0, u1, c0, c1}: the batch holds the units
 *                                 [u0, u1) of the plan (band-major order: all windows of band 0, then band 1, ...) and
 *                                 its rows are the cells [c0, c1) of each grid / of the mask (cell = band * vector_len
 *                                 + window); *block = the mirror.  Batches finish in index order.  Cells outside
 *                                 the batches waited for so far are undefined; the mirror is valid until the handle's
 *                                 next nbls_execute*.  The host may work on batch k (build its dictionary entries)
 *                                 while the GPU runs batch k+1.
 * Results are identical to the unstreamed pass; nbls_fetch* still work afterwards. */
int nbls_stream_results(nbls_handle* h, int32_t on);
int nbls_result_batches(nbls_handle* h, int32_t* nbatches);
int nbls_wait_result_batch(nbls_handle* h, int32_t k, int64_t* out4, const void** host_block);

/* ---- several estimators on one pass's lags ---------------------------------------------------------------------
 * Replaces "one whole call per ALPHA and per sub-array" (narrow_band_least_squares.py:110-124 returns sig_tau_array
 * only for ALPHA == 1.0 and the dictionary only for ALPHA < 1.0; re-processing an array without the element LTS named
 * is a third call): filter, screening and verification depend on neither ALPHA nor on which other elements are
 * present, so one pass correlates the full array once and then solves every unit once per estimator.
 * Estimator 0 is what nbls_set_geometry / nbls_plan / nbls_set_uncertainty describe.  nbls_set_estimators names up to
 * 8 FURTHER ones, before nbls_plan; each is an array of `nkept` of the trace's elements (kept[]: 0-based, ascending, no
 * repeats; all of them = the full array) with the tables of THAT array exactly as a pass over it alone would get them:
 *   lts       FAST-LTS parameters (as for nbls_plan; starts index the sub-array's pairs), NULL for OLS
 *   xij       [P'][2], pair_idx [P'][2] (element numbers 0..nkept-1, lexicographic), xpinv [2][P'], P' = nkept (nkept-1)/2
 *   eig6      as nbls_set_uncertainty, NULL: no confidence intervals for this estimator
 * The arrays are copied.  Everything is checked before the handle changes: NBLS_ERR_GEOMETRY for fewer than 3 kept
 * elements (4 under LTS) or a collinear sub-array, NBLS_ERR_ARG for a bad index or table, NBLS_ERR_UNSUPPORTED for more
 * than 8 estimators and together with several segments, window ranges or an RCCL communicator (a plan refuses those
 * combinations too, whichever was set first).  n == 0 resets: the next plan is the plain pass again, launch for launch.
 * A sub-array's solve reads compact copies [B][VL][P'] of its pairs' lags and maxima, gathered per unit batch behind the
 * verifier; the solve kernels themselves are the ones of a plain pass.
 * The results of estimator e (0 = the existing calls) come from the nbls_est_* forms of the result calls: the layout and
 * block hold ceil(P'/8) mask bytes per cell, nbls_est_fetch gives lag / cmax / weights as [B][VL][P'].  A streamed pass
 * delivers batch k of EVERY estimator before batch k+1 of any; each estimator has a pinned mirror of its own. */
typedef struct {
    const nbls_lts_params* lts;
    int32_t nkept;
    const int32_t* kept;
    const double* xij;
    const int32_t* pair_idx;
    const double* xpinv;
    const double* eig6;
} nbls_estimator_desc;
int nbls_set_estimators(nbls_handle* h, int32_t n, const nbls_estimator_desc* desc);
int nbls_est_result_layout(nbls_handle* h, int32_t e, int64_t* out4);
int nbls_est_fetch_packed(nbls_handle* h, int32_t e, void* out, int64_t nbytes);
int nbls_est_fetch(nbls_handle* h, int32_t e, double* vel, double* baz, double* mdccm, double* sigma_tau, int32_t* nwin,
                   int32_t* lag, double* cmax, uint8_t* weights, double* z);
int nbls_est_fetch_uncertainty(nbls_handle* h, int32_t e, double* vel_uncert, double* baz_uncert);
int nbls_est_fetch_beam(nbls_handle* h, int32_t e, double* beam_power, double* fstat);
int nbls_est_fetch_closure(nbls_handle* h, int32_t e, double* consistency, double* closure_max, double* element_consistency);
int nbls_est_wait_result_batch(nbls_handle* h, int32_t e, int32_t k, int64_t* out4, const void** host_block);

/* ---- multi-GPU: ONE grouped RCCL operation collects every GPU's result block ----------------------
 * Replaces the joblib fan-out / collection of narrow_band_least_squares_parallel()
 * (narrow_band_least_squares.py:285 and :291-320).  Bands (or window slices) are sharded by the host;
 * every GPU runs nbls_plan/nbls_execute for its share; nbls_comm_gather moves the blocks over xGMI.
 *
 *   nbls_comm_init_all(hs, n)       one process, n handles on n different devices (ncclCommInitAll);
 *                                   handle i becomes rank i of n
 *   nbls_comm_unique_id(id, 128)    rank 0 of a multi-process job creates the communicator id ...
 *   nbls_comm_init_rank(h, id, world, rank)   ... and every process (one GPU each) joins with it; the
 *                                   128 id bytes travel by any side channel (the Python host: a TCP socket)
 *   nbls_reserve_results(h, bytes)  make the NEXT plans allocate the result block with at least
 *                                   `bytes` (= the common block size of the gather: ranks hold
 *                                   different numbers of bands, the gather needs equal blocks)
 *   nbls_comm_gather(hs, n, root, block_bytes, status, host_out, host_bytes)
 *       hs[0..n): the handles this process drives (n = 1 with one process per GPU).  Every rank sends
 *       block_bytes (a multiple of 8, >= its result block + 8): its result block, padding, and in the
 *       last 8 bytes `status` (int64; 0 = this rank's pass succeeded — lets a failed rank still take
 *       part so that nobody hangs; pass the rank's error code otherwise).  root >= 0: gather to that
 *       rank (grouped ncclSend/ncclRecv); root < 0: ncclAllGather.  The process that drives the root
 *       (all-gather: every process) receives host_out[world][block_bytes]; other processes may pass NULL.
 *       The operation is ordered on the handles' streams after their nbls_execute and returns after the
 *       copy to the host has finished.
 *   nbls_comm_destroy(h)            release the communicator (also done by nbls_destroy)
 * RCCL is resolved with dlopen at the first of these calls (librccl.so.1, librccl.so, /opt/rocm/lib/...).
 *   nbls_comm_set_library(path, allow_shared_device)
 *       for rehearsals on a one-GPU box: resolve the ten entry points from `path` instead (the tests' loopback
 *       stand-in, tests/c_caller/loopback_rccl.cpp); allow_shared_device = 1 lets nbls_comm_init_all take several
 *       handles of one device.  Must come before the first comm call (NBLS_ERR_STATE once RCCL has been resolved
 *       from elsewhere); path NULL = RCCL.  The library reads no environment variable.              */
int nbls_comm_set_library(const char* path, int32_t allow_shared_device);
int nbls_comm_init_all(nbls_handle* const* hs, int32_t n);
int nbls_comm_unique_id(void* id, int32_t nbytes);
int nbls_comm_init_rank(nbls_handle* h, const void* id, int32_t world, int32_t rank);
int nbls_reserve_results(nbls_handle* h, int64_t bytes);
int nbls_comm_gather(nbls_handle* const* hs, int32_t n, int32_t root, int64_t block_bytes, int64_t status,
                     void* host_out, int64_t host_bytes);
/* A rank whose share of the bands does not fit the HBM budget of one pass runs it in several passes
 * (nbls_plan / nbls_execute / nbls_fetch_packed per round), assembles its block on the host and puts it back where
 * nbls_comm_gather sends from.  block[nbytes]: the layout of nbls_result_layout for ALL of the rank's bands.
 * The handle needs a new nbls_plan before its next pass. */
int nbls_load_result_block(nbls_handle* h, const void* block, int64_t nbytes);
int nbls_comm_destroy(nbls_handle* h);

/* Per-handle switches, read by the next nbls_plan / nbls_execute.  Every key of the shipped library selects
 * between implementations that give IDENTICAL results (A/B timing; tests that check kernels against each other):
 *   "lts_impl" 0 auto | 1 lane-per-start generic FAST-LTS kernel | 3 generic only where no register kernel exists;
 *   "lts_generic_h", "lts_coop_threads", "lts_sample_its", "screen_tb4", "screen_tb8", "screen_nsl1", "screen_static",
 *   "screen_pretest", "screen_batch_mb", "solve_min_units" (units a per-batch solve / streamed result batch covers at least),
 *   "result_tail_units" (streamed pass: units of the last result batch, cut off the last solve; 0 = default 2048, < 0 = not cut),
 *   "overlap" (the solve of a unit batch on a second stream beside the next batch's correlation: 1 on, -1 off, 0 auto = on
 *   for streamed passes of several small batches), "filter_nofuse", "filter_row_step" (channels per filter launch: what a
 *   pass queued on an announced upload does as the rows land, forced),
 *   "filter_nomfma";
 *   "stream_priority" (applied at once; the handle must be idle): 0 normal, > 0 lower, < 0 higher, clamped to the
 *   device's range — for several handles of one GPU whose passes run side by side.
 * A developer build (make dev, -DNBLS_DEVELOPER; nbls_developer_build() == 1) adds "ablate" (skips kernel parts,
 * results WRONG), "screen_stamps", "lts_stamps", "screen_pad_kb", "lts_pad_kb", "plan_timing"; in the shipped
 * library those keys return NBLS_ERR_UNSUPPORTED and the corresponding code is not in the kernels.  The library
 * reads no environment variable. */
int nbls_set_option(nbls_handle* h, const char* key, int64_t value);
int nbls_developer_build(void);

/* The correlator route of one window group: which kernels the correlation stage launches for windows of W samples of an
 * array of `nelem` elements, with what tiling and how much LDS.  A pure host function (no handle, no device): nbls_plan
 * and the launchers take every window-length decision from it, tests scan it.  `npairs` pairs per unit, `vrows` result
 * rows the launch covers (several recordings: nbls_set_segments), `npts_pad` the padded trace length (its parity
 * matters), `xcorr_impl` as in nbls_plan, `flags` the NBLS_ROUTE_OPT_* bits of the handle options that change the
 * route.  Returns NBLS_ERR_ARG for arguments out of range, else 0 — also when a forced xcorr_impl does not apply
 * (correlator == NBLS_ROUTE_REJECTED). */
enum {
    NBLS_ROUTE_REJECTED = 0,      /* the forced xcorr_impl (2: f64 MFMA, 3: int8 screening) does not take this window  */
    NBLS_ROUTE_SCREEN = 1,        /* quantiser + int8 screening kernel + FP64 verifier                                 */
    NBLS_ROUTE_MFMA = 2,          /* xcorr_mfma_kernel                                                                 */
    NBLS_ROUTE_VALU_LDS = 3,      /* xcorr_simple_kernel, both windows in LDS                                          */
    NBLS_ROUTE_VALU_GLOBAL = 4    /* xcorr_simple_kernel, windows read from global memory                              */
};
enum { NBLS_ROUTE_QUANTIZE = 0, NBLS_ROUTE_SCREEN_STAGE = 1, NBLS_ROUTE_VERIFY = 2, NBLS_ROUTE_GENERAL = 3 };   /* lds_* index */
enum { NBLS_ROUTE_OPT_NC4 = 1, NBLS_ROUTE_OPT_NSL1 = 2, NBLS_ROUTE_OPT_TB8 = 4, NBLS_ROUTE_OPT_TB4 = 8 };   /* options screen_nc4 ... */
typedef struct {
    int32_t correlator;       /* NBLS_ROUTE_*                                                                       */
    int32_t impl;             /* what nbls_get_timings reports as xcorr_impl: 3 screening, 2 f64 MFMA, 1 VALU, 0 none */
    int32_t ncopy, G, S, nsl; /* screening: byte-shifted copies (8 / 4), partners per workgroup, lag blocks per tile,
                                 sliding channels per workgroup; f64 MFMA: S lag blocks per tile                      */
    int32_t PFB, CSB, CSA, WP;/* screening: lag-block prefix, partner image / copy stride (bytes), padded window;
                                 f64 MFMA: PFB = zero prefix, CSB = channel stride (doubles)                          */
    int32_t screen_inst;      /* 0 none, 1 screen_kernel<4,8>, 2 <4,4>, 3 <8,8>                                    */
    int32_t tab_lds;          /* the screening kernel's energy tables in LDS                                        */
    int32_t quant_inst;       /* 0 none, 2/3/4/6/8 quantize_reg_kernel<G>, 1 quantize_kernel                       */
    int32_t quant_waves;      /* waves per quantiser workgroup                                                      */
    int32_t verifier;         /* 0 none, 1 verify_dma_kernel, 2 verify_lds_kernel, 3 verify_kernel                  */
    int32_t verify_threads;   /* workgroup size of the verifier                                                     */
    int64_t lds_dyn[4];       /* dynamic LDS bytes per workgroup of each kernel launched (NBLS_ROUTE_QUANTIZE ...)  */
    int64_t lds_static[4];    /* static LDS bytes of the same kernels                                               */
} nbls_route;
int nbls_route_xcorr(int32_t nelem, int32_t W, int32_t npairs, int32_t vrows, int64_t npts_pad, int32_t xcorr_impl,
                     int32_t flags, nbls_route* out);
/* The routes of every window length W0..W1 (out[W - W0]): one call for a scan. */
int nbls_route_table(int32_t nelem, int32_t W0, int32_t W1, int32_t npairs, int32_t vrows, int64_t npts_pad,
                     int32_t xcorr_impl, int32_t flags, nbls_route* out);

/* Enable (1) / disable (0) HIP-event timing of the stages; read the last run's timings. */
int nbls_set_profiling(nbls_handle* h, int32_t on);
int nbls_get_timings(nbls_handle* h, nbls_timings* out);

/* plan + execute + sync + fetch in one call. */
int nbls_run(nbls_handle* h, int32_t nbands, const double* sos, int32_t nsections,
             int32_t zero_phase, const double* taper_left, const double* taper_right,
             int32_t taper_len, const int32_t* winlen, const int32_t* wininc,
             int32_t vector_len, const nbls_lts_params* lts, int32_t xcorr_impl,
             double* vel, double* baz, double* mdccm, double* sigma_tau, int32_t* nwin,
             int32_t* lag, double* cmax, uint8_t* weights, double* z);

/* Debug / self-test: run one f64 MFMA 16x16x4 on caller data (a[64], b[64] one value per
 * lane) and return the 256 accumulator values as out[lane*4 + reg]. */
int nbls_probe_mfma_f64(nbls_handle* h, const double* a, const double* b, double* out);
/* Same for one int8 MFMA 16x16x64: a[64][4], b[64][4] packed dwords (16 int8 per lane),
 * out[lane*4 + reg] int32. */
int nbls_probe_mfma_i8(nbls_handle* h, const int32_t* a, const int32_t* b, int32_t* out);

/* Developer statistic of the int8 screening correlator (last unit batch): out8 (EIGHT int64) = {ordered pairs,
 * pairs whose candidate buffer overflowed, total candidates, max candidates per ordered pair, runs of consecutive
 * listed lags, listed lags that sit in a run of two or more, 0, 0}. */
int nbls_debug_screen_stats(nbls_handle* h, int64_t* out8);
/* Developer / tests: the candidate records the screening kernel left for the last unit batch, [units][N][N][32] int32,
 * record (unit, sliding channel i, partner j) = {count, flags (1 interval, 2 list overflow), kk_lo, kk_hi, screening
 * maximum (f32 bits), theta (f32 bits), up to 26 np.correlate indices kk}; the diagonal is not written.  *units = units
 * of that batch; out NULL: only that.  capacity: int32 elements of out. */
int nbls_debug_screen_records(nbls_handle* h, int32_t* out, int64_t capacity, int64_t* units);
/* Developer: mean s_memtime cycle counts of the phases of the wave-per-unit FAST-LTS kernel
(developer build, options "screen_stamps" / "lts_stamps"): out8 = {setup+medians, elemental starts,
 * C-steps, candidate peel, refinement, finish, 0, total}. */
int nbls_debug_lts_stamps(nbls_handle* h, double* out8);
/* Developer: C-step phases of the large-array FAST-LTS kernel (9..32 elements): out8 = mean cycles of thread 0 in
 * {groups (selection + sums), subset merging, compaction}, the live entries summed over the iterations, and wave 0's
 * {selection passes, selection cycles, sums cycles, groups taken}. */
int nbls_debug_lts_coop_breakdown(nbls_handle* h, double* out8);
int nbls_debug_screen_stamps(nbls_handle* h, double* out10);

#ifdef __cplusplus
}
#endif
#endif /* NBLS_H */
