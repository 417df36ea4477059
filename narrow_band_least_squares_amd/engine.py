"""Host driver of the HIP path: turns a stream + band list into one batched device pass
(filter -> xcorr/lag pick -> MdCCM + OLS|LTS for every band x window) and unpacks the result
grids.  Used by ``ltsva``, ``filter_data``, ``narrow_band_least_squares*`` and ``bench.py``.
"""
import functools
import itertools
import operator
import os
import contextlib
import threading
import types

import numpy as np

from . import _hip, planner
from ._hip import Handle
from .call_requests import (CLEAN_FIELDS, EXTRA_FIELDS, MUSIC_FIELDS, PEAK_FIELDS, RESULT_GROUPS, Requests,   # noqa: F401
                            _check_beam_trace, _check_element_delays)       # (the last five: for the public calls' modules)
from .stream import start_datenum

try:                                   # C++ helpers for the stdict keys / dictionary (csrc/host_ext.cpp)
    from . import _nbls_host as _hostext
except ImportError:                    # not built: the pure-Python equivalents below are used
    _hostext = None

_handles = {}

# Scheduling switches of the band-group path of rounds 2-3 and of the host helpers: module attributes, set by tests and
# tools (they were environment variables until round 4: NBLS_UPLOAD_OVERLAP, NBLS_GROUP_ORDER, NBLS_STREAM_PRIORITY,
# NBLS_PIPELINE_SPLIT, NBLS_KEY_THREADS).  Results never depend on them.
UPLOAD_OVERLAP = True      # the trace goes up on a helper thread beside the filter design and the plan
ROW_PIPELINE = True        # ... and the pass is queued while it still does: the library filters the channels as they land
ROW_PIPELINE_MIN_BYTES = 256 << 20   # ... for traces whose upload is worth hiding (1.1 GB at cfg-4: the 12-band share's call 236 ->
                           # 221 ms; at cfg-3's 55 MB = 1.2 ms the extra filter launches cost 0.4 ms more than they hide)
GROUP_ORDER = True         # band groups: the groups' correlation stages are chained on the GPU (nbls_execute_after)
STREAM_PRIORITY = True     # band groups: earlier groups on higher-priority streams
PIPELINE_SPLIT = None      # band groups: explicit shares, e.g. (0.15, 0.5, 0.35)
KEY_THREADS = None         # threads that format the stdict key text (default: min(4, cores - 1))


def default_device():
    """NBLS_DEVICE, else LOCAL_RANK (one process per GPU under torch.distributed.run), else 0."""
    for key in ('NBLS_DEVICE', 'LOCAL_RANK'):
        v = os.environ.get(key)
        if v is not None and v != '':
            return int(v)
    return 0


def get_handle(device=None, slot=0):
    """Per-(process, device, slot) handle, created lazily so that a fork before first use is safe.  Slots > 0
    are further handles (own stream, own buffers) on the same GPU: the band groups of a pipelined call."""
    dev = default_device() if device is None else int(device)
    key = (os.getpid(), dev, int(slot))
    h = _handles.get(key)
    if h is None:
        h = Handle(dev)
        # the groups' passes run side by side; the earlier group's workgroups are dispatched first so that its rows
        # land while the later groups still keep the GPU busy (the host builds that group's dictionary meanwhile)
        if STREAM_PRIORITY:
            h.set_option('stream_priority', min(int(slot), 2) - 1)
        _handles[key] = h
    return h


def pipeline_groups(nwin, npairs=28):
    """Into how many band groups a call is cut (``NBLS_PIPELINE_GROUPS`` overrides).  Each group is its own
    asynchronous pass on its own handle of the same GPU: while the GPU works on group k, the host designs the
    filters of group k+1, and later turns the finished groups' weights into the dropped-element dictionary
    while the remaining groups are still being computed.  Small calls are one group.  "Small" is measured in units
    weighted by the pair count (a unit of a 32-element array costs ~20x the GPU time of an 8-element one, and its
    dictionary entry — up to 62 mask bytes, a value array of its own — several times the host time: at 32 elements x
    128 bands the dictionary of a single-group call was a 15-25 ms tail behind the GPU)."""
    env = os.environ.get('NBLS_PIPELINE_GROUPS')
    nb = len(nwin)
    if env:
        return max(1, min(nb, int(env)))
    weight = max(1.0, float(npairs) / 28.0)
    return max(1, min(4, nb, int(np.sum(nwin) * weight) // 16000))


_graveyard = []


def release_later(*objs):
    """Keep helper objects of a finished call alive until ``release_deferred`` (their teardown — tens of thousands of
    small records — is host time that can hide behind the next call's GPU pass)."""
    _graveyard.append(objs)


def release_deferred():
    del _graveyard[:]


STREAM_MIN_UNITS = 16000    # (band, window) units x (pairs / 28) from which a call streams its rows (``stream_pays``)


def streamed_default():
    """Whether ``NBLS_STREAM_RESULTS`` / ``NBLS_PIPELINE_GROUPS`` allow the streamed form at all (see ``stream_pays``)."""
    if os.environ.get('NBLS_STREAM_RESULTS', '1') == '0':
        return False
    env = os.environ.get('NBLS_PIPELINE_GROUPS')
    return not (env and int(env) > 1)


def stream_pays(alpha, nwin, npairs=28):
    """Whether a whole call runs as ONE pass whose unit batches stream their rows to the host (``nbls_stream_results``)
    while the GPU works on the next batch.  What the host does with a batch's rows is the dropped-element dictionary, so:
    under LTS, from ``STREAM_MIN_UNITS`` units on (weighted by the pair count as in ``pipeline_groups``).  Below that, and
    under OLS (no dictionary), the pass is fetched in one piece: the per-batch solves, copies and events of the streamed
    form are pure overhead there (cfg-1b, 443 OLS units in 8 window groups: 2.2 ms per call streamed, 1.07 ms in one piece;
    cfg-2, 5 700 LTS units: no difference; cfg-3: 17.1 against 18.5 ms).  ``NBLS_STREAM_RESULTS=1`` streams always, ``=0``
    never; ``NBLS_PIPELINE_GROUPS`` > 1 selects the band groups of rounds 2-3."""
    if not streamed_default():
        return False
    if os.environ.get('NBLS_STREAM_RESULTS') == '1':
        return True
    weight = max(1.0, float(npairs) / 28.0)
    return float(alpha) < 1.0 and int(np.sum(nwin) * weight) >= STREAM_MIN_UNITS


def stream_to_array(st):
    """-> (data (N, npts) float64 C-contiguous, fs, start date number)."""
    nchans = len(st)
    if nchans == 0:
        raise ValueError('empty stream')
    npts = len(st[0].data)
    fs = float(st[0].stats.sampling_rate)
    data = np.empty((nchans, npts), dtype=np.float64)
    for i, tr in enumerate(st):
        if len(tr.data) != npts:
            raise ValueError('All traces must have the same number of samples.')
        data[i] = tr.data
    return data, fs, start_datenum(getattr(st[0].stats, 'starttime', 0.0))


def stream_rows(st):
    """-> (list of per-channel 1-D float64 arrays — the traces' own buffers when they already are
    C-contiguous float64 —, fs, start date number).  Nothing is packed: ``Handle.set_trace_rows``
    uploads every row from where it lies."""
    nchans = len(st)
    if nchans == 0:
        raise ValueError('empty stream')
    npts = len(st[0].data)
    fs = float(st[0].stats.sampling_rate)
    rows = []
    for tr in st:
        d = np.asarray(tr.data)
        if len(d) != npts:
            raise ValueError('All traces must have the same number of samples.')
        if d.dtype != np.float64 or not d.flags.c_contiguous:
            d = np.ascontiguousarray(d, dtype=np.float64)
        rows.append(d)
    return rows, fs, start_datenum(getattr(st[0].stats, 'starttime', 0.0))


class _UploadWorker:
    """One helper thread per process, kept between calls, that runs the trace uploads of ``process`` (the copy happens
    inside the library with the GIL released).  ``submit(fn)`` -> an object with ``join()``."""

    class _Job:
        def __init__(self, fn):
            self.fn, self.done = fn, threading.Event()

        def join(self):
            self.done.wait()

    def __init__(self):
        import queue
        self.pid = os.getpid()
        self.q = queue.SimpleQueue()
        self.thread = threading.Thread(target=self._run, name='nbls-upload', daemon=True)
        self.thread.start()

    def _run(self):
        while True:
            job = self.q.get()
            try:
                job.fn()                          # (the uploads catch their own exceptions and hand them to the caller)
            finally:
                job.done.set()

    def submit(self, fn):
        job = self._Job(fn)
        self.q.put(job)
        return job


_upload_worker_obj = None
_upload_worker_lock = threading.Lock()


def _upload_worker():
    global _upload_worker_obj
    w = _upload_worker_obj
    if w is None or w.pid != os.getpid() or not w.thread.is_alive():      # (a forked child starts its own)
        with _upload_worker_lock:
            w = _upload_worker_obj
            if w is None or w.pid != os.getpid() or not w.thread.is_alive():
                w = _upload_worker_obj = _UploadWorker()
    return w


def row_pipeline_for(nchans, npts):
    """Queue the pass while the trace is still going up (``Handle.expect_upload``)?  Worth it for long uploads only."""
    return bool(ROW_PIPELINE) and 8 * int(nchans) * int(npts) >= ROW_PIPELINE_MIN_BYTES


class TraceUpload:
    """The rows of a trace going up to handle ``h`` on a helper thread (a blocking copy from pageable memory inside the
    library, GIL released) while the caller designs filters and plans the pass: the handle knows the trace's shape
    (``set_trace_shape``), only ``nbls_execute`` needs the samples.  ``landed()`` joins the copy and re-raises ITS exception
    on the caller's thread; a second call does nothing.  ``close()`` only joins: every way out of a call goes through
    it, so that no copy is left running behind the caller.  ``row_pipeline``: the handle has been told to expect the rows
    (``row_pipeline_for``), the pass may be queued before ``landed()``.  ``worker``: an ``_UploadWorker`` (``process``: one
    thread kept between calls, starting one costs 0.1 ms of the 1.3 ms the copy takes); None starts a thread of its own
    (the sharded call: one per GPU at the same time)."""

    def __init__(self, h, rows, fs, worker=None):
        self.h, self.rows, self.error = h, rows, None
        h.set_trace_shape(len(rows), len(rows[0]), fs)
        self.row_pipeline = row_pipeline_for(len(rows), len(rows[0])) and hasattr(h, 'expect_upload')
        if self.row_pipeline:
            h.expect_upload()
        if worker is not None:
            self.job = worker.submit(self._run)
        else:
            self.job = threading.Thread(target=self._run, name='nbls-upload')
            self.job.start()

    def _run(self):
        try:
            self.h.upload_rows(self.rows)
        except BaseException as e:                # handed to the calling thread by landed()
            self.error = e

    def close(self):
        job, self.job = self.job, None
        if job is not None:
            job.join()
        return job is not None

    def landed(self):
        if self.close() and self.error is not None:
            raise self.error


def _trace_key(data, fs):
    """Identity of a trace as the caller holds it: where its samples lie (address, length of every row) and the
    sampling rate.  None for anything that is not float64 C-contiguous (such rows are converted per call: no identity)."""
    rows = [data] if isinstance(data, np.ndarray) and data.ndim == 2 else list(data)
    key = [float(fs)]
    for r in rows:
        if not isinstance(r, np.ndarray) or r.dtype != np.float64 or not r.flags.c_contiguous:
            return None
        key.append((r.ctypes.data, r.shape))
    return tuple(key)


class resident_trace:
    """``with engine.resident_trace(st):`` — upload the stream's samples ONCE and keep them in HBM: every call made inside
    the block on the SAME buffers (``narrow_band_least_squares(..., st, ...)``, ``ltsva`` — the same Stream object, its
    traces' ``data`` arrays float64 and C-contiguous, which is what ``stream_rows`` passes through untouched) skips its
    upload (55 MB over PCIe = 1.4 ms of a 17 ms call at the benchmark's shape).  For a caller that runs several
    parameter sets over one trace.  The caller promises not to write to the samples inside the block; any other trace
    processed on the same GPU meanwhile ends the residency (the next call uploads again).  Accepts a Stream, a 2-D array
    or a list of rows (then ``fs`` is required)."""

    def __init__(self, st, fs=None, device=None):
        if fs is None:
            self.rows, self.fs, _ = stream_rows(st)
        else:
            self.rows, self.fs = st, float(fs)
        self.device = device
        self.handle = None

    def __enter__(self):
        key = _trace_key(self.rows, self.fs)
        if key is None:
            raise ValueError('resident_trace: the samples must be float64 and C-contiguous (they are converted per call otherwise)')
        h = get_handle(self.device, 0)
        upload_trace(h, self.rows, self.fs)
        h.resident_key = key
        self.handle = h
        return self

    def __exit__(self, *exc):
        if self.handle is not None and self.handle.resident_key is not None:
            self.handle.resident_key = None
        return False


def _shape_of(data):
    """(nchans, npts) of a 2-D array or of a list of equally long rows."""
    if isinstance(data, np.ndarray):
        if data.ndim != 2:
            raise ValueError('trace must be (nchans, npts)')
        return data.shape
    return len(data), len(data[0])


def check_elements(nchans, alpha):
    if nchans < 3:
        raise RuntimeError('At least 3 array elements are needed for the least squares estimate.')
    if alpha < 1.0 and nchans < 4:
        raise RuntimeError('At least 4 array elements are needed for least trimmed squares.')
    if not (0.5 <= alpha <= 1.0):
        raise ValueError('ALPHA must be in [0.5, 1.0].')


def window_times(t0_datenum, fs, W, inc, nwin):
    """t[w] = tvec[w*inc + W//2], tvec = start + (arange(npts)/fs)/86400 (matplotlib dates)."""
    idx = np.arange(nwin) * inc + int(W / 2)
    return t0_datenum + (idx / fs) / 86400.0


def time_grid(t0_datenum, fs, W, inc, nwin, vector_len):
    """Window-centre times of every band -> (nbands, vector_len), zero behind a band's last window."""
    tt = np.zeros((len(nwin), vector_len))
    rows = {}                                    # (one row of window times per distinct window plan)
    for b in range(len(nwin)):
        key = (int(W[b]), int(inc[b]), int(nwin[b]))
        if key not in rows:
            rows[key] = window_times(t0_datenum, fs, *key)
        tt[b, :key[2]] = rows[key]
    return tt


def plan_windows(npts, fs, winlens, winover, vector_len=None):
    """Per-band window plan -> (W samples int32, inc samples int32, nwin int64, vector_len): the result row length
    defaults to the longest band's window count and must hold it."""
    nb = len(winlens)
    W, inc, nwin = [np.empty(nb, dtype=t) for t in (np.int32, np.int32, np.int64)]
    plans = {}                                   # (bands usually share a few window lengths: one plan per length)
    for b in range(nb):
        wl = float(winlens[b])
        if wl not in plans:
            plans[wl] = planner.window_plan(npts, fs, winlens[b], winover)
        W[b], inc[b], nwin[b] = plans[wl]
    if vector_len is None:
        vector_len = max(1, int(nwin.max()))
    if nwin.max() > vector_len:
        raise ValueError('could not broadcast %d windows into result rows of length %d '
                         '(vector_len too small for this band)' % (int(nwin.max()), vector_len))
    return W, inc, nwin, int(vector_len)


class BandBatch:
    """Results of one device pass over ``nbands`` bands (arrays are (nbands, vector_len)).
    ``mask`` (nbands, vector_len, ceil(P/8)) is the packed LTS weight mask as the GPU returns it;
    ``weights`` (nbands, vector_len, P) uint8 is unpacked from it on first use."""

    def __init__(self, **kw):
        self._weights = None
        self.__dict__.update(kw)

    @property
    def weights(self):
        if self._weights is None and getattr(self, 'mask', None) is not None and self.lts:
            P = len(self.pair_idx)
            self._weights = np.unpackbits(self.mask, axis=-1, bitorder='little')[..., :P]
        return self._weights


GRID_NAMES = ('vel', 'baz', 'mdccm', 'sigma_tau')      # the four planes of ``BandBatch.grids``, in result-block order


def new_result(nchans, alpha, fs, W, inc, nwin, vector_len, want_lag=False, want_cmax=False, want_z=False,
               want_uncert=False, want_beam=False, want_subsample=False, grid_points=0, want_grid_map=False,
               want_consistency=False, capon_points=0, want_capon_maps=False, want_capon_csdm=False, capon_peaks=0,
               want_kept=False, beam_trace_npts=0, want_element_delays=False, grid_refine_levels=0, clean_iterations=0,
               want_clean_csdm=False, want_music=False, want_music_maps=False, want_music_vectors=False, want_music_peaks=False):
    """The zero-filled ``BandBatch`` of a call (calloc: pages a pass never writes stay untouched).  ``grids`` (4, nbands,
    vector_len) is what the drivers fill, ``vel`` ... ``sigma_tau`` are its planes; ``t``, ``sos``, ``pair_idx``, ``xij`` and
    ``handle`` are the driver's to set.  The keywords are what ``Requests.result_keywords`` makes of a call's requests; the
    fields they bring are the rows of ``call_requests.RESULT_GROUPS`` and ``EXTRA_FIELDS`` that apply, each (nbands,
    vector_len) + its trailing shape with N = ``nchans``, P pairs, G = ``grid_points``, R = ``grid_refine_levels``, C =
    ``capon_points``, K = ``capon_peaks``, I = ``clean_iterations`` and T = ``beam_trace_npts`` (``beam_trace``: (nbands, T)); None otherwise —
    the fields of a ``sparse`` group are attributes of the result only where the group applies
    (``Requests.check`` says what each is)."""
    want = types.SimpleNamespace(**locals())
    nb, P = len(nwin), nchans * (nchans - 1) // 2
    size = dict(N=nchans, P=P, G=grid_points, R=grid_refine_levels, C=capon_points, K=capon_peaks, I=clean_iterations,
                T=beam_trace_npts)
    fields = {}

    def allocate(on, rows, group, sparse=False):
        for name, trailing, dtype in group:
            if on or not sparse:
                fields[name] = np.zeros(rows + tuple(int(size.get(n, n)) for n in trailing), dtype=dtype) if on else None

    for name, trailing, dtype in EXTRA_FIELDS:
        allocate(getattr(want, 'want_' + name), (nb, vector_len), [(name, trailing, dtype)])
    for g in RESULT_GROUPS:
        for _, group in g.calls:
            allocate(g.applies(want), (nb,) if g.per_row else (nb, vector_len), group, g.sparse)
    grids = np.zeros((4, nb, vector_len))
    return BandBatch(grids=grids, nwin=nwin.astype(int), t=None, mask=np.zeros((nb, vector_len, (P + 7) // 8), dtype=np.uint8),
                     sos=[], W=W, inc=inc, pair_idx=None, xij=None, nchans=nchans, alpha=alpha, handle=None, lts=alpha < 1.0,
                     fs=fs, **dict(zip(GRID_NAMES, grids)), **fields)


def drain(h, streamed, grids, mask, b0, b1, batch_done=None):
    """Bring the result of the pass that handle ``h`` has just run into rows [b0, b1) of ``grids`` (4, B, VL; None: the
    mask only) and ``mask`` (B, VL, MB), both C-contiguous.  Not streamed: waits for the pass, ONE D2H copy (grids + weight
    mask).  Streamed: the rows arrive batch by batch in a pinned mirror of the result block; each batch is waited for once,
    in order, its cells [c0, c1) are copied out (the mirror is undefined outside them) and ``batch_done(u0, u1)`` is told
    the batch's units — relative to the pass — while the GPU is busy with the next batch."""
    if not streamed:
        out = h.fetch_packed()
        if grids is not None:
            for g, name in enumerate(GRID_NAMES):
                grids[g, b0:b1] = out[name]
        mask[b0:b1] = out['mask']
        return
    gdst = None if grids is None else [grids[g, b0:b1].reshape(-1) for g in range(4)]
    mdst = mask[b0:b1].reshape(-1, mask.shape[-1])
    for k in range(h.result_batches()):
        u0, u1, c0, c1, gsrc, msrc = h.wait_result_batch(k)
        if c1 > c0:
            if gdst is not None:
                for g in range(4):
                    gdst[g][c0:c1] = gsrc[g, c0:c1]
            mdst[c0:c1] = msrc[c0:c1]
        if batch_done is not None:
            batch_done(u0, u1)
    if getattr(h, 'profiling', False):
        h.sync()                                   # (turns the pass's events into ``timings()``)


def _filtered_budget_bytes():
    return float(os.environ.get('NBLS_MAX_FILTERED_GB', '160')) * 2.0 ** 30


def max_bands_per_pass(nchans, npts, trace_rows=0):
    """Bands whose filtered traces fit the HBM budget of one pass (NBLS_MAX_FILTERED_GB, default 160 of
    the 288 GB): each band keeps an (N, npts) float64 copy resident for the correlation stage — and, in a pass that forms
    the beam trace (``nbls_set_beam_trace``), ``trace_rows`` more rows, one per recording.  0: not even
    one band fits -> ``process`` switches to the time-segmented path."""
    return int(_filtered_budget_bytes() // (8.0 * (nchans + trace_rows) * (npts + 64)))


def filter_band_segmented(h, rows, fs, sos_apply, zero_phase, seg_len):
    """Band-pass ONE band of a trace that is too long for the HBM budget: the trace goes through the GPU in
    consecutive time segments of ``seg_len`` samples (a multiple of the 512-sample scan chunk) and the IIR state
    is handed from segment to segment (``nbls_filter_segment``), forward in time and — zero-phase — backward in
    time over the forward outputs.  Equals the whole-trace filter (helpers.py:124-139) up to the rounding of the
    carried states.  -> (N, npts) filtered, UNTAPERED traces on the host."""
    nchans, npts = len(rows), len(rows[0])
    chunk = 512
    seg = max(chunk, int(seg_len) // chunk * chunk)
    bounds = [(a, min(a + seg, npts)) for a in range(0, npts, seg)]
    y = np.empty((nchans, npts))
    sos3 = np.ascontiguousarray(sos_apply, dtype=np.float64)[None, :, :]

    def plan_for(n):                # filter-only plan of an n-sample segment (one dummy window, no geometry needed)
        h.plan(sos3, zero_phase, None, None, [2], [max(1, n)], 1)

    state = None
    for (a, b) in bounds:
        h.set_trace_rows([r[a:b] for r in rows], fs)
        plan_for(b - a)
        state = h.filter_segment(False, state_in=state, want_state=(b < npts))
        y[:, a:b] = h.fetch_filtered(0)
    if zero_phase:
        state = None
        for (a, b) in reversed(bounds):
            seg_y = np.ascontiguousarray(y[:, a:b])
            h.set_trace(seg_y, fs)                          # (sets the segment length; the backward pass reads the filtered buffer)
            plan_for(b - a)
            h.set_filtered(0, seg_y)
            state = h.filter_segment(True, state_in=state, want_state=(a > 0))
            y[:, a:b] = h.fetch_filtered(0)
    return y


def process_segmented(data, fs, t0_datenum, rij, band_edges, winlens, winover, alpha, filter_type, filter_order,
                      filter_ripple, vector_len, device=None, xcorr_impl=0, want_lag=False, want_cmax=False, want_z=False,
                      host_overlap=None, group_done=None, want_beam=False, want_subsample=False, min_velocity=None,
                      slowness_grid=None, seed_halfwidths=None, want_consistency=False, element_max_shift=None,
                      want_beam_trace=None, beam_taps=0):
    """The hot path when not even ONE band's filtered trace fits the HBM budget: band by band,
    (1) the band is filtered in time segments with IIR state hand-off (``filter_band_segmented``) and tapered at
    global positions, (2) its windows go through the correlation + solve kernels in slices of consecutive windows
    (the ``ltsva`` entry of the device pass).  Same rows as the in-core pass up to the rounding of the carried filter
    states; HBM holds one segment / one window slice at a time.  The filtered band stays on the host and the windows reach
    the GPU slice by slice, so what reads the filtered band or the lag table of a whole pass in HBM is not available here:
    every opt-in keyword of this signature is refused when it is given, ``ValueError`` (``Requests.segmented_refusal``)."""
    Requests(beam=want_beam, subsample=want_subsample, lag_limits=min_velocity, beam_grid=slowness_grid,
             lag_seed=seed_halfwidths, closure=want_consistency, element_delays=element_max_shift, beam_trace=want_beam_trace,
             beam_taps=beam_taps).segmented_refusal(*_shape_of(data))        # (unchecked: only what is given matters)
    rows = [np.ascontiguousarray(r, dtype=np.float64) for r in data]
    nchans, npts = len(rows), len(rows[0])
    nb = len(band_edges)
    h = get_handle(device)
    budget = _filtered_budget_bytes()
    seg_len = max(512, int(budget // (16.0 * nchans)))               # raw + filtered copy of a segment
    W, inc, nwin, vector_len = plan_windows(npts, fs, winlens, winover, vector_len)
    designs = planner.design_bandpass_many(filter_type, band_edges, filter_order, filter_ripple, fs)
    res = new_result(nchans, alpha, fs, W, inc, nwin, vector_len, want_lag, want_cmax, want_z)
    res.xij, res.pair_idx, _ = planner.co_array(rij)
    res.t, res.sos, res.handle = time_grid(t0_datenum, fs, W, inc, nwin, vector_len), [d[2] for d in designs], h
    if host_overlap is not None:
        host_overlap(res)
    tl, tr = planner.taper_ramps(npts)
    for b in range(nb):
        sos_apply, zero_phase, _ = designs[b]
        y = filter_band_segmented(h, rows, fs, sos_apply, zero_phase, seg_len)
        if len(tl):
            y[:, :len(tl)] *= tl
            y[:, npts - len(tr):] *= tr
        # windows in slices of consecutive windows: slice [w0, w1) needs samples [w0*inc, (w1-1)*inc + W + 1)
        Wb, ib, nw = int(W[b]), int(inc[b]), int(nwin[b])
        per_slice = max(1, int((budget // (16.0 * nchans) - Wb - 1) // ib))
        for w0 in range(0, nw, per_slice):
            w1 = min(nw, w0 + per_slice)
            s0 = w0 * ib
            L = min(npts - s0, (w1 - w0 - 1) * ib + Wb + 1)
            part = process(np.ascontiguousarray(y[:, s0:s0 + L]), fs, 0.0, rij, [(None, None)], [winlens[b]], winover, alpha,
                           prefiltered=True, handle=h, xcorr_impl=xcorr_impl, want_lag=want_lag, want_cmax=want_cmax,
                           want_z=want_z, vector_len=w1 - w0)
            assert int(part.nwin[0]) == w1 - w0
            res.grids[:, b, w0:w1] = part.grids[:, 0]
            res.mask[b, w0:w1] = part.mask[0]
            for name, _, _ in EXTRA_FIELDS:
                if getattr(res, name) is not None:
                    getattr(res, name)[b, w0:w1] = getattr(part, name)[0]
        if group_done is not None:
            group_done(res, b, b + 1)
    return res


class Prep:
    """Host-side plan of a call: everything the GPU pass needs that is computed on the host — window
    plan, filter design, taper ramps, co-array, FAST-LTS constants — for ALL bands of the call.  A device
    then runs any subset of the bands (band sharding) or of the windows (window sharding) of it."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def prepare(nchans, npts, fs, rij, band_edges, winlens, winover, alpha, filter_type=None, filter_order=None,
            filter_ripple=None, vector_len=None, prefiltered=False, common=None, windows=None):
    """``common``: the Prep of another band group of the same call — its co-array, taper ramps and FAST-LTS plan
    do not depend on the bands and are reused instead of being recomputed per group.  ``windows``: these bands'
    ``plan_windows`` result, where the caller has planned the windows of the whole call already."""
    check_elements(nchans, alpha)
    nb = len(band_edges)
    if common is not None:
        xij, pair_idx, xpinv = common.xij, common.pair_idx, common.xpinv
    else:
        xij, pair_idx, xpinv = planner.co_array(rij)
    W, inc, nwin, vector_len = windows or plan_windows(npts, fs, winlens, winover, vector_len)
    sos_ret = []
    if prefiltered:
        if nb != 1:
            raise ValueError('a pre-filtered pass has exactly one band')
        sos, zero_phase, tl, tr = None, False, None, None
    else:
        applied = []
        zero_phase = None
        # all bands of the group designed in one vectorised pass (bit-identical to SciPy's per-band design)
        for sa, zp, sr in planner.design_bandpass_many(filter_type, band_edges, filter_order, filter_ripple, fs):
            applied.append(sa)
            sos_ret.append(sr)
            zero_phase = zp
        sos = planner.pad_sections(applied)
        tl, tr = (common.tl, common.tr) if common is not None else planner.taper_ramps(npts)
    if common is not None:
        lts = common.lts
    else:
        lts = planner.lts_plan(xij, alpha) if alpha < 1.0 else None
    return Prep(nchans=nchans, npts=npts, fs=fs, nbands=nb, xij=xij, pair_idx=pair_idx, xpinv=xpinv, W=W, inc=inc,
                nwin=nwin, vector_len=int(vector_len), sos=sos, zero_phase=zero_phase, tl=tl, tr=tr, lts=lts,
                sos_ret=sos_ret, alpha=alpha, npairs=xij.shape[0], mask_bytes=(xij.shape[0] + 7) // 8)


def upload_trace(h, data, fs):
    if isinstance(data, np.ndarray):
        h.set_trace(data, fs)
    else:
        h.set_trace_rows(data, fs)


def launch(h, data, prep, bands=None, upload=True, window_slice=None, xcorr_impl=0, reserve_bytes=0, trace_from=None,
           trace_ready=False, after=None, before_execute=None, stream=False, requests=None, uncert=False, estimators=None,
           beam=False, subsample=False, lag_limits=None, beam_grid=None, beam_grid_map=False, lag_seed=None, closure=False,
           capon=None, kept=None, capon_clean=None, capon_music=None, families=None, grid_refine=None, element_delays=None,
           element_delays_kept=False, beam_trace=None, beam_taps=0):
    """Upload (optional), plan and start the pass for the band subset ``bands`` (indices into the Prep;
    None = all) on handle ``h``.  Returns as soon as the kernels are queued.  ``trace_from``: another handle of
    the same GPU that already holds this trace (device-to-device copy instead of a second upload).
    ``trace_ready``: the caller has already uploaded the trace to ``h`` (``upload_trace``).  ``after``: the handle
    of the band group queued before this one (``Handle.execute``).  ``before_execute()``: called between plan and
    execute (the caller joins its upload thread there).  ``estimators``: the further estimators of the pass
    (``Handle.set_estimators``); a handle that still carries some from an earlier call is reset.  ``requests``: the opt-in
    requests of the plan, a ``Requests`` record — or, without one, its attributes as the keywords from ``uncert`` on.  Its
    per-band tables have one entry per band of the Prep: ``bands`` cuts them (``Requests.for_bands``).  They are on the
    handle for this plan only (``Requests.applied``), and so is the ``window_slice``."""
    req = requests if requests is not None else Requests(
        uncert=uncert, beam=beam, subsample=subsample, lag_limits=lag_limits, beam_grid=beam_grid, beam_grid_map=beam_grid_map,
        lag_seed=lag_seed, closure=closure, capon=capon, kept=kept, capon_clean=capon_clean, capon_music=capon_music,
        families=families, element_delays=element_delays, element_delays_kept=element_delays_kept, beam_trace=beam_trace,
        beam_taps=beam_taps, grid_refine=grid_refine)
    if upload:
        if trace_ready:
            pass
        elif trace_from is not None and trace_from is not h:
            h.set_trace_from(trace_from)
        else:
            upload_trace(h, data, prep.fs)
        h.set_geometry(prep.xij, prep.pair_idx, prep.xpinv)
    if estimators or getattr(h, 'est_npairs', None):       # (behind the trace: the library checks the indices against its elements)
        h.set_estimators(estimators or ())
    idx = np.arange(prep.nbands) if bands is None else np.asarray(bands, dtype=np.int64)
    sos = None if prep.sos is None else prep.sos[idx]
    with contextlib.ExitStack() as undo:          # (the handle is shared with calls that plan for themselves)
        if window_slice is not None:
            k, n = window_slice
            nw = prep.nwin[idx]
            first = (nw * k) // n
            h.set_window_ranges(first, (nw * (k + 1)) // n - first)
            undo.callback(h.set_window_ranges, None)
        h.reserve_results(reserve_bytes)
        undo.enter_context((req if bands is None else req.for_bands(idx)).applied(h, prep.xij))
        h.plan(sos, prep.zero_phase, prep.tl, prep.tr, prep.W[idx], prep.inc[idx], prep.vector_len, lts=prep.lts,
               xcorr_impl=xcorr_impl)
    if before_execute is not None:
        before_execute()
    h.stream_results(stream)             # (``stream``: the rows come back batch by batch, see ``process``)
    h.execute(after=after)


def all_window_times(prep, t0_datenum):
    return time_grid(t0_datenum, prep.fs, prep.W, prep.inc, prep.nwin, prep.vector_len)


def split_block(block, nbands, vector_len, mask_bytes):
    """A result block (bytes as the GPU wrote them, see nbls_result_layout) -> (grids (4, B, VL) float64,
    mask (B, VL, MB) uint8) views."""
    cells = nbands * vector_len
    grids = block[:32 * cells].view(np.float64).reshape(4, nbands, vector_len)
    mask = block[32 * cells:32 * cells + cells * mask_bytes].reshape(nbands, vector_len, mask_bytes)
    return grids, mask


def group_bounds(nwin, ngroups, cap, split=None):
    """Contiguous band groups by unit count -> (bounds [(b0, b1), ...], sequential).  ``split`` (``PIPELINE_SPLIT``, e.g.
    (0.15, 0.5, 0.35)): explicit shares, which also set the group count (a small first group gets the GPU started sooner,
    a small last group leaves less dictionary work after the GPU has finished).  The groups' filtered traces are in HBM
    side by side: if ``ngroups`` times the largest group exceeds ``cap`` bands, the call runs in consecutive rounds of
    <= ``cap`` bands on one handle instead (``sequential``)."""
    nb = len(nwin)
    if split and ngroups > 1:
        shares = [max(0.0, float(x)) for x in split]
        ngroups = max(1, min(len(shares), nb))
        shares = np.cumsum(shares[:ngroups]) / max(1e-30, float(np.sum(shares[:ngroups])))
    else:
        # mildly decreasing shares (0.41 / 0.33 / 0.26 for three groups): what is left to do on the host after the
        # GPU has finished is the dictionary of the LAST group (measured: 23.1 -> 22.6 ms per cfg-3 call)
        wts = 1.0 + 0.3 * np.arange(ngroups - 1, -1, -1)
        shares = np.cumsum(wts) / float(np.sum(wts))
    cum = np.concatenate(([0], np.cumsum(nwin)))
    cuts = [0]
    for g in range(1, ngroups):
        b = int(np.searchsorted(cum, cum[-1] * shares[g - 1]))
        cuts.append(min(max(b, cuts[-1] + 1), nb - (ngroups - g)))
    cuts.append(nb)
    bounds = [(cuts[g], cuts[g + 1]) for g in range(ngroups)]
    if max(b1 - b0 for b0, b1 in bounds) * ngroups > cap:           # HBM budget: consecutive rounds of <= cap bands
        return [(b0, min(b0 + cap, nb)) for b0 in range(0, nb, cap)], True
    return bounds, False


def choose_form(alpha, nwin, nchans, cap, groups=None, window_slice=None, single=False):
    """How ``process`` runs a call -> (streamed, bounds, sequential): ONE streamed pass where ``stream_pays``; else
    ``groups`` / ``pipeline_groups`` band groups side by side (one group for ``single`` calls — pre-filtered, on a given
    handle, without upload — and for OLS: nothing for the host to do per group); either way in rounds where HBM is short."""
    nb, npairs = len(nwin), nchans * (nchans - 1) // 2
    streamed = groups is None and window_slice is None and stream_pays(alpha, nwin, npairs)
    one_pass = (single or (alpha >= 1.0 and not os.environ.get('NBLS_PIPELINE_GROUPS'))) and groups is None
    ngroups = 1 if one_pass or streamed else (groups or pipeline_groups(nwin, npairs))
    bounds, sequential = group_bounds(nwin, max(1, min(ngroups, nb)), cap, PIPELINE_SPLIT if groups is None else None)
    return streamed, bounds, sequential


class _Notifier:
    """Tells the caller of ``process`` which rows are in ``res``: ``units_done(res, u0, u1)`` if given (flat unit index over
    all bands of the call, band-major), else ``group_done(res, b0, b1)`` for the bands a unit range completes, else
    nothing.  What lands before ``host_overlap`` has run (``ready``) is kept and replayed behind it, in band order."""

    def __init__(self, res, units_done, group_done):
        self.res, self.units_done, self.group_done = res, units_done, group_done
        self.cum = np.concatenate(([0], np.cumsum(res.nwin))).astype(np.int64)
        self.done_band = 0                            # bands [0, done_band) have been reported through group_done
        self.ready, self.deferred = False, []

    def units(self, b0, b1, u0, u1):
        """Units [u0, u1) of the pass over bands [b0, b1) have landed (a batch of a streamed pass)."""
        cum = self.cum
        g0, g1 = int(cum[b0]) + u0, int(cum[b0]) + u1
        if self.units_done is not None:
            if g1 > g0:
                self.units_done(self.res, g0, g1)
        elif self.group_done is not None:
            bd = int(np.searchsorted(cum, g1, side='right')) - 1       # bands complete up to unit g1
            bd = b1 if g1 >= cum[b1] else min(max(bd, self.done_band), b1)
            if bd > self.done_band:
                self.group_done(self.res, self.done_band, bd)
                self.done_band = bd

    def bands(self, b0, b1):
        """All rows of bands [b0, b1) have landed."""
        if not self.ready:
            self.deferred.append((b0, b1))
        elif self.units_done is not None:
            self.units(b0, b1, 0, int(self.cum[b1] - self.cum[b0]))
        elif self.group_done is not None:
            self.group_done(self.res, b0, b1)
            self.done_band = b1

    def replay(self):
        self.ready = True
        for b0, b1 in self.deferred:
            self.bands(b0, b1)


def fetch_groups(h, req, results, b0, b1, est=None):
    """Everything but the result block that the pass handle ``h`` has just run has, by the requests ``req`` of its call,
    into the rows of bands [b0, b1) of ``results``: the k ``BandBatch`` of the k recordings of the pass, whose row b * k + s
    is band b of recording s.  Each group of ``RESULT_GROUPS`` that applies is fetched once (its method once per call it
    lists; the beam trace once per result row) and, like the planes of ``EXTRA_FIELDS``, goes straight into the one result
    of a pass over one recording.  ``est``: the results of that estimator of the pass — the groups that take one only, and
    the index is passed to them.  The families of a pass that labels them (``req.families``) come as one table per pass,
    cut per recording by ``split_families``."""
    k, want, index = len(results), req.wants(), () if est is None else (est,)

    def put(name, a):
        if k == 1:
            getattr(results[0], name)[b0:b1] = a
        else:
            a = a.reshape((b1 - b0, k) + a.shape[1:])
            for j, res in enumerate(results):
                getattr(res, name)[b0:b1] = a[:, j]

    extras = {'want_' + name: True for name, _, _ in EXTRA_FIELDS if getattr(want, 'want_' + name)}
    if extras:
        ext = h.fetch(grids=False, **extras, **({} if est is None else dict(est=est)))
        for name in extras:
            put(name[len('want_'):], ext[name[len('want_'):]])
    for g in RESULT_GROUPS:
        if not g.applies(want) or (est is not None and not g.est):
            continue
        fetch = getattr(h, g.method)
        for args, fields in g.calls:
            if g.per_row:
                for j, res in enumerate(results):
                    for b in range(b0, b1):
                        getattr(res, fields[0][0])[b] = fetch((b - b0) * k + j)
                continue
            out = fetch(*args, *(index if g.est else ()))
            for (name, _, _), a in zip(fields, (out,) if len(fields) == 1 else out):
                put(name, a)
    if req.families is not None and est is None:
        family, _, table = h.fetch_families()
        parts = [(family, table)] if k == 1 else split_families(family, table, b1 - b0, k, family.shape[1])
        for res, (f, t) in zip(results, parts):
            res.family, res.family_table = f, t


def collect(res, h, b0, b1, streamed, note, req):
    """The rows of bands [b0, b1), whose pass handle ``h`` has just run with the requests ``req``, into ``res``; then
    (streamed and past ``host_overlap``: batch by batch) ``note`` is told."""
    live = streamed and note.ready
    drain(h, streamed, res.grids, res.mask, b0, b1, functools.partial(note.units, b0, b1) if live else None)
    fetch_groups(h, req, [res], b0, b1)
    if not live:
        note.bands(b0, b1)


def start_upload(data, fs, device):
    """``process``: unless these very buffers are in HBM already (``resident_trace``) or ``UPLOAD_OVERLAP`` is off, start
    the trace's upload to the call's first handle -> (``TraceUpload`` or None, resident)."""
    h0 = get_handle(device, 0)
    rk = getattr(h0, 'resident_key', None)
    if rk is not None and rk == _trace_key(data, fs):
        return None, True
    if not UPLOAD_OVERLAP:
        return None, False
    rows = list(np.ascontiguousarray(data, dtype=np.float64)) if isinstance(data, np.ndarray) else data
    return TraceUpload(h0, rows, fs, _upload_worker()), False


def launch_groups(data, rij, band_edges, winlens, prep_tail, res, bounds, sequential, streamed, up, resident, note,
                  handle=None, device=None, requests=Requests(), **launch_kw):
    """Design, plan and queue the pass of every band group (``prepare`` of its bands — ``prep_tail``: the arguments behind
    ``winlens`` — then ``launch`` with the group's share of ``requests``), group 0 while the trace is still going up (``up``).
    Sequential rounds share one handle: each is collected before the next is planned.  -> the (handle, b0, b1) still to
    collect."""
    launched, prep = [], None
    nchans, npts = _shape_of(data)
    for g, (b0, b1) in enumerate(bounds):
        prep = prepare(nchans, npts, res.fs, rij, band_edges[b0:b1], winlens[b0:b1], *prep_tail, common=prep,
                       windows=(res.W[b0:b1], res.inc[b0:b1], res.nwin[b0:b1], res.grids.shape[2]))
        res.sos.extend(prep.sos_ret)
        res.pair_idx, res.xij = prep.pair_idx, prep.xij
        h = handle if handle is not None else get_handle(device, 0 if sequential else g)
        if sequential and launched:               # one handle, one plan at a time: finish the previous round first
            collect(res, *launched.pop(), streamed, note, requests)
        joins = up is not None and g == 0                 # this launch rides on the upload thread's rows
        early = joins or (resident and (g == 0 or sequential))
        # the groups finish in the order they were queued (GPU-side ordering of their correlation stages): the
        # dictionary of group k is built while groups k+1.. are still running.  Left to itself the GPU shares
        # itself between the passes and all of them land together at the end (stream priorities alone did the
        # job on some boxes and not on others)
        ordered = launched and not sequential and GROUP_ORDER
        try:
            launch(h, data, prep, trace_from=launched[0][0] if (launched and not sequential) else None, trace_ready=early,
                   after=launched[-1][0] if ordered else None, stream=streamed,
                   before_execute=up.landed if (joins and not up.row_pipeline) else None,
                   requests=requests.for_bands(slice(b0, b1)), **launch_kw)
        except BaseException:
            if joins:
                up.landed()                       # the pass could not be queued: the upload's own error is the cause, if it has one
            raise
        if joins:
            up.landed()                           # (row_pipeline: the pass is queued, the library filters the rows as they land)
        launched.append((h, b0, b1))
        res.handle = h
    return launched


def label_result(h, res, par):
    """``res.family`` / ``res.family_table`` of a ``BandBatch`` whose bands did not run in one pass: the kernels of the in-pass
    request on the assembled grids (``Handle.label_families``)."""
    gate = par['sigma_tau_max'] is not None
    res.family, _, res.family_table = h.label_families(_hip.family_params(**par), 1, res.W, res.inc, res.nwin, res.vel, res.baz,
                                                       res.mdccm, res.sigma_tau if gate else None)


def split_families(family, table, nb, k, vector_len):
    """The labelling of a pass over k recordings (rows b * k + s) -> per recording (family (nb, vector_len), table) as a
    pass over that recording alone gives them: its families renumbered in their order, cells counted in its own lattice."""
    family = family.reshape(nb, k, vector_len)
    out = []
    for j in range(k):
        mine = np.flatnonzero(table[:, 5] == j)
        new_id = np.full(len(table) + 2, -1, dtype=np.int32)        # [-2] and [-1] keep their meaning
        new_id[-2] = -2
        new_id[mine] = np.arange(len(mine), dtype=np.int32)
        t = table[mine].copy()
        for col in (1, 2):
            t[:, col] = (t[:, col] // vector_len // k) * vector_len + t[:, col] % vector_len
        t[:, 5] = 0
        out.append((np.ascontiguousarray(new_id[family[:, j]]), t))
    return out


def process(data, fs, t0_datenum, rij, band_edges, winlens, winover, alpha, filter_type=None,
            filter_order=None, filter_ripple=None, vector_len=None, device=None, xcorr_impl=0,
            want_lag=False, want_cmax=False, want_z=False, prefiltered=False, handle=None,
            upload=True, window_slice=None, host_overlap=None, group_done=None, groups=None, units_done=None,
            want_uncert=False, want_beam=False, want_subsample=False, min_velocity=None, slowness_grid=None,
            want_grid_map=False, seed_halfwidths=None, want_consistency=False, capon_grid=None, capon_freqs=None,
            capon_snapshots=None, capon_loading=0.01, want_capon_maps=False, want_capon_csdm=False, capon_peaks=0,
            capon_peak_floor=0.25, capon_cells=None, kept=None, capon_clean=None, capon_music=None, families=None,
            grid_refine=None, element_max_shift=None, element_delays_kept=False, want_beam_trace=None, beam_taps=0):
    """Run the hot path for a list of bands on one GPU -> ``BandBatch``.

    data (N, npts) raw traces — a 2-D array or a list of N rows (uploaded from where they lie);
    band_edges [(fmin, fmax), ...]; winlens [seconds per band].
    prefiltered=True: ``data`` is already filtered/tapered (``ltsva`` entry), one band.
    window_slice=(k, n): process only the k-th of n contiguous window slices of every band (window
    sharding across GPUs); rows outside the slice stay zero, ``nwin``/``t`` describe the whole band.
    The keywords from ``want_uncert`` on, and ``want_lag`` / ``want_cmax`` / ``want_z``, are the opt-in requests of the call:
    ``Requests.check`` describes every one and the results it brings, and refuses a bad one (``ValueError``) before any GPU
    work.

    In this order:
    1. the trace starts going up on a helper thread (``start_upload``; not for a ``handle`` of the caller's, ``upload=False``
       or a resident trace); every way out from here on joins that copy;
    2. the windows of all bands are planned once; a trace of which not even one filtered band fits the HBM budget goes to
       ``process_segmented``;
    3. the form is chosen (``choose_form``): ONE pass whose unit batches — consecutive (band, window) units, each a complete
       correlate -> solve -> pack chain on the GPU — stream their rows to the host (``stream_pays``), or contiguous band
       groups, each an asynchronous pass on its own handle of the same GPU (small and OLS calls: one group, fetched in
       one piece); more bands than fit in HBM at once run in consecutive rounds on one handle;
    4. every group's filters are designed and its pass is queued (``launch_groups``), group 0 while the rows still go up;
    5. with everything queued, the host work that needs no GPU result: ``release_deferred``, the window times,
       ``host_overlap(res)`` (filter responses, key strings);
    6. the passes are collected in band order (``collect``).  ``units_done(res, u0, u1)`` runs as soon as the rows of the
       units [u0, u1) (flat index over all bands of the call, band-major) are in ``res`` — per batch of a streamed pass,
       while the GPU works on the next one —; without it ``group_done(res, b0, b1)`` runs for the bands a batch or a
       group completes (the caller builds its dictionary there).  Rounds collected in step 4 are reported after step 5."""
    asked = Requests.keywords_of(locals())
    nchans, npts = _shape_of(data)
    # (what is checked against the window lengths has them planned here already, before the upload starts)
    req = Requests.check(nchans, len(band_edges), fs, lambda: plan_windows(npts, fs, winlens, winover, vector_len)[0],
                         window_slice, rij=rij, **asked)
    fam = req.families
    cap = max_bands_per_pass(nchans, npts, 0 if req.beam_trace is None else 1)
    if cap < 1 and not prefiltered:
        req.segmented_refusal(nchans, npts, ('kept', 'capon_grid'))
    single = prefiltered or handle is not None or not upload
    up, resident = start_upload(data, fs, device) if upload and handle is None and (cap >= 1 or prefiltered) else (None, False)
    try:
        W, inc, nwin, vector_len = plan_windows(npts, fs, winlens, winover, vector_len)
        check_elements(nchans, alpha)
        if cap < 1 and not prefiltered:            # not even one band's filtered trace fits the HBM budget
            res = process_segmented(data, fs, t0_datenum, rij, band_edges, winlens, winover, alpha, filter_type, filter_order,
                                    filter_ripple, vector_len, device, xcorr_impl, want_lag, want_cmax, want_z, host_overlap,
                                    group_done, want_beam, want_subsample, min_velocity, slowness_grid, seed_halfwidths,
                                    want_consistency, element_max_shift, None if req.beam_trace is None else want_beam_trace,
                                    beam_taps=beam_taps)
            if fam is not None:
                label_result(res.handle if getattr(res, 'handle', None) is not None else get_handle(device, 0), res, fam)
            return res
        streamed, bounds, sequential = choose_form(alpha, nwin, nchans, max(1, cap), groups, window_slice, single)
        res = new_result(nchans, alpha, fs, W, inc, nwin, vector_len, **req.result_keywords(npts))
        res.families_in_pass = fam is not None and len(bounds) == 1      # (one pass covers every band: the in-pass request)
        if not res.families_in_pass:
            req = req.replace(families=None)
        note = _Notifier(res, units_done, group_done)
        launched = launch_groups(data, rij, band_edges, winlens, (winover, alpha, filter_type, filter_order, filter_ripple,
                                                                  vector_len, prefiltered),
                                 res, bounds, sequential, streamed, up, resident, note, handle, device, req, upload=upload,
                                 window_slice=window_slice, xcorr_impl=xcorr_impl)
    finally:
        if up is not None:
            up.close()
    # everything is queued: host work that needs no GPU result hides behind the passes
    release_deferred()
    res.t = time_grid(t0_datenum, fs, W, inc, nwin, vector_len)
    if host_overlap is not None:
        host_overlap(res)
    note.replay()
    for h, b0, b1 in launched:
        collect(res, h, b0, b1, streamed, note, req)
    if fam is not None and not res.families_in_pass:
        label_result(res.handle, res, fam)
    return res


MAX_ESTIMATORS = 8        # estimators of one multi-estimator call


def normalize_estimators(estimators, nchans):
    """``ESTIMATORS`` of the multi-estimator calls -> list of ``(alpha float, remove tuple of ascending ints)``; a bare
    number means ``(alpha, ())``.  ``ValueError`` (host-side, before any GPU work) for an empty list, more than
    ``MAX_ESTIMATORS``, an ALPHA outside [0.5, 1], a ``remove`` index that is out of range, given twice or not ascending,
    and fewer than 3 kept elements (4 under LTS)."""
    ests = list(estimators)
    if not ests:
        raise ValueError('ESTIMATORS is empty: at least one (ALPHA, remove) estimator is needed')
    if len(ests) > MAX_ESTIMATORS:
        raise ValueError('%d estimators: at most %d in one call' % (len(ests), MAX_ESTIMATORS))
    out = []
    for i, e in enumerate(ests):
        if isinstance(e, (tuple, list)):
            if len(e) != 2:
                raise ValueError('estimator %d: expected ALPHA or (ALPHA, remove)' % i)
            alpha, remove = float(e[0]), tuple(e[1])
        else:
            alpha, remove = float(e), ()
        if not (0.5 <= alpha <= 1.0):
            raise ValueError('estimator %d: ALPHA must be in [0.5, 1.0].' % i)
        idx = []
        for r in remove:
            if isinstance(r, bool) or int(r) != r:
                raise ValueError('estimator %d: remove holds %r, not a trace index' % (i, r))
            r = int(r)
            if not (0 <= r < nchans):
                raise ValueError('estimator %d: remove index %d is out of range for %d traces' % (i, r, nchans))
            if idx and r <= idx[-1]:
                raise ValueError('estimator %d: remove indices must ascend without repeats' % i)
            idx.append(r)
        kept = nchans - len(idx)
        if kept < 3:
            raise ValueError('estimator %d: %d elements kept, at least 3 are needed for the least squares estimate' % (i, kept))
        if alpha < 1.0 and kept < 4:
            raise ValueError('estimator %d: %d elements kept, at least 4 are needed for least trimmed squares' % (i, kept))
        out.append((alpha, tuple(idx)))
    return out


def kept_elements(nchans, remove):
    """The 0-based trace indices an estimator keeps, ascending."""
    gone = set(remove)
    return [i for i in range(nchans) if i not in gone]


def kept_pair_map(nchans, remove):
    """For every pair of the reduced array, in its own (lexicographic) order, the index of the same pair in the full
    array's pair list (what ``gather_pairs_kernel`` follows; the library builds its own from the kept elements)."""
    kept = kept_elements(nchans, remove)
    return np.array([a * (2 * nchans - a - 1) // 2 + (c - a - 1) for n, a in enumerate(kept) for c in kept[n + 1:]],
                    dtype=np.int32)


class _EstimatorResults:
    """What ``drain`` needs of a handle, for the results of estimator ``est`` of its pass."""

    def __init__(self, h, est):
        self.h, self.est = h, est
        self.profiling = False            # (the events of the pass are read once, through estimator 0)

    def fetch_packed(self):
        return self.h.fetch_packed(est=self.est)

    def result_batches(self):
        return self.h.result_batches()

    def wait_result_batch(self, k):
        return self.h.wait_result_batch(k, est=self.est)


def process_multi(data, fs, t0s, rijs, band_edges, winlens, winover, estimators, filter_type=None, filter_order=None,
                  filter_ripple=None, vector_len=None, device=None, prefiltered=False, want_uncert=False, want_lag=False,
                  want_cmax=False, host_overlap=None, units_done=None, want_beam=False, want_subsample=False,
                  min_velocity=None, want_consistency=False, want_beam_trace=None):
    """``process`` for several estimators ``(alpha, remove)`` of ONE trace in one device pass -> a list of ``BandBatch``,
    element e what ``process`` gives for ``alpha_e`` on the rows that ``remove_e`` leaves (``estimators`` as
    ``normalize_estimators`` returns them; ``rijs[e]``: the (2, kept) geometry of estimator e, ``t0s[e]`` its start date).

    The full array is filtered and correlated once; every unit is then solved once per estimator, a sub-array's on compact
    copies of its pairs' lags (``nbls_set_estimators``).  Estimator 0 of the pass is the first estimator that removes
    nothing — or, when every one removes something, an OLS solve of the full array whose rows are not returned.  Every
    estimator's geometry goes through the host functions of a single call on its rows (``planner.co_array``, ``lts_plan``,
    ``uncertainty_frame``).  The bands run in rounds where HBM is short (``max_bands_per_pass``); the rows come back in one
    piece or, where ``stream_pays`` for the most demanding estimator, batch by batch — estimator by estimator, each through
    ``drain``.  ``host_overlap(results)`` runs once the first pass is queued; ``units_done(e, res, u0, u1)`` when the
    units [u0, u1) (flat over all bands) of estimator e are in ``results[e]``.  ``want_beam``: every estimator's
    ``beam_power`` / ``fstat``, of ITS elements at ITS slowness (``process``).  ``want_subsample``: the pass refines the full
    array's lags once and every estimator solves on the refined delays of ITS pairs (``lag_frac`` with ``want_lag``).
    ``min_velocity``: the full array's lags are searched within their physical range (``process``); a sub-array reads them.
    ``want_consistency``: every estimator's ``consistency`` / ``closure_max`` / ``element_consistency``, the closure of the
    picked lags over the triplets of ITS elements (``process``).  ``want_beam_trace``: refused (``ValueError``) — the beam trace
    is estimator 0's, further estimators are out of its scope."""
    asked = Requests.keywords_of(locals())
    if want_beam_trace is not None and want_beam_trace is not False:
        raise ValueError('want_beam_trace: the beam trace is not available with several estimators (nbls_set_beam_trace is '
                         'refused beside nbls_set_estimators)')
    rows = list(np.ascontiguousarray(data, dtype=np.float64)) if isinstance(data, np.ndarray) else data
    nchans, npts = _shape_of(rows)
    nb = len(band_edges)
    cap = max_bands_per_pass(nchans, npts)
    if cap < 1 and not prefiltered:
        raise ValueError('not even one filtered band of %d x %d samples fits the HBM budget of one pass' % (nchans, npts))
    cap = max(1, cap)
    full = next((i for i, (_, rm) in enumerate(estimators) if not rm), None)
    order = ([full] if full is not None else []) + [i for i in range(len(estimators)) if i != full]
    alpha0 = estimators[full][0] if full is not None else 1.0
    rij0 = rijs[full] if full is not None else rijs[-1]        # (no full-array estimator: ``rijs`` ends with the full geometry)
    first_est = 0 if full is not None else 1                   # device index of order[0]
    req = Requests.check(nchans, nb, fs, None, rij=rij0, **asked)          # (of the full array; a sub-array reads its lags)
    extras = []
    for i in (order[1:] if full is not None else order):
        alpha, remove = estimators[i]
        xij, pair_idx, xpinv = planner.co_array(rijs[i])
        extras.append(dict(kept=kept_elements(nchans, remove), xij=xij, pair_idx=pair_idx, xpinv=xpinv,
                           lts=planner.lts_plan(xij, alpha) if alpha < 1.0 else None,
                           eig6=planner.uncertainty_frame(xij) if want_uncert else None))
    W, inc, nwin, vector_len = plan_windows(npts, fs, winlens, winover, vector_len)
    check_elements(nchans, alpha0)
    results = [None] * len(estimators)
    for i, (alpha, remove) in enumerate(estimators):
        res = new_result(nchans - len(remove), alpha, fs, W, inc, nwin, vector_len, **req.result_keywords(npts))
        res.xij, res.pair_idx, _ = planner.co_array(rijs[i])
        results[i] = res
    streamed = stream_pays(min(a for a, _ in estimators), nwin, nchans * (nchans - 1) // 2)
    cum = np.concatenate(([0], np.cumsum(nwin))).astype(np.int64)
    h = get_handle(device, 0)
    up, resident = start_upload(rows, fs, device)
    prep, told = None, False
    try:
        for b0 in range(0, nb, cap):
            b1 = min(nb, b0 + cap)
            prep = prepare(nchans, npts, fs, rij0, band_edges[b0:b1], winlens[b0:b1], winover, alpha0, filter_type,
                           filter_order, filter_ripple, vector_len, prefiltered, common=prep,
                           windows=(W[b0:b1], inc[b0:b1], nwin[b0:b1], vector_len))
            joins = up is not None and b0 == 0
            try:
                launch(h, rows, prep, trace_ready=joins or resident or b0 > 0, stream=streamed, requests=req,
                       before_execute=up.landed if (joins and not up.row_pipeline) else None, estimators=extras)
            finally:
                if joins:
                    up.landed()
            for res in results:
                res.sos.extend(prep.sos_ret)
                res.handle = h
            if not told:                   # the pass is queued: host work that needs no GPU result
                told = True
                release_deferred()
                grids = {}
                for res, t0 in zip(results, t0s):
                    if t0 not in grids:
                        grids[t0] = time_grid(t0, fs, W, inc, nwin, vector_len)
                    res.t = grids[t0]
                if host_overlap is not None:
                    host_overlap(results)
            for n, i in enumerate(order):
                res, est = results[i], n + first_est
                view = h if est == 0 else _EstimatorResults(h, est)
                done = None
                if units_done is not None and streamed:
                    done = functools.partial(_multi_units, units_done, i, res, int(cum[b0]))
                drain(view, streamed, res.grids, res.mask, b0, b1, done)
                if units_done is not None and not streamed:
                    units_done(i, res, int(cum[b0]), int(cum[b1]))
                fetch_groups(h, req, [res], b0, b1, est)
    finally:
        if up is not None:
            up.close()
        h.set_estimators(())              # the handle is shared with the plain calls: back to the plain pass
    return results


def _multi_units(units_done, e, res, base, u0, u1):
    if u1 > u0:
        units_done(e, res, base + u0, base + u1)


def batch_rows(streams):
    """Several recordings of one array -> (per recording the ``stream_rows`` list of rows, fs, per recording the start
    date number).  Every recording must have the same element count, sample count and sampling rate: ``ValueError``
    naming the mismatch otherwise (host-side only, before any GPU work)."""
    rows, t0s = [], []
    fs = npts = nchans = None
    for i, st in enumerate(streams):
        r, f, t0 = stream_rows(st)
        if nchans is None:
            nchans, npts, fs = len(r), len(r[0]), f
        elif len(r) != nchans:
            raise ValueError('recording %d has %d elements, recording 0 has %d' % (i, len(r), nchans))
        elif len(r[0]) != npts:
            raise ValueError('recording %d has %d samples per trace, recording 0 has %d' % (i, len(r[0]), npts))
        elif f != fs:
            raise ValueError('recording %d is sampled at %r Hz, recording 0 at %r Hz' % (i, f, fs))
        rows.append(r)
        t0s.append(t0)
    return rows, fs, t0s


def process_batch(recordings, fs, t0s, rij, band_edges, winlens, winover, alpha, filter_type=None, filter_order=None,
                  filter_ripple=None, vector_len=None, device=None, prefiltered=False, want_uncert=False, want_beam=False,
                  want_subsample=False, min_velocity=None, slowness_grid=None, want_grid_map=False, seed_halfwidths=None,
                  want_consistency=False, capon_grid=None, capon_freqs=None, capon_snapshots=None, capon_loading=0.01,
                  want_capon_maps=False, want_capon_csdm=False, capon_peaks=0, capon_peak_floor=0.25, capon_cells=None,
                  kept=None, capon_clean=None, capon_music=None, families=None, grid_refine=None, element_max_shift=None,
                  element_delays_kept=False, want_beam_trace=None, beam_taps=0):
    """``process`` for S recordings of ONE array (``recordings[s]``: the N rows of recording s, all of one length and
    rate, one geometry ``rij``) in one device pass -> a list of S ``BandBatch``, element s what ``process`` gives for
    recording s alone (bit for bit: the kernels see the same per-row work).

    The S*N rows go up as one trace of S segments (``nbls_set_segments``); a plan of B bands then holds B*S result rows,
    row b*S + s.  The bands of a batch whose filtered traces do not fit the HBM budget (``max_bands_per_pass`` of S*N rows)
    run in consecutive rounds; if not even one band of the whole batch fits, the batch is cut into sub-batches of as many
    recordings as fit.  A batch never takes the time-segmented path.  The passes are fetched in one piece, or streamed
    batch by batch where ``stream_pays`` (per-row windows) says so; either way every recording's rows are complete before
    its dictionary is built (the caller's side: rows of one recording are spread over all bands).  The opt-in keywords are
    those of ``process``, checked the same way and in the same order (``Requests.check``)."""
    asked = Requests.keywords_of(locals())
    S = len(recordings)
    nchans, npts = len(recordings[0]), len(recordings[0][0])
    nb = len(band_edges)
    req = Requests.check(nchans, nb, fs, lambda: plan_windows(npts, fs, winlens, winover, vector_len)[0], rij=rij, **asked)
    prep = prepare(nchans, npts, fs, rij, band_edges, winlens, winover, alpha, filter_type, filter_order, filter_ripple,
                   vector_len, prefiltered)
    VL, P, MB = prep.vector_len, prep.npairs, prep.mask_bytes
    fam, tr = req.families, 0 if req.beam_trace is None else 1     # (tr: rows of the beam trace per recording and band, beside its N filtered ones)
    per_sub = S if max_bands_per_pass(S * nchans, npts, S * tr) >= 1 else max_bands_per_pass(nchans, npts, tr)
    if per_sub < 1:
        raise ValueError('a recording of %d x %d samples does not fit the HBM budget of one pass (NBLS_MAX_FILTERED_GB): '
                         'process it on its own' % (nchans, npts))
    out = [new_result(nchans, alpha, fs, prep.W, prep.inc, prep.nwin, VL, **req.result_keywords(npts)) for _ in range(S)]
    h = get_handle(device, 0)
    try:
        for s0 in range(0, S, per_sub):
            k = min(per_sub, S - s0)
            h.set_segments(k)
            h.set_trace_rows([r for rec in recordings[s0:s0 + k] for r in rec], fs)
            cap = max(1, max_bands_per_pass(k * nchans, npts, k * tr))
            streamed = stream_pays(alpha, np.tile(prep.nwin, k), P)
            # (the families are labelled in the pass where one pass covers every band of these recordings)
            passes = req if (fam is not None and cap >= nb) else req.replace(families=None)
            for b0 in range(0, nb, cap):
                b1 = min(nb, b0 + cap)
                R = (b1 - b0) * k
                launch(h, None, prep, bands=list(range(b0, b1)), trace_ready=True, stream=streamed, requests=passes)
                g = np.zeros((4, R, VL))
                m = np.zeros((R, VL, MB), dtype=np.uint8)
                drain(h, streamed, g, m, 0, R)
                g = g.reshape(4, b1 - b0, k, VL)
                m = m.reshape(b1 - b0, k, VL, MB)
                for j, res in enumerate(out[s0:s0 + k]):
                    res.grids[:, b0:b1] = g[:, :, j]
                    res.mask[b0:b1] = m[:, j]
                fetch_groups(h, passes, out[s0:s0 + k], b0, b1)
    finally:
        h.set_segments(1)
    for res, t0 in zip(out, t0s):
        res.t = time_grid(t0, fs, prep.W, prep.inc, prep.nwin, VL)
        res.sos, res.pair_idx, res.xij, res.handle = list(prep.sos_ret), prep.pair_idx, prep.xij, h
        if fam is not None and getattr(res, 'family', None) is None:     # (several rounds: the kernels on the assembled grids)
            label_result(h, res, fam)
    return out



def time_keys(t, nwin, prefixes=None):
    """The ``stdict`` key text of every (band, window): prefix + ``str(numpy.float64 time)`` — repr of a
    Python float is the same shortest round-trip text.  -> ONE flat list of strings, bands in order,
    ``nwin[b]`` keys per band.  Needs no GPU result, so the band loop computes it while the pass is running."""
    if _hostext is not None:
        return _hostext.time_keys(np.ascontiguousarray(t, dtype=np.float64), np.ascontiguousarray(nwin, dtype=np.int64),
                                  None if prefixes is None else list(prefixes))
    return _py_time_keys(t, nwin, prefixes)


def time_key_text(t, nwin, prefixes=None):
    """``time_keys`` without the string objects: the key TEXT of every (band, window) as a ``(text (K, 40) uint8,
    length (K,) uint8)`` pair, formatted in C++ with the GIL released on a few threads.  ``stdict_from_mask`` takes
    the pair in place of the key list and makes a string only for the windows that get an entry.  Without the
    helper module this is ``time_keys`` (a list)."""
    if _hostext is not None and hasattr(_hostext, 'time_key_text'):
        return _hostext.time_key_text(np.ascontiguousarray(t, dtype=np.float64), np.ascontiguousarray(nwin, dtype=np.int64),
                                      None if prefixes is None else list(prefixes), _key_threads())
    return _py_time_keys(t, nwin, prefixes)


def _key_threads():
    if KEY_THREADS:
        return max(1, int(KEY_THREADS))
    try:
        n = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        n = os.cpu_count() or 1
    return max(1, min(4, n - 1))


def n_keys(keys):
    """Number of keys in a ``time_keys`` list or a ``time_key_text`` pair."""
    return len(keys[1]) if isinstance(keys, tuple) else len(keys)


def _py_time_keys(t, nwin, prefixes=None):
    out = []
    for b in range(len(nwin)):
        p = '' if prefixes is None else prefixes[b]
        reps = map(repr, np.asarray(t[b, :int(nwin[b])], dtype=np.float64).tolist())
        out.extend([p + s for s in reps] if p else reps)
    return out


def new_stdict(nkeys):
    """An empty dictionary with room for ``nkeys`` entries (no re-hashing while a call's ~5*10^4 keys go in)."""
    if _hostext is not None:
        return _hostext.new_dict(int(nkeys) + 1)
    return {}


def new_pattern_cache():
    """Holder of the shared value arrays for the ``stdict_from_mask`` calls of ONE pipelined call (one per band group):
    a dropped-pair pattern met in an earlier group is not built again.  None without the helper module."""
    if _hostext is not None and hasattr(_hostext, 'new_pattern_cache'):
        return _hostext.new_pattern_cache()
    return None


def stdict_from_mask(mask, nwin, pair_idx, nchans, keys, into=None, k0=0, cache=None, units=None):
    """lts_array's dropped-element dictionary for ALL bands of a pass from the packed weight mask
    (B, VL, ceil(P/8)): key (``keys[b][w]``, see ``time_keys``) -> 1-based element numbers of both
    members of every zero-weight pair (first members, then second members), only for windows that
    dropped something; ``'size'`` -> number of elements.  Entries are inserted in (band, window) order as
    the reference's loops do (narrow_band_least_squares.py:114-124; ``'size'`` therefore sits right after
    the first band's entries).

    Windows that dropped the SAME set of pairs share ONE read-only array (the reference makes a fresh
    array per window; the values are equal, and an in-place write raises instead of aliasing): creating
    ~5*10^4 tiny arrays per call costs as much host time as the whole GPU pass.  With the C++ helper
    module built, one C++ pass does the work; the NumPy form below is its equivalent.

    ``into`` / ``k0``: update an existing dictionary with the bands of one group of a pipelined call (``k0`` =
    index in ``keys`` of this mask's first window); 'size' is only placed by the call that starts the dictionary.

    ``units=(u0, u1)``: enter only the units [u0, u1) of the flattened (band, window) order of ``mask`` / ``nwin`` (the
    batches of a streamed pass; consecutive ranges in ascending order); 'size' goes in with the range that holds the
    first band's last window."""
    if _hostext is not None:
        u0, u1 = (-1, -1) if units is None else (int(units[0]), int(units[1]))
        return _hostext.build_stdict(np.ascontiguousarray(mask, dtype=np.uint8), np.ascontiguousarray(nwin, dtype=np.int64),
                                     np.ascontiguousarray(pair_idx, dtype=np.int32), int(nchans), keys, into, int(k0), cache, u0, u1)
    return _py_stdict_from_mask(mask, nwin, pair_idx, nchans, keys, into, k0, units)


def _py_stdict_from_mask(mask, nwin, pair_idx, nchans, keys, into=None, k0=0, units=None):
    if units is not None:
        # a unit range: the bands it touches, cut at the end of the first band ('size' follows that band's entries)
        u0, u1 = int(units[0]), int(units[1])
        nw = np.asarray(nwin, dtype=np.int64)
        cum = np.concatenate(([0], np.cumsum(nw)))
        stdict = {} if into is None else into
        B, VL, MB = mask.shape
        flat_keys = keys
        if isinstance(keys, tuple):
            text, length = keys
            flat_keys = [bytes(text[i, :length[i]]).decode('ascii') for i in range(len(length))]
        full = np.packbits(np.ones(len(pair_idx), dtype=np.uint8), bitorder='little')
        pidx = np.asarray(pair_idx)
        for b in range(B):
            lo, hi = max(u0, int(cum[b])), min(u1, int(cum[b + 1]))
            for u in range(lo, hi):
                m = mask[b, u - int(cum[b])]
                if ((m & full) != full).any():
                    cols = np.nonzero(np.unpackbits(m, bitorder='little')[:len(pidx)] == 0)[0]
                    arr = np.concatenate((pidx[cols, 0] + 1, pidx[cols, 1] + 1)).astype((pidx[:1, 0] + 1).dtype, copy=False)
                    arr.flags.writeable = False
                    stdict[flat_keys[k0 + u]] = arr
            if b == 0 and ((u0 < nw[0] <= u1) or (nw[0] == 0 and u0 == 0)):
                stdict['size'] = nchans
        return stdict
    if isinstance(keys, tuple):                                  # (text, length) of time_key_text
        text, length = keys
        keys = [bytes(text[i, :length[i]]).decode('ascii') for i in range(len(length))]
    pair_idx = np.asarray(pair_idx)
    P = len(pair_idx)
    B, VL, MB = mask.shape
    nwin = np.asarray(nwin, dtype=np.int64)
    valid = np.arange(VL)[None, :] < nwin[:, None]
    m = mask[valid]                                              # (U, MB), (band, window) order
    full = np.packbits(np.ones(P, dtype=np.uint8), bitorder='little')
    hit = ((m & full[None, :]) != full[None, :]).any(axis=1)
    stdict = {} if into is None else into
    fresh = len(stdict) == 0
    keys = keys[k0:k0 + len(hit)] if (k0 or len(keys) != len(hit)) else keys
    n = int(np.count_nonzero(hit))
    if n:
        sel = np.ascontiguousarray(m[hit])
        if MB <= 8:                                              # pattern code of every window
            code = np.zeros(n, dtype=np.uint64)
            for i in range(MB):
                code |= sel[:, i].astype(np.uint64) << np.uint64(8 * i)
        else:
            code = sel.view(np.dtype((np.void, MB))).ravel()
        _, first, inv = np.unique(code, return_index=True, return_inverse=True)
        one = (pair_idx[:1, 0] + 1).dtype
        pats = []
        for row in np.unpackbits(sel[first], axis=1, bitorder='little')[:, :P]:
            cols = np.nonzero(row == 0)[0]
            arr = np.concatenate((pair_idx[cols, 0] + 1, pair_idx[cols, 1] + 1)).astype(one, copy=False)
            arr.flags.writeable = False
            pats.append(arr)
        pieces = operator.itemgetter(*inv.ravel().tolist())(pats) if n > 1 else (pats[0],)
        items = zip(itertools.compress(keys, hit.tolist()), pieces)
        # key order of the reference's merge loop: the first band's time keys, 'size', then the other bands
        if fresh:
            stdict.update(itertools.islice(items, int(np.count_nonzero(hit[:int(nwin[0])]))))
            stdict['size'] = nchans
        stdict.update(items)
    if fresh:
        stdict['size'] = nchans
    return stdict


def stdict_from_weights(weights_row, nwin, t_row, pair_idx, nchans, prefix=''):
    """Single-band form of ``stdict_from_mask`` taking unpacked weights (nwin.., P) uint8 and the window
    times: key ``prefix + str(t)`` (``prefix`` = the band prefix of narrow_band_least_squares.py:114-124)."""
    nwin = int(nwin)
    w = np.asarray(weights_row[:nwin]) != 0
    mask = np.packbits(w, axis=-1, bitorder='little')[None, :, :]
    keys = time_keys(np.asarray(t_row, dtype=np.float64)[None, :nwin], [nwin], [prefix] if prefix else None)
    return stdict_from_mask(mask, [nwin], pair_idx, nchans, keys)
