"""MI355X-native narrow-band least-squares / least-trimmed-squares array processing.

Same Python call surface as amiezzi/narrow_band_least_squares (+ ``lts_array.ltsva``); the
(band x window) hot path runs in hand-written HIP kernels behind the C ABI of
``include/nbls.h`` (ctypes, no PyTorch on the compute path).  There is no CPU fallback.
"""
import sys as _sys

from .narrow_band_least_squares import (narrow_band_least_squares, narrow_band_loop,
                                        narrow_band_least_squares_parallel, narrow_band_least_squares_batch,
                                        narrow_band_least_squares_multi, narrow_band_least_squares_beam,
                                        narrow_band_least_squares_subsample, narrow_band_least_squares_bounded,
                                        narrow_band_least_squares_grid, narrow_band_least_squares_seeded,
                                        narrow_band_least_squares_consistency, narrow_band_least_squares_capon,
                                        narrow_band_least_squares_kept, narrow_band_least_squares_beam_trace,
                                        narrow_band_least_squares_element_delays, narrow_band_least_squares_clean,
                                        narrow_band_least_squares_music, narrow_band_least_squares_families,
                                        narrow_band_least_squares_families_batch, label_families,
                                        narrow_band_least_squares_steered, narrow_band_least_squares_grid_refined)
from .lts_array import ltsva, ltsva_batch, ltsva_multi, ltsva_beam, ltsva_subsample, ltsva_bounded, ltsva_grid, \
    ltsva_seeded, ltsva_consistency, ltsva_capon, ltsva_capon_batch, ltsva_kept, ltsva_kept_batch, ltsva_beam_trace, \
    ltsva_beam_trace_batch, ltsva_steered, ltsva_steered_batch, ltsva_element_delays, ltsva_element_delays_batch, \
    ltsva_clean, ltsva_clean_batch, clean_map, clean_sources, ltsva_music, ltsva_music_batch, ltsva_families, \
    ltsva_families_batch, ltsva_grid_refined, ltsva_grid_refined_batch
from .helpers import (get_freqlist, get_winlenlist, filter_data, make_float, get_rij,
                      write_txtfile, read_txtfile)
from .stream import Stream, Trace, Stats
from .engine import resident_trace

__all__ = ['narrow_band_least_squares', 'narrow_band_loop', 'narrow_band_least_squares_parallel',
           'ltsva', 'get_freqlist', 'get_winlenlist', 'filter_data', 'make_float', 'get_rij',
           'write_txtfile', 'read_txtfile', 'Stream', 'Trace', 'Stats', 'install_as_reference_modules', 'resident_trace',
           'narrow_band_least_squares_batch', 'ltsva_batch', 'narrow_band_least_squares_multi', 'ltsva_multi',
           'narrow_band_least_squares_beam', 'ltsva_beam', 'narrow_band_least_squares_subsample', 'ltsva_subsample',
           'narrow_band_least_squares_bounded', 'ltsva_bounded', 'narrow_band_least_squares_grid', 'ltsva_grid',
           'narrow_band_least_squares_seeded', 'ltsva_seeded', 'narrow_band_least_squares_consistency', 'ltsva_consistency',
           'narrow_band_least_squares_capon', 'ltsva_capon', 'ltsva_capon_batch',
           'narrow_band_least_squares_kept', 'ltsva_kept', 'ltsva_kept_batch',
           'narrow_band_least_squares_beam_trace', 'ltsva_beam_trace', 'ltsva_beam_trace_batch',
           'narrow_band_least_squares_steered', 'ltsva_steered', 'ltsva_steered_batch',
           'narrow_band_least_squares_element_delays', 'ltsva_element_delays', 'ltsva_element_delays_batch',
           'narrow_band_least_squares_clean', 'ltsva_clean', 'ltsva_clean_batch', 'clean_map', 'clean_sources',
           'narrow_band_least_squares_music', 'ltsva_music', 'ltsva_music_batch',
           'narrow_band_least_squares_families', 'narrow_band_least_squares_families_batch', 'ltsva_families',
           'ltsva_families_batch', 'label_families',
           'narrow_band_least_squares_grid_refined', 'ltsva_grid_refined', 'ltsva_grid_refined_batch']


def install_as_reference_modules():
    """Register this package's modules under the reference's module names, so that a script
    written like the reference's example.py (``from narrow_band_least_squares import ...``,
    ``from helpers import ...``, ``from lts_array import ltsva``) runs on the GPU path unchanged."""
    # (the package attribute `narrow_band_least_squares` is the function; fetch the modules by name)
    for name in ('narrow_band_least_squares', 'helpers', 'lts_array'):
        _sys.modules[name] = _sys.modules[__name__ + '.' + name]
