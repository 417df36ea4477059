"""Worker of tests/test_gpu_grid_refine.py: a handle with an RCCL communicator (a world of one over the loopback stand-in named
in NBLS_TEST_TRANSPORT) refuses a plan that refines its grid maximum as it refuses the grid itself — the gathered block
carries neither — and plans as before once the requests are off.  A process of its own: a communicator lives as long as its
process."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from narrow_band_least_squares_amd import _hip, dist, engine, planner, synthetic
    dist.set_transport_library(os.environ['NBLS_TEST_TRANSPORT'], allow_shared_device=True)
    h = engine.get_handle()
    uid = (C.c_char * 128)()
    assert h.lib.nbls_comm_unique_id(uid, 128) == 0
    h._chk(h.lib.nbls_comm_init_rank(h._h, bytes(uid), 1, 0))
    rij = synthetic.array_geometry(4, 0.15)
    data = synthetic.plane_wave(rij, 1201, 20.0, 0.5, 4.0)
    xij, pair_idx, xpinv = planner.co_array(rij)
    h.set_trace(data, 20.0)
    h.set_geometry(xij, pair_idx, xpinv)
    h.set_beam_interpolation(8)
    h.set_beam_grid(np.array([[a, b] for a in (-1.0, 0.0, 1.0) for b in (-1.0, 0.0, 1.0)]))
    h.set_beam_grid_refinement(4, (1.0, 1.0))
    try:                                         # (the Python wrapper reports NBLS_ERR_UNSUPPORTED as ValueError)
        h.plan(None, False, None, None, [65], [32], 40)
        raise SystemExit('a refining plan was accepted on a handle with a communicator')
    except ValueError as e:
        assert e.code == _hip.NBLS_ERR_UNSUPPORTED and 'RCCL communicator' in str(e), e
    h.set_beam_grid(None)
    try:                                         # the refinement alone: no grid to refine
        h.plan(None, False, None, None, [65], [32], 40)
        raise SystemExit('a plan that refines without a grid was accepted')
    except _hip.NblsError as e:
        assert e.code == _hip.NBLS_ERR_STATE, e
    h.set_beam_grid_refinement(0, None)
    h.set_beam_interpolation(0)
    h.plan(None, False, None, None, [65], [32], 40)
    h.execute()
    assert np.any(h.fetch()['vel'] != 0)
    print('GRID_REFINE_COMM_OK')


if __name__ == '__main__':
    main()
