"""Worker of tests/test_gpu_music.py: a handle with an RCCL communicator (a world of one over the loopback stand-in named in
NBLS_TEST_TRANSPORT) must refuse a plan that asks for the Capon spectra with a MUSIC request — the gathered block carries
neither —, and plan as before without them.  A process of its own: a communicator lives as long as its process."""
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
    rij = synthetic.array_geometry(4, 1.0)
    data = synthetic.plane_wave(rij, 1201, 20.0, 0.5, 4.0)
    xij, pair_idx, xpinv = planner.co_array(rij)
    h.set_trace(data, 20.0)
    h.set_geometry(xij, pair_idx, xpinv)
    grid = planner.slowness_grid(3.07, 5)
    W, inc = np.array([65], dtype=np.int32), np.array([32], dtype=np.int32)
    h.set_capon(grid, [1.3], [16], [8])
    h.set_capon_music(2, 0.05, True, True)
    try:                                             # (the Python wrapper reports NBLS_ERR_UNSUPPORTED as ValueError)
        h.plan(None, False, None, None, W, inc, 40)
        raise SystemExit('a plan with a MUSIC request was accepted on a handle with a communicator')
    except ValueError as e:
        assert 'nbls_set_capon' in str(e), e
    h.set_capon(None)
    try:                                             # the request alone: no spectra to work on
        h.plan(None, False, None, None, W, inc, 40)
        raise SystemExit('a plan with a MUSIC request and no Capon spectra was accepted')
    except _hip.NblsError as e:
        assert e.code == _hip.NBLS_ERR_STATE and 'nbls_set_capon_music' in str(e), e
    h.set_capon_music(None)
    h.plan(None, False, None, None, [65], [32], 40)
    h.execute()
    assert np.any(h.fetch()['vel'] != 0)
    for fetch in (h.fetch_capon_music, h.fetch_capon_music_map, h.fetch_capon_music_vectors):
        try:
            fetch()
            raise SystemExit('a fetch of MUSIC results of a plan without them returned')
        except _hip.NblsError as e:
            assert e.code == _hip.NBLS_ERR_STATE, e
    print('MUSIC_COMM_OK')


if __name__ == '__main__':
    main()
