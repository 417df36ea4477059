"""Worker of tests/test_gpu_beam_trace.py: a handle with an RCCL communicator (a world of one over the loopback stand-in named
in NBLS_TEST_TRANSPORT) must refuse a plan that asks for the beam trace — the gathered block does not carry it —, gated or
not, and plan as before without the request.  A process of its own: a communicator lives as long as its process."""
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
    W, inc = np.array([65], dtype=np.int32), np.array([32], dtype=np.int32)
    ip = C.POINTER(C.c_int32)
    for gate in (None, 0.5):
        h.set_beam_trace(planner.beam_trace_window(65), gate)
        rc = h.lib.nbls_plan(h._h, 1, None, 0, 0, None, None, 0, W.ctypes.data_as(ip), inc.ctypes.data_as(ip), 40, None, 0)
        assert rc == _hip.NBLS_ERR_UNSUPPORTED, (gate, rc)
        assert b'nbls_set_beam_trace' in h.lib.nbls_last_error(h._h)
        try:                                         # (the Python wrapper reports NBLS_ERR_UNSUPPORTED as ValueError)
            h.plan(None, False, None, None, W, inc, 40)
            raise SystemExit('a plan with the beam trace was accepted on a handle with a communicator')
        except ValueError as e:
            assert 'nbls_set_beam_trace' in str(e), e
        h.set_beam_trace(None)
        h.plan(None, False, None, None, [65], [32], 40)
        h.execute()
        assert np.any(h.fetch()['vel'] != 0)
        try:
            h.fetch_beam_trace(0)
            raise SystemExit('a fetch of the beam trace of a plan without it returned')
        except _hip.NblsError as e:
            assert e.code == _hip.NBLS_ERR_STATE, e
    print('BEAM_TRACE_COMM_OK')


if __name__ == '__main__':
    main()
