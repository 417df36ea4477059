"""Worker of tests/test_gpu_element_delay.py: a handle with an RCCL communicator (a world of one over the loopback stand-in
named in NBLS_TEST_TRANSPORT) refuses a plan with element delays — the gathered block does not carry them — and plans as
before once the request is off.  A process of its own: a communicator lives as long as its process."""
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
    h.set_element_delays([3])
    try:                                         # (the Python wrapper reports NBLS_ERR_UNSUPPORTED as ValueError)
        h.plan(None, False, None, None, [65], [32], 40)
        raise SystemExit('a plan with element delays was accepted on a handle with a communicator')
    except ValueError as e:
        assert e.code == _hip.NBLS_ERR_UNSUPPORTED and 'nbls_set_element_delays' in str(e), e
    h.set_element_delays(None)
    h.plan(None, False, None, None, [65], [32], 40)
    h.execute()
    assert np.any(h.fetch()['vel'] != 0)
    print('ELEMENT_DELAY_COMM_OK')


if __name__ == '__main__':
    main()
