"""Worker of tests/test_gpu_families.py: a handle with an RCCL communicator (a world of one over the loopback stand-in named
in NBLS_TEST_TRANSPORT) must refuse a plan that asks for families — the gathered block does not carry them — and plan as
before without the request; ``label_families`` works on such a handle.  A process of its own: a communicator lives as long
as its process."""
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
    par = _hip.family_params(0.5, 0.2, 0.6, None, 5.0, 0.05, 1, 1, 1)
    h.set_families(par)
    rc = h.lib.nbls_plan(h._h, 1, None, 0, 0, None, None, 0, W.ctypes.data_as(ip), inc.ctypes.data_as(ip), 40, None, 0)
    assert rc == _hip.NBLS_ERR_UNSUPPORTED, rc
    assert b'nbls_set_families' in h.lib.nbls_last_error(h._h)
    try:                                         # (the Python wrapper reports NBLS_ERR_UNSUPPORTED as ValueError)
        h.plan(None, False, None, None, W, inc, 40)
        raise SystemExit('a plan with families was accepted on a handle with a communicator')
    except ValueError as e:
        assert 'nbls_set_families' in str(e), e
    h.set_families(None)
    h.plan(None, False, None, None, [65], [32], 40)
    h.execute()
    r = h.fetch()
    assert np.any(r['vel'] != 0)
    try:
        h.fetch_families()
        raise SystemExit('a fetch of the families of a plan without them returned')
    except _hip.NblsError as e:
        assert e.code == _hip.NBLS_ERR_STATE, e
    fam, n, tab = h.label_families(par, 1, W, inc, r['nwin'], r['vel'], r['baz'], r['mdccm'])      # covers what the plan refuses
    assert fam.shape == r['vel'].shape and n == len(tab) and n >= 1
    print('FAMILIES_COMM_OK')


if __name__ == '__main__':
    main()
