"""Worker of tests/test_gpu_subsample.py: a handle with an RCCL communicator (a world of one over the loopback stand-in
named in NBLS_TEST_TRANSPORT) accepts a plan with lag refinement, and the block it gathers is the block of the same
refined pass on a handle without a communicator — the gathered block carries everything the refinement changes.  The
fractions themselves are fetched locally.  A process of its own: a communicator lives as long as its process."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def run(h, data, geometry, refine, reserve):
    h.set_trace(data, 20.0)
    h.set_geometry(*geometry)
    h.reserve_results(reserve)
    h.set_lag_refinement(refine)
    try:
        h.plan(None, False, None, None, [65], [32], 40)
    finally:
        h.set_lag_refinement(False)
    h.execute()
    return h.fetch_packed()


def main():
    import refine_truth as rt
    from narrow_band_least_squares_amd import dist, engine, planner
    dist.set_transport_library(os.environ['NBLS_TEST_TRANSPORT'], allow_shared_device=True)
    h = engine.get_handle(None, 0)
    plain_h = engine.get_handle(None, 1)                   # the same device, no communicator
    uid = (C.c_char * 128)()
    assert h.lib.nbls_comm_unique_id(uid, 128) == 0
    h._chk(h.lib.nbls_comm_init_rank(h._h, bytes(uid), 1, 0))
    data, rij, _ = rt.sinusoid_wave(4, 1201, 20.0, 769, max_delay=16.0, noise=0.05)
    geometry = planner.co_array(rij)
    cells, mb = 40, 1
    total = cells * (32 + mb)
    block_bytes = (total + 8 + 7) // 8 * 8
    mine = run(h, data, geometry, True, block_bytes)
    frac = h.fetch_lag_fraction()
    assert np.count_nonzero(frac) > frac.size // 4
    hs = (C.c_void_p * 1)(h._h)
    out = np.empty((1, block_bytes), dtype=np.uint8)
    h._chk(h.lib.nbls_comm_gather(hs, 1, 0, block_bytes, 0, out.ctypes.data, out.nbytes))
    assert int(out[0, -8:].view(np.int64)[0]) == 0
    grids = out[0, :32 * cells].view(np.float64).reshape(4, 1, cells)
    mask = out[0, 32 * cells:total].reshape(1, cells, mb)
    ref = run(plain_h, data, geometry, True, 0)
    np.testing.assert_array_equal(plain_h.fetch_lag_fraction(), frac)
    for i, k in enumerate(('vel', 'baz', 'mdccm', 'sigma_tau')):
        np.testing.assert_array_equal(grids[i], ref[k], err_msg=k)
        np.testing.assert_array_equal(mine[k], ref[k], err_msg=k)
    np.testing.assert_array_equal(mask, ref['mask'])
    unrefined = run(plain_h, data, geometry, False, 0)
    np.testing.assert_array_equal(unrefined['mdccm'], ref['mdccm'])
    assert not np.array_equal(unrefined['sigma_tau'], ref['sigma_tau'])
    print('SUBSAMPLE_COMM_OK')


if __name__ == '__main__':
    main()
