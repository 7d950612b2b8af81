"""The gate the three route writers share (write_routes in t2d_api.hip behind t2d_curve_routes, t2d_spline_routes and
t2d_planview_routes): which call is refused with which code and which text, and in which order the checks come.  Every refusal is
the host's: nothing is launched, and the installed vertices are the same afterwards.  The texts are those the three entry points
had while each carried its own copy of the checks."""
import numpy as np
import pytest

from route_writers import A, N_ENV, placeholder, route_pool

pytestmark = pytest.mark.gpu
CAP = 40


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _writer(torch, who, pool):
    """call(route, count_ptr, bad): one direct call of the entry point with valid arguments of its family (bad: one invalid one)"""
    from tactics2d_amd import _ffi, layout as L
    from tactics2d_amd.interpolator import pack_planview, pack_words
    lib, h = _ffi.lib(), pool._h
    if who == "t2d_curve_routes":
        words = pack_words(torch.ones((N_ENV, 5), dtype=torch.float64, device="cuda"), torch.ones((N_ENV, 5), dtype=torch.int8, device="cuda"),
                           torch.full((N_ENV,), 3, dtype=torch.int32, device="cuda"))
        starts = torch.zeros((N_ENV, 3), dtype=torch.float64, device="cuda")
        keep = (words, starts)
        call = lambda route=0, cnt=None, bad=False: lib.t2d_curve_routes(h, words.data_ptr(), starts.data_ptr(), 0.0 if bad else 4.0, 0.5,
                                                                         L.CURVE_DUBINS, route, cnt, None)
    elif who == "t2d_spline_routes":
        ctrl = torch.as_tensor(np.cumsum(np.ones((N_ENV, 4, 2)), 1), device="cuda")
        n_ctrl = torch.full((N_ENV,), 4, dtype=torch.int32, device="cuda")
        keep = (ctrl, n_ctrl)
        call = lambda route=0, cnt=None, bad=False: lib.t2d_spline_routes(h, 5 if bad else L.SPLINE_CUBIC, ctrl.data_ptr(), n_ctrl.data_ptr(), 4,
                                                                          10, 0, None, L.SPLINE_NATURAL, None, route, cnt, None)
    else:
        rec, n_geom = pack_planview([[dict(s=0.0, x=0.0, y=0.0, hdg=0.1 * e, length=5.0, line={})] for e in range(N_ENV)])
        rec, n_geom = rec.cuda(), n_geom.cuda()
        keep = (rec, n_geom)
        call = lambda route=0, cnt=None, bad=False: lib.t2d_planview_routes(h, rec.data_ptr(), n_geom.data_ptr(), 1, L.SPIRAL_REFERENCE,
                                                                            0 if bad else 1, route, cnt, None)
    return call, keep


def _refused(pool, rc, code, text):
    from tactics2d_amd import _ffi
    assert rc == code, (rc, code, text)
    with pytest.raises(_ffi.T2DError) as ei:
        _ffi.check(rc, pool._h)
    assert str(ei.value) == f"libt2d_hip error {code}: {text}"


WRITERS = ["t2d_curve_routes", "t2d_spline_routes", "t2d_planview_routes"]


@pytest.mark.parametrize("who", WRITERS)
def test_the_gate_refuses_in_order_and_with_the_texts_of_the_three_copies(torch, who):
    from tactics2d_amd import _ffi
    z = np.zeros(N_ENV * A, np.float32)
    pool = route_pool(z, z, z, z)
    call, keep = _writer(torch, who, pool)
    no_sets = f"{who} writes into route sets: t2d_set_routes must precede it"
    # no routes installed: an invalid argument of the family, and of the gate, wins over the state
    assert call(bad=True) == _ffi.ERR_INVALID
    _refused(pool, call(route=-1), _ffi.ERR_INVALID, f"{who}: route must be >= 0")
    _refused(pool, call(), _ffi.ERR_STATE, no_sets)
    pool.set_routes([[placeholder(CAP, 0)]], None, 0, 1.0)                              # one set shared by every env
    before = pool.route_vertices().cpu().numpy().copy()
    _refused(pool, call(), _ffi.ERR_STATE, f"{who}: two envs share a route set; install one set per env (set_of_env)")
    _refused(pool, call(route=-1), _ffi.ERR_INVALID, f"{who}: route must be >= 0")
    pool.sync()
    assert np.array_equal(pool.route_vertices().cpu().numpy(), before)
    sets = [[placeholder(CAP, e)] + ([placeholder(4, e), placeholder(4, e)] if e != 3 else []) for e in range(N_ENV)]
    pool.set_routes(sets, np.arange(N_ENV), 0, 1.0)                                     # env 3's set has one route, the others three
    before = pool.route_vertices().cpu().numpy().copy()
    for route in (1, 2, 1000):
        _refused(pool, call(route=route), _ffi.ERR_STATE,
                 f"{who}: route {route} does not exist in every env's set (the smallest set has 1 routes)")
    assert call(route=1, bad=True) == _ffi.ERR_INVALID
    pool.sync()
    assert np.array_equal(pool.route_vertices().cpu().numpy(), before)                  # nothing was launched
    assert call() == _ffi.OK                                                            # the arguments were good otherwise
    pool.sync()
    assert not np.array_equal(pool.route_vertices().cpu().numpy(), before)
    pool.clear_routes()
    _refused(pool, call(), _ffi.ERR_STATE, no_sets)
    pool.close()


@pytest.mark.parametrize("who", WRITERS)
def test_a_misaligned_count_is_an_invalid_argument_of_every_writer(torch, who):
    from tactics2d_amd import _ffi
    z = np.zeros(N_ENV * A, np.float32)
    pool = route_pool(z, z, z, z)
    call, keep = _writer(torch, who, pool)
    count = torch.zeros(N_ENV + 1, dtype=torch.int32, device="cuda")
    text = f"{who}: misaligned count_dev"
    _refused(pool, call(cnt=count.data_ptr() + 2), _ffi.ERR_INVALID, text)              # before the state: no routes installed yet
    pool.set_routes([[placeholder(CAP, e)] for e in range(N_ENV)], np.arange(N_ENV), 0, 1.0)
    before = pool.route_vertices().cpu().numpy().copy()
    _refused(pool, call(cnt=count.data_ptr() + 2), _ffi.ERR_INVALID, text)
    pool.sync()
    assert np.array_equal(pool.route_vertices().cpu().numpy(), before) and not count.cpu().numpy().any()   # nothing was launched
    assert call(cnt=count.data_ptr() + 4) == _ffi.OK
    pool.sync()
    assert (count.cpu().numpy()[1:] > 0).all() and count[0].item() == 0
    pool.close()
