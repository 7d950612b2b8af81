"""t2d_grid_dijkstra on the device: EVERY case of the fixture made by running the reference's Dijkstra
(tests/golden/grid_search.npz) as ragged batches, field, status, path length and path BIT-EQUAL to the specification
(tests/grid_search_ref.py) and the world-coordinate paths equal to the reference's recorded arrays; the same cases in reversed
order in wider rows (the other kernel form) with identical results; truncated, invalid and field-only rows beside good ones, in
sentinel-filled buffers with a guard region; a grid at the cap and one a cell over it; device tensors in and out; and
Dijkstra.plan against the recorded arrays."""
import numpy as np
import pytest

import grid_search_ref as R
from test_grid_search import fixture, fixture_case, n_cases, spec_case

pytestmark = pytest.mark.gpu
SENTINEL, PAD = -12345.0, 7.0e30   # outputs start as SENTINEL; PAD fills the weights no kernel may read
GUARD = 64


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _raw(torch, grids, sources, targets, stride, conn, mult, max_path, hw=None):
    """t2d_grid_dijkstra through the C interface into sentinel-filled buffers with a guard region behind them ->
    (rc, g [n, stride], path [n, max_path], path_len, status, sweeps [n]); the guards are checked here"""
    from tactics2d_amd import _ffi
    n = len(grids)
    w = np.full((n, stride), PAD)
    for k, gr in enumerate(grids):
        w[k, :gr.size] = gr.reshape(-1)
    hw = np.int32([gr.shape for gr in grids]) if hw is None else np.int32(hw)
    t = lambda v, dt: torch.as_tensor(np.ascontiguousarray(v, dt), device="cuda")
    w_d, hw_d, s_d, t_d = t(w, np.float64), t(hw, np.int32), t(sources, np.int32), t(targets, np.int32)
    g = torch.full((n * stride + GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
    path = torch.full((n * max_path + GUARD,), -7, dtype=torch.int32, device="cuda")
    small = [torch.full((n + GUARD,), -7, dtype=torch.int32, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    rc = _ffi.lib().t2d_grid_dijkstra(0, n, w_d.data_ptr(), hw_d.data_ptr(), s_d.data_ptr(), t_d.data_ptr(), stride, conn, mult, max_path,
                                      g.data_ptr(), path.data_ptr(), *(x.data_ptr() for x in small), None)
    torch.cuda.synchronize()
    g, path = g.cpu().numpy(), path.cpu().numpy()
    small = [x.cpu().numpy() for x in small]
    assert (g[n * stride:] == SENTINEL).all() and (path[n * max_path:] == -7).all() and all((x[n:] == -7).all() for x in small)
    return (rc, g[:n * stride].reshape(n, stride), path[:n * max_path].reshape(n, max_path)) + tuple(x[:n] for x in small)


def _same(got, want, cells, what):
    """one row of _raw against a specification dict; the field's entries past the grid are untouched"""
    g, path, path_len, status, sweeps = got
    assert status == want["status"], (what, status, want["status"])
    assert g[:cells].tobytes() == want["g"].tobytes(), what
    assert (g[cells:] == SENTINEL).all(), what
    m = min(len(path), len(want["path"]))   # (the specification's row is as long as the grid unless it was given max_path)
    assert path_len == want["path_len"] and (path[:m] == want["path"][:m]).all(), what
    assert (path[m:] == -1).all() and (want["path"][m:] == -1).all(), what
    assert (sweeps == 0) == (status == R.INVALID) and sweeps <= cells, (what, sweeps)


def _groups():
    g = fixture()
    out = {}
    for k in range(n_cases()):
        out.setdefault((int(g["connectivity"][k]), float(g["mult"][k])), []).append(k)
    return out


@pytest.fixture(scope="module")
def forward(torch):
    """every fixture case, one launch per (connectivity, multiplier), rows as wide as the largest grid -> {case: row of _raw}"""
    rows = {}
    for (conn, mult), ks in _groups().items():
        cases = [fixture_case(k) for k in ks]
        stride = max(c[0].size for c in cases)
        rc, *out = _raw(torch, [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], stride, conn, mult, stride)
        assert rc == 0
        for i, k in enumerate(ks):
            rows[k] = tuple(o[i] for o in out)
    return rows


def test_the_whole_fixture_is_bit_equal_to_the_specification_and_the_reference(forward):
    from tactics2d_amd import search
    found = 0
    for k in range(n_cases()):
        grid, s, t, conn, mult, want, cost, plan, boundary, res = fixture_case(k)
        name = fixture()["name"][k]
        _same(forward[k], spec_case(k), grid.size, name)
        g, path, path_len, status, _ = forward[k]
        assert g[t] == cost and path_len == len(want) and (path[:path_len] == want).all(), name
        if plan is not None:
            xy = search.world_path(path[:path_len], grid.shape[1], boundary, res)
            assert xy.dtype == plan.dtype and (xy == plan).all(), name
            found += 1
    assert found > 150


def test_reversed_order_and_wider_rows_change_no_row(torch, forward):
    """rows 2048 wide take the 1024-lane form of the kernel, the fixture's own rows the 256-lane one"""
    for (conn, mult), ks in _groups().items():
        ks = ks[::-1]
        cases = [fixture_case(k) for k in ks]
        rc, *out = _raw(torch, [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], 2048, conn, mult, 600)
        assert rc == 0
        for i, k in enumerate(ks):
            g, path, path_len, status, sweeps = (o[i] for o in out)
            fg, fpath, fpath_len, fstatus, fsweeps = forward[k]
            cells = cases[i][0].size
            assert g[:cells].tobytes() == fg[:cells].tobytes() and (g[cells:] == SENTINEL).all(), fixture()["name"][k]
            assert (status, path_len, sweeps) == (fstatus, fpath_len, fsweeps), fixture()["name"][k]
            m = min(len(path), len(fpath))
            assert (path[:m] == fpath[:m]).all() and (path[m:] == -1).all() and (fpath[m:] == -1).all(), fixture()["name"][k]


def test_truncated_invalid_and_field_only_rows_sit_beside_good_ones(torch):
    g = fixture()
    long_k = int(np.argmax(g["index_len"]))
    conn, mult = int(g["connectivity"][long_k]), float(g["mult"][long_k])
    same = [k for k in _groups()[(conn, mult)] if g["index_len"][k] > 0]
    short_k = next(k for k in same if 2 <= g["index_len"][k] <= 7)
    mid_k = next(k for k in same if 8 <= g["index_len"][k] <= 40)
    L, S, M = fixture_case(long_k), fixture_case(short_k), fixture_case(mid_k)
    negative = M[0].copy()
    negative.reshape(-1)[M[2]] = -1.0
    wall = int(np.flatnonzero(np.isinf(L[0].reshape(-1)))[0])
    #        grid      source  target       what
    rows = [(S[0], S[1], S[2]),           # found
            (L[0], L[1], L[2]),           # truncated
            (M[0], M[1], -1),             # field only
            (negative, M[1], M[2]),       # a negative weight
            (M[0], M[1], M[2]),           # truncated
            (L[0], wall, L[2]),           # the source is an obstacle
            (L[0], L[1], wall),           # the target is an obstacle
            (M[0], -1, M[2]),             # the source is out of range
            (M[0], M[1], M[0].size),      # the target is out of range
            (M[0], M[1], -2),
            (S[0], S[1], S[1]),           # source == target: one cell
            (S[0], S[1], S[2])]           # found again
    max_path, stride = 7, L[0].size
    rc, *out = _raw(torch, [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], stride, conn, mult, max_path)
    assert rc == 0
    want_status = [R.FOUND, R.TRUNCATED, R.FIELD_ONLY, R.INVALID, R.TRUNCATED, R.INVALID, R.INVALID, R.INVALID, R.INVALID, R.INVALID,
                   R.FOUND, R.FOUND]
    for i, (grid, s, t) in enumerate(rows):
        want = R.solve(grid, s, t, conn, mult, max_path=max_path)
        assert want["status"] == want_status[i], i
        _same(tuple(o[i] for o in out), want, grid.size, i)
    assert (out[1][0] == out[1][11]).all() and out[0][0].tobytes() == out[0][11].tobytes()
    # a shape that is not one: nothing of the row's field is written, the neighbours are as before
    hw = [r[0].shape for r in rows]
    hw[3], hw[5], hw[7] = (0, 5), (-3, 4), (stride, 2)
    rc, *bad = _raw(torch, [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], stride, conn, mult, max_path, hw=hw)
    assert rc == 0
    for i in range(len(rows)):
        if i in (3, 5, 7):
            assert (bad[0][i] == SENTINEL).all() and (bad[1][i] == -1).all() and (bad[2][i], bad[3][i], bad[4][i]) == (0, R.INVALID, 0)
        else:
            assert all(b[i].tobytes() == o[i].tobytes() for b, o in zip(bad, out)), i


def test_a_grid_at_the_cap_and_one_cell_over_it(torch):
    from tactics2d_amd import _ffi, layout as L, search
    side = 64
    assert side * side == L.GRID_MAX_CELLS
    rng = np.random.RandomState(3)
    busy = rng.randint(1, 6, size=(side, side)).astype(float)
    busy[rng.rand(side, side) < 0.3] = np.inf
    busy[0, 0] = busy[side - 1, side - 1] = 1.0
    corridor = np.ones((side, side))   # a serpentine: about half the cap's cells on the path, as many rounds
    for r in range(1, side, 2):
        corridor[r, :] = np.inf
        corridor[r, side - 1 if (r // 2) % 2 == 0 else 0] = 1.0
    last = side * side - 1
    rc, *out = _raw(torch, [busy, corridor], [0, 0], [last, (side - 2) * side], side * side, 8, 1.4142135623730951, side * side)
    assert rc == 0
    for i, (grid, t) in enumerate(((busy, last), (corridor, (side - 2) * side))):
        want = R.solve(grid, 0, t, 8, 1.4142135623730951)
        _same(tuple(o[i] for o in out), want, grid.size, i)
    assert out[3][1] == R.FOUND and out[2][1] > side * side // 4
    print(f"sweeps at the cap: 30 % obstacles {out[4][0]}, serpentine {out[4][1]}")
    # one cell over: refused by name, nothing launched
    over = np.ones((1, side, side + 1))
    with pytest.raises(_ffi.GeometryError) as ei:
        search.plan_batch(over, [0], [5])
    assert ei.value.code == _ffi.ERR_GEOMETRY and "T2D_GRID_MAX_CELLS" in str(ei.value) and str(L.GRID_MAX_CELLS) in str(ei.value)
    status = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    w = torch.ones(side * (side + 1), dtype=torch.float64, device="cuda")
    z = torch.zeros(2, dtype=torch.int32, device="cuda")
    rc = _ffi.lib().t2d_grid_dijkstra(0, 1, w.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), side * (side + 1), 4, 1.0, 0,
                                      w.data_ptr(), None, status.data_ptr(), status.data_ptr(), status.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == _ffi.ERR_GEOMETRY and int(status[0]) == -7


def test_tensors_in_and_out_stay_on_the_device(torch):
    from tactics2d_amd import search
    ks = [k for k in _groups()[(8, 1.4142135623730951)] if tuple(fixture()["hw"][k]) == (16, 16)]
    cases = [fixture_case(k) for k in ks]
    weights = torch.as_tensor(np.stack([c[0] for c in cases]), device="cuda")
    sources = torch.as_tensor(np.int32([c[1] for c in cases]), device="cuda")
    targets = torch.as_tensor(np.int32([c[2] for c in cases]), device="cuda")
    out = search.Dijkstra.plan_batch(weights, sources, targets, connectivity=8)
    assert out._inputs[0].data_ptr() == weights.data_ptr() and out._inputs[1].data_ptr() == sources.data_ptr()
    assert out._inputs[2].data_ptr() == targets.data_ptr()
    for x, dt in ((out.field, torch.float64), (out.path, torch.int32), (out.path_len, torch.int32), (out.status, torch.int32)):
        assert x.is_cuda and x.dtype == dt
    assert out.field.shape == (len(ks), 16, 16) and out.path.shape == (len(ks), 256)
    field = search.cost_to_go(weights, sources, connectivity=8)
    assert field.is_cuda and field.shape == (len(ks), 16, 16)
    for i, k in enumerate(ks):
        want = spec_case(k)
        assert out.flat_field()[i].cpu().numpy().tobytes() == want["g"].tobytes() == field[i].reshape(-1).cpu().numpy().tobytes()
        assert int(out.status[i]) == want["status"] and int(out.path_len[i]) == want["path_len"]
        assert (out.path[i].cpu().numpy() == want["path"]).all()
    # (row, col) pairs from the host generator's batch
    pairs = search.plan_batch(np.stack([c[0] for c in cases]), np.int32([divmod(c[1], 16) for c in cases]),
                              np.int32([divmod(c[2], 16) for c in cases]), connectivity=8)
    assert (pairs.path.cpu().numpy() == out.path.cpu().numpy()).all()


def test_plan_returns_the_reference_arrays():
    from tactics2d_amd.search import Dijkstra
    g = fixture()
    picks = [int(np.argmax(g["index_len"]))] + [int(k) for k in np.flatnonzero(g["index_len"] == 0)[:2]] + \
            [int(k) for k in np.flatnonzero((g["connectivity"] == 8) & (g["index_len"] > 5))[:3]]
    for k in picks:
        grid, s, t, conn, mult, want, cost, plan, boundary, res = fixture_case(k)
        w = grid.shape[1]
        xy = Dijkstra.plan([s % w * res + boundary[0], s // w * res + boundary[2]], [t % w * res + boundary[0], t // w * res + boundary[2]],
                           boundary, grid, res, connectivity=conn, diagonal_cost_multiplier=mult)
        if plan is None:
            assert xy is None, g["name"][k]
        else:
            assert xy.dtype == plan.dtype and xy.shape == plan.shape and (xy == plan).all(), g["name"][k]
