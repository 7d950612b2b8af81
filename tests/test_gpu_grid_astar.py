"""t2d_grid_astar on the device: EVERY run of the fixture made by running the reference's AStar (tests/golden/grid_astar.npz) as
ragged batches grouped by the launch's scalars, every output BIT-EQUAL to the specification (tests/astar_ref.py), in sentinel-filled
buffers with guard regions and a pattern-filled workspace; the same runs in reversed order; one query at both ends of a 130-row
batch and alone; invalid, truncated, max_iter and no-path rows beside good ones; NULL optional outputs; device tensors on a side
stream; two launches; AStar.plan and plan_graph against the recorded arrays, a Python callable through the table included; a fresh
random batch; and occupancy_grid -> AStar.plan_batch -> polyline_routes on a generated parking pool."""
import numpy as np
import pytest

import astar_ref as A
from test_grid_astar import fixture, grid_of, n_runs, recorded, run_inputs, run_name, spec_run

pytestmark = pytest.mark.gpu
SENTINEL, PAD = -12345.0, 7.0e30   # outputs start as SENTINEL; PAD fills the weights and table entries no kernel may read
GUARD = 64
SQRT2 = 1.4142135623730951
OUTPUTS = ("path", "path_len", "path_xy", "status", "iterations", "expanded", "g", "closed", "parent")


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _raw(torch, rows, stride, conn, mult, kind, scale, max_iter, max_path, cell_size=1.0, origin=(0.0, 0.0), hw=None, skip=()):
    """t2d_grid_astar through the C interface: rows of dict(weight, source, target, htarget, table) into sentinel-filled buffers
    with a guard region behind each and a workspace filled with a pattern -> (rc, {name: array with one row per query}); the
    guards are checked here.  skip: the optional outputs passed as NULL."""
    from tactics2d_amd import _ffi
    n = len(rows)
    w, tab = np.full((n, stride), PAD), np.full((n, stride), PAD)
    for k, r in enumerate(rows):
        w[k, :r["weight"].size] = r["weight"].reshape(-1)
        if kind == A.H_TABLE:
            tab[k, :r["weight"].size] = np.asarray(r["table"]).reshape(-1)
    hw = np.int32([r["weight"].shape for r in rows]) if hw is None else np.int32(hw)
    point = np.float64([r["htarget"] if r.get("htarget") is not None else (r["target"] % s[1], r["target"] // s[1])
                        for r, s in zip(rows, [r["weight"].shape for r in rows])])
    t = lambda v, dt: torch.as_tensor(np.ascontiguousarray(v, dt), device="cuda")
    w_d, hw_d, p_d, tab_d = t(w, np.float64), t(hw, np.int32), t(point, np.float64), t(tab, np.float64)
    s_d, t_d = t([r["source"] for r in rows], np.int32), t([r["target"] for r in rows], np.int32)
    lib = _ffi.lib()
    need = lib.t2d_grid_astar_workspace_bytes(n, stride, conn)
    assert need > 0
    ws = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    shapes = dict(path=(max_path,), path_xy=(max_path, 2), g=(stride,), closed=(stride,), parent=(stride,))
    kinds = dict(path_xy=torch.float64, g=torch.float64, closed=torch.uint8)
    fill = lambda dt: SENTINEL if dt == torch.float64 else (0xEE if dt == torch.uint8 else -7)
    bufs = {}
    for name in OUTPUTS:
        dt = kinds.get(name, torch.int32)
        bufs[name] = torch.full((n * int(np.prod(shapes.get(name, (1,)))) + GUARD,), fill(dt), dtype=dt, device="cuda")
    ptr = lambda name: None if name in skip else bufs[name].data_ptr()
    torch.cuda.synchronize()
    rc = lib.t2d_grid_astar(0, n, w_d.data_ptr(), hw_d.data_ptr(), s_d.data_ptr(), t_d.data_ptr(), stride, conn, mult, kind,
                            p_d.data_ptr(), tab_d.data_ptr() if kind == A.H_TABLE else None, scale, max_iter, max_path, cell_size,
                            origin[0], origin[1], ws.data_ptr(), need, ptr("path"), ptr("path_len"), ptr("path_xy"), ptr("status"),
                            ptr("iterations"), ptr("expanded"), ptr("g"), ptr("closed"), ptr("parent"), None)
    torch.cuda.synchronize()
    assert (ws[need:].cpu().numpy() == 0xA5).all()
    out = {}
    for name in OUTPUTS:
        a = bufs[name].cpu().numpy()
        size = n * int(np.prod(shapes.get(name, (1,))))
        assert (a[size:] == fill(bufs[name].dtype)).all(), name
        if name in skip:
            assert (a == fill(bufs[name].dtype)).all(), name
        out[name] = a[:size].reshape((n,) + shapes.get(name, ()))
    return rc, out


def _same(out, i, want, cells, what, skip=()):
    """row i of _raw against a specification dict, bit for bit; entries past the grid are untouched"""
    for name in ("status", "path_len", "iterations", "expanded"):
        assert out[name][i] == want[name], (what, name, out[name][i], want[name])
    m = min(out["path"].shape[1], len(want["path"]))   # (the specification's row is as long as the grid unless it was given max_path)
    assert (out["path"][i, :m] == want["path"][:m]).all() and (out["path"][i, m:] == -1).all() and (want["path"][m:] == -1).all(), what
    if "path_xy" not in skip:
        assert out["path_xy"][i, :m].tobytes() == want["path_xy"][:m].tobytes() and np.isnan(out["path_xy"][i, m:]).all(), what
    for name, fill in (("g", SENTINEL), ("closed", 0xEE), ("parent", -7)):
        if name not in skip:
            assert out[name][i, :cells].tobytes() == want[name].tobytes(), (what, name)
            assert (out[name][i, cells:] == fill).all(), (what, name)


def _groups():
    """the fixture's runs by the scalars of a launch: (connectivity, mult, kind, scale, max_iter) -> [run]"""
    out = {}
    for r in range(n_runs()):
        a = run_inputs(r)
        out.setdefault((a["connectivity"], a["mult"], a["kind"], a["scale"], a["max_iter"]), []).append(r)
    return out


def _launch(torch, runs, key, max_path=None, stride=None):
    rows = [run_inputs(r) for r in runs]
    stride = max(a["weight"].size for a in rows) if stride is None else stride
    rc, out = _raw(torch, rows, stride, *key, stride if max_path is None else max_path)
    assert rc == 0
    return out, stride


@pytest.fixture(scope="module")
def forward(torch):
    """every fixture run, one launch per group -> {run: (outputs of its launch, row)}"""
    rows = {}
    for key, runs in _groups().items():
        out, _ = _launch(torch, runs, key)
        for i, r in enumerate(runs):
            rows[r] = (out, i)
    return rows


def test_the_whole_fixture_is_bit_equal_to_the_specification_and_the_reference(forward):
    g = fixture()
    found = 0
    for r in range(n_runs()):
        out, i = forward[r]
        want, rec = spec_run(r)[0], recorded(r)
        cells = run_inputs(r)["weight"].size
        _same(out, i, want, cells, run_name(r))
        # ... and the reference itself: iterations, closed set, came_from, g_score
        assert out["iterations"][i] == rec["iteration"] and (out["closed"][i, :cells] == rec["closed"]).all(), run_name(r)
        assert (out["parent"][i, :cells] == rec["parent"]).all() and out["g"][i, :cells].tobytes() == rec["g"].tobytes(), run_name(r)
        assert (out["status"][i] == A.FOUND) == bool(rec["found"]), run_name(r)
        if rec["found"] and g["mode"][r] == 0:
            assert (out["path"][i, :out["path_len"][i]] == rec["path"]).all(), run_name(r)
            found += 1
    assert found > 250


def test_reversed_order_and_wider_rows_change_no_row(torch, forward):
    for key, runs in _groups().items():
        runs = runs[::-1]
        widest = max(run_inputs(r)["weight"].size for r in runs)
        out, stride = _launch(torch, runs, key, max_path=widest, stride=min(widest + 37, 4096))
        for i, r in enumerate(runs):
            fwd, j = forward[r]
            cells = run_inputs(r)["weight"].size
            for name in OUTPUTS:
                a, b = out[name][i], fwd[name][j]
                if name in ("g", "closed", "parent"):
                    a, b = a[:cells], b[:cells]
                elif name in ("path", "path_xy"):
                    m = min(len(a), len(b))
                    a, b = a[:m], b[:m]
                assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), (run_name(r), name)


def test_one_query_at_both_ends_of_130_rows_and_alone(torch):
    g = fixture()
    pick = next(r for r in range(n_runs()) if g["mode"][r] == 0 and g["kind"][r] == A.H_EUCLIDEAN and g["max_iter"][r] == 100000
                and g["scale"][r] == 1.0 and g["grid_connectivity"][g["grid_id"][r]] == 8 and spec_run(r)[1]["stale_at"]
                and 100 < run_inputs(r)["weight"].size <= 600)
    a = run_inputs(pick)
    same = [r for r in _groups()[(8, a["mult"], A.H_EUCLIDEAN, 1.0, 100000)] if run_inputs(r)["weight"].size <= 600]
    filler = (same * 3)[:128]
    key = (8, a["mult"], A.H_EUCLIDEAN, 1.0, 100000)
    out, _ = _launch(torch, [pick] + filler + [pick], key, stride=600)
    alone, _ = _launch(torch, [pick], key, stride=600)
    cells = a["weight"].size
    for i in (0, 129):
        _same(out, i, spec_run(pick)[0], cells, i)
        for name in OUTPUTS:
            assert out[name][i].tobytes() == alone[name][0].tobytes(), (i, name)
    for i, r in enumerate(filler):
        _same(out, i + 1, spec_run(r)[0], run_inputs(r)["weight"].size, run_name(r))


def _row(grid, s, t, htarget=None, table=None):
    return dict(weight=grid, source=s, target=t, htarget=htarget, table=table)


def test_invalid_truncated_max_iter_and_no_path_rows_sit_beside_good_ones(torch):
    g = fixture()
    names = list(g["grid_name"])
    kL, kW, kM = names.index("serpentine_24x24_8"), names.index("walled_in_8"), names.index("decimal_weights_0_8")
    gl, gw, gm = grid_of(kL), grid_of(kW), grid_of(kM)
    cell = lambda k, what: int(g[what][k][0] * g["grid_hw"][k][1] + g[what][k][1])
    sL, tL, sW, tW, sM, tM = cell(kL, "grid_start"), cell(kL, "grid_goal"), cell(kW, "grid_start"), cell(kW, "grid_goal"), \
        cell(kM, "grid_start"), cell(kM, "grid_goal")
    negative = gm.copy()
    negative.reshape(-1)[tM] = -1.0
    wall = int(np.flatnonzero(np.isinf(gl.reshape(-1)))[0])
    nan, inf = float("nan"), float("inf")
    rows = [_row(gm, sM, tM),                          # found
            _row(gl, sL, tL),                          # truncated: 7 cells of a long corridor
            _row(gw, sW, tW),                          # no path: the target is walled in
            _row(negative, sM, tM),                    # a negative weight
            _row(gl, wall, tL),                        # the source is an obstacle
            _row(gl, sL, wall),                        # the target is an obstacle
            _row(gm, -1, tM),                          # out of range
            _row(gm, sM, gm.size),
            _row(gm, sM, -1),                          # (no field-only call)
            _row(gm, sM, tM, htarget=(nan, 2.0)),      # htarget is not finite
            _row(gm, sM, tM, htarget=(1.0, -inf)),
            _row(gm, sM, sM),                          # source == target: one cell, found by the first pop
            _row(gm, sM, tM, htarget=(3.25, -1.5)),    # a point that is no cell: found
            _row(gm, sM, tM)]                          # found again
    status = [A.FOUND, A.TRUNCATED, A.NO_PATH] + [A.INVALID] * 8 + [A.FOUND, A.FOUND, A.FOUND]
    max_path, stride = 21, gl.size
    rc, out = _raw(torch, rows, stride, 8, SQRT2, A.H_EUCLIDEAN, 1.0, 100000, max_path, 0.5, (-3.0, 7.25))
    assert rc == 0
    for i, r in enumerate(rows):
        want = A.solve(r["weight"], r["source"], r["target"], A.H_EUCLIDEAN, r["htarget"], None, 1.0, 8, SQRT2, 100000, max_path, 0.5,
                       (-3.0, 7.25))
        assert want["status"] == status[i], i
        _same(out, i, want, r["weight"].size, i)
    assert out["path_len"][1] > max_path and out["path_len"][11] == 1 and out["iterations"][11] == 0 and out["expanded"][11] == 1
    for name in OUTPUTS:
        assert out[name][0].tobytes() == out[name][13].tobytes(), name
    # max_iter: the same rows stopped after 5 iterations; the short ones still find their target
    rc, lim = _raw(torch, rows, stride, 8, SQRT2, A.H_EUCLIDEAN, 1.0, 5, max_path, 0.5, (-3.0, 7.25))
    assert rc == 0
    for i, r in enumerate(rows):
        want = A.solve(r["weight"], r["source"], r["target"], A.H_EUCLIDEAN, r["htarget"], None, 1.0, 8, SQRT2, 5, max_path, 0.5, (-3.0, 7.25))
        _same(lim, i, want, r["weight"].size, i)
    assert list(lim["status"][:3]) == [A.MAX_ITER] * 3 and lim["status"][11] == A.FOUND and (lim["iterations"][:3] == 5).all()
    # a shape that is not one: nothing of the row's state is written, the neighbours are as before
    hw = [r["weight"].shape for r in rows]
    hw[3], hw[5], hw[7] = (0, 5), (-3, 4), (stride, 2)
    rc, bad = _raw(torch, rows, stride, 8, SQRT2, A.H_EUCLIDEAN, 1.0, 100000, max_path, 0.5, (-3.0, 7.25), hw=hw)
    assert rc == 0
    for i in range(len(rows)):
        if i in (3, 5, 7):
            assert (bad["g"][i] == SENTINEL).all() and (bad["closed"][i] == 0xEE).all() and (bad["parent"][i] == -7).all()
            assert (bad["path"][i] == -1).all() and np.isnan(bad["path_xy"][i]).all()
            assert (bad["path_len"][i], bad["status"][i], bad["iterations"][i], bad["expanded"][i]) == (0, A.INVALID, 0, 0)
        else:
            assert all(bad[name][i].tobytes() == out[name][i].tobytes() for name in OUTPUTS), i
    # a scale that is negative or not finite: every row; a table entry that is NaN or -inf, or 0 * inf: its row
    for scale in (-1.0, nan, inf):
        rc, o = _raw(torch, rows[:2], stride, 8, SQRT2, A.H_EUCLIDEAN, scale, 100000, max_path)
        assert rc == 0 and list(o["status"]) == [A.INVALID] * 2 and not o["closed"][0, :gm.size].any()
    base = np.array([A.heuristic(A.H_EUCLIDEAN, v % gm.shape[1], v // gm.shape[1], tM % gm.shape[1], tM // gm.shape[1]) for v in range(gm.size)])
    tables = [base.copy() for _ in range(5)]
    tables[1][7], tables[2][gm.size - 1], tables[3][5] = nan, -inf, inf
    trows = [_row(gm, sM, tM, table=tb) for tb in tables]
    for scale, status in ((1.0, [A.FOUND, A.INVALID, A.INVALID, A.FOUND, A.FOUND]), (0.0, [A.FOUND, A.INVALID, A.INVALID, A.INVALID, A.FOUND])):
        rc, o = _raw(torch, trows, gm.size, 8, SQRT2, A.H_TABLE, scale, 100000, gm.size)
        assert rc == 0 and list(o["status"]) == status, scale
        for i, r in enumerate(trows):
            _same(o, i, A.solve(gm, sM, tM, A.H_TABLE, None, r["table"], scale, 8, SQRT2), gm.size, (scale, i))


def test_null_optional_outputs_and_refused_calls(torch):
    from tactics2d_amd import _ffi, layout as L, search
    runs = _groups()[(4, SQRT2, A.H_MANHATTAN, 1.0, 100000)][:6]
    key = (4, SQRT2, A.H_MANHATTAN, 1.0, 100000)
    rows = [run_inputs(r) for r in runs]
    stride = max(a["weight"].size for a in rows)
    for skip in (("path_xy", "g", "closed", "parent"), ("g",), ("closed", "parent"), ("path_xy",)):
        rc, out = _raw(torch, rows, stride, *key, stride, skip=skip)
        assert rc == 0
        for i, r in enumerate(runs):
            _same(out, i, spec_run(r)[0], rows[i]["weight"].size, (skip, run_name(r)), skip=skip)
    # nothing is launched and an error code comes back
    for bad in (dict(conn=6), dict(mult=-1.0), dict(mult=float("nan")), dict(kind=5), dict(kind=-1), dict(max_path=-1), dict(cell_size=0.0),
                dict(cell_size=float("inf")), dict(origin=(float("nan"), 0.0))):
        a = dict(conn=4, mult=SQRT2, kind=A.H_MANHATTAN, max_path=stride, cell_size=1.0, origin=(0.0, 0.0))
        a.update(bad)
        lib = _ffi.lib()
        w = torch.ones(stride, dtype=torch.float64, device="cuda")
        z = torch.zeros(4, dtype=torch.int32, device="cuda")
        status = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
        rc = lib.t2d_grid_astar(0, 1, w.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), stride, a["conn"], a["mult"], a["kind"],
                                w.data_ptr(), w.data_ptr(), 1.0, 10, a["max_path"], a["cell_size"], a["origin"][0], a["origin"][1],
                                ws.data_ptr(), 1 << 20, z.data_ptr(), z.data_ptr(), None, status.data_ptr(), z.data_ptr(), z.data_ptr(),
                                None, None, None, None)
        torch.cuda.synchronize()
        assert rc == _ffi.ERR_INVALID and int(status[0]) == -7, bad
    with pytest.raises(_ffi.GeometryError) as ei:
        search.AStar.plan_batch(np.ones((1, 64, 65)), [0], [5])
    assert ei.value.code == _ffi.ERR_GEOMETRY and "T2D_GRID_MAX_CELLS" in str(ei.value) and str(L.GRID_MAX_CELLS) in str(ei.value)
    for kw in (dict(heuristic="nearest"), dict(heuristic="table"), dict(heuristic_table=np.ones((1, 4, 4))), dict(connectivity=5),
               dict(cell_size=-1.0), dict(max_path=-2)):
        with pytest.raises(ValueError):
            search.AStar.plan_batch(np.ones((1, 4, 4)), [0], [5], **kw)


def test_tensors_in_and_out_on_a_side_stream_and_two_launches_are_identical(torch):
    from tactics2d_amd import search
    g = fixture()
    ks = [k for k in range(len(g["grid_name"])) if tuple(g["grid_hw"][k]) == (16, 16) and g["grid_connectivity"][k] == 8]
    assert len(ks) >= 4
    grids = np.stack([grid_of(k) for k in ks])
    src = np.int32([g["grid_start"][k][0] * 16 + g["grid_start"][k][1] for k in ks])
    tgt = np.int32([g["grid_goal"][k][0] * 16 + g["grid_goal"][k][1] for k in ks])
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        weights, sources, targets = (torch.as_tensor(v, device="cuda") for v in (grids, src, tgt))
        points = torch.as_tensor(np.float64([[t % 16 + 0.25, t // 16 - 0.4] for t in tgt]), device="cuda")
    outs = [search.AStar.plan_batch(weights, sources, targets, "euclidean", points, heuristic_scale=2.5, connectivity=8, cell_size=0.5,
                                    origin=(10.0, -4.0), want_state=True, stream=side) for _ in range(2)]
    side.synchronize()
    first, again = outs
    assert first._inputs[0].data_ptr() == weights.data_ptr() and first._inputs[1].data_ptr() == sources.data_ptr()
    assert first._inputs[3].data_ptr() == points.data_ptr()
    for x, dt, shape in ((first.path, torch.int32, (len(ks), 256)), (first.path_xy, torch.float64, (len(ks), 256, 2)),
                         (first.path_len, torch.int32, (len(ks),)), (first.status, torch.int32, (len(ks),)),
                         (first.iterations, torch.int32, (len(ks),)), (first.expanded, torch.int32, (len(ks),)),
                         (first.g, torch.float64, (len(ks), 256)), (first.closed, torch.uint8, (len(ks), 256)),
                         (first.parent, torch.int32, (len(ks), 256))):
        assert x.is_cuda and x.dtype == dt and tuple(x.shape) == shape
    names = ("path", "path_xy", "path_len", "status", "iterations", "expanded", "g", "closed", "parent")
    for name in names:
        assert getattr(first, name).cpu().numpy().tobytes() == getattr(again, name).cpu().numpy().tobytes(), name
    for i in range(len(ks)):
        want = A.solve(grids[i], int(src[i]), int(tgt[i]), A.H_EUCLIDEAN, tuple(points[i].cpu().tolist()), None, 2.5, 8, SQRT2, 100000,
                       256, 0.5, (10.0, -4.0))
        for name in names:
            got = getattr(first, name)[i].cpu().numpy()
            assert np.asarray(want[name], got.dtype).tobytes() == got.tobytes(), (i, name)
    # the defaults: the target cell's own (col, row), no state; (row, col) pairs from the host
    plain = search.astar_plan_batch(grids, np.int32([divmod(int(s), 16) for s in src]), np.int32([divmod(int(t), 16) for t in tgt]), connectivity=8)
    assert plain.g is None and plain.closed is None and plain.parent is None
    for i in range(len(ks)):
        want = A.solve(grids[i], int(src[i]), int(tgt[i]), connectivity=8)
        assert int(plain.status[i]) == want["status"] and (plain.path[i].cpu().numpy() == want["path"]).all()
        assert int(plain.iterations[i]) == want["iterations"]


def test_plan_and_plan_graph_return_the_reference_arrays():
    from tactics2d_amd import search
    g = fixture()
    markers = {A.H_ZERO: search.zero_heuristic, A.H_EUCLIDEAN: search.euclidean_heuristic, A.H_MANHATTAN: search.manhattan_heuristic,
               A.H_OCTILE: search.octile_heuristic}
    plain = (g["scale"] == 1.0) & (g["table_id"] < 0) & (g["grid_hw"][g["grid_id"]].prod(axis=1) <= 600)
    off = np.abs(g["htarget"] - np.round(g["htarget"])).max(axis=1) > 0.1
    picks = list(np.flatnonzero(plain & (g["mode"] == 1) & (g["fn"] == 1))[:3])            # an arbitrary callable: the table path
    picks += list(np.flatnonzero(plain & (g["mode"] == 1) & (g["fn"] == 0) & off)[:4])       # markers against a point that is no cell
    picks += list(np.flatnonzero(plain & (g["mode"] == 1) & (g["found"] == 0) & (g["max_iter"] == 100000))[:1])
    picks += list(np.flatnonzero(plain & (g["mode"] == 1) & (g["max_iter"] < 100000) & (g["max_iter"] > 1))[:3])
    for r in picks:
        k, rec = int(g["grid_id"][r]), recorded(r)
        fn = A.wavy if g["fn"][r] else markers[int(g["kind"][r])]
        xy = search.AStar.plan(list(g["start_xy"][r]), list(g["target_xy"][r]), list(g["grid_boundary"][k]), grid_of(k), fn,
                               float(g["grid_resolution"][k]), int(g["max_iter"][r]), connectivity=int(g["grid_connectivity"][k]),
                               diagonal_cost_multiplier=float(g["grid_mult"][k]))
        if not rec["found"]:
            assert xy is None, run_name(r)
        else:
            assert xy.dtype == rec["path"].dtype and xy.shape == rec["path"].shape and (xy == rec["path"]).all(), run_name(r)
    graph = list(np.flatnonzero(plain & (g["mode"] == 0) & (g["kind"] == A.H_OCTILE))[:2])
    graph += list(np.flatnonzero(plain & (g["mode"] == 0) & (g["kind"] == A.H_EUCLIDEAN) & (g["found"] == 0))[:1])
    graph += list(np.flatnonzero(plain & (g["mode"] == 0) & (g["max_iter"] < 100000) & (g["max_iter"] > 1))[:2])
    for r in graph:
        k, rec = int(g["grid_id"][r]), recorded(r)
        path, cost = search.AStar.plan_graph(int(g["source"][r]), int(g["target"][r]), grid_of(k), markers[int(g["kind"][r])],
                                             int(g["max_iter"][r]), int(g["grid_connectivity"][k]), float(g["grid_mult"][k]))
        assert path == [int(c) for c in rec["path"]] and cost == rec["cost"], run_name(r)
    # a callable of (cell, target cell) through the table: the euclidean formula written by the caller gives the marker's answer
    r = graph[0]
    k, w = int(g["grid_id"][r]), int(g["grid_hw"][g["grid_id"][r]][1])
    mine = lambda i, t: float(np.sqrt((i % w - t % w) ** 2 + (i // w - t // w) ** 2))   # noqa: E731
    args = (int(g["source"][r]), int(g["target"][r]), grid_of(k))
    assert search.AStar.plan_graph(*args, mine, connectivity=8) == search.AStar.plan_graph(*args, search.euclidean_heuristic, connectivity=8)


def test_a_fresh_random_batch_equals_the_specification(torch):
    rng = np.random.RandomState(20261021)
    for conn in (4, 8):
        for scale in (1.0, 2.5):
            rows = []
            for _ in range(12):
                h, w = int(rng.randint(2, 25)), int(rng.randint(2, 25))
                grid = rng.choice([0.1, 0.25, 0.5, 0.9, 1.0, 2.0, 3.5], size=(h, w))
                grid[rng.rand(h, w) < rng.choice([0.0, 0.15, 0.35])] = np.inf
                free = np.flatnonzero(np.isfinite(grid.reshape(-1)))
                if len(free) < 2:
                    continue
                s, t = (int(v) for v in rng.choice(free, 2, replace=False))
                rows.append(_row(grid, s, t, htarget=(t % w + rng.uniform(-0.5, 0.5), t // w + rng.uniform(-0.5, 0.5))))
            stride = max(r["weight"].size for r in rows)
            rc, out = _raw(torch, rows, stride, conn, SQRT2, A.H_EUCLIDEAN, scale, 100000, stride, 0.25, (1.5, -2.0))
            assert rc == 0
            for i, r in enumerate(rows):
                want = A.solve(r["weight"], r["source"], r["target"], A.H_EUCLIDEAN, r["htarget"], None, scale, conn, SQRT2, 100000, stride,
                               0.25, (1.5, -2.0))
                _same(out, i, want, r["weight"].size, (conn, scale, i))
            assert (out["status"] == A.FOUND).sum() >= 6


def test_occupancy_grid_to_astar_to_polyline_routes_on_a_generated_parking_pool(torch):
    """the planned path goes into t2d_polyline_routes as it is: the installed vertices equal those of the same polyline installed
    from the host, bit for bit"""
    from tactics2d_amd import search
    from tactics2d_amd.participant import VEHICLE_TEMPLATE, vehicle_row
    from tactics2d_amd.pool import ParticipantPool
    from tactics2d_amd.sensor import OccupancyGrid
    n, H, W, cap = 6, 33, 70, 160
    pool = ParticipantPool(n, 1)
    try:
        pool.set_param_table(vehicle_row("medium_car")[None])
        pool.set_status_config(max_step=100)
        size = VEHICLE_TEMPLATE["medium_car"][:2]
        pool.parking_scenes(3, 0.5, size)
        origin = OccupancyGrid(pool, H, W, 0.5, inflate=0.3, vehicle_size=size).origin
        grid = pool.occupancy_grid(H, W, 0.5, origin, inflate=0.3)
        mask = grid.mask.cpu().numpy().reshape(n, -1)
        assert mask.any() and not mask.all()
        src = np.int32([np.flatnonzero(m == 0)[0] for m in mask])
        field = search.cost_to_go(grid.weight, src, connectivity=8).cpu().numpy().reshape(n, -1)
        tgt = np.int32([np.argmax(np.where(np.isfinite(f), f, -1.0)) for f in field])      # the farthest cell that can be reached
        out = search.AStar.plan_batch(grid.weight, src, tgt, connectivity=8, max_path=cap, **grid.planner_kwargs())
        status, length = out.status.cpu().numpy(), out.path_len.cpu().numpy()
        assert (status == search.FOUND).all() and length.min() >= 10 and length.max() <= cap
        path, xy = out.path.cpu().numpy(), out.path_xy.cpu().numpy()
        weight = grid.weight.cpu().numpy()
        for e in range(n):
            want = A.solve(weight[e], int(src[e]), int(tgt[e]), connectivity=8, max_path=cap, cell_size=0.5, origin=grid.origin)
            assert (path[e] == want["path"]).all() and xy[e].tobytes() == want["path_xy"].tobytes(), e
        pool.set_routes([[np.float32([[float(k), -50.0 - e] for k in range(cap)])] for e in range(n)], np.arange(n), 0, 1.5)
        count = pool.polyline_routes(out.path_xy, out.path_len)
        pool.sync()
        assert count.cpu().tolist() == length.tolist()
        device = pool.route_vertices().cpu().numpy().copy()
        host = [np.float32(np.concatenate([xy[e, :length[e]], np.repeat(xy[e, length[e] - 1:length[e]], cap - length[e], 0)])) for e in range(n)]
        pool.set_routes([[v] for v in host], np.arange(n), 0, 1.5)
        assert device.tobytes() == pool.route_vertices().cpu().numpy().tobytes()
    finally:
        pool.close()
