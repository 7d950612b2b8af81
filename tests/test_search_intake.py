"""The intake the five batch functions of tactics2d_amd.search share: what it refuses, it refuses as ValueError BEFORE the library is
loaded, a stream is looked up or anything is uploaded -- `_ffi.lib` and `search._stream_of` are replaced by functions that raise."""
import inspect

import numpy as np
import pytest

GRIDS = np.ones((2, 3, 4))
BOUNDARY = [0.0, 3.0, 0.0, 2.0]
# a call that is in order, by keyword
CALLS = {
    "plan_batch": dict(weight_grids=GRIDS, sources=[0, 0], targets=[5, 5]),
    "astar_plan_batch": dict(weight_grids=GRIDS, sources=[0, 0], targets=[5, 5]),
    "hybrid_plan_batch": dict(starts=np.zeros((2, 3)), targets=np.ones((2, 3)), boundaries=BOUNDARY, weight_grids=GRIDS),
    "sample_plan_batch": dict(kind="rrt", starts=np.zeros((2, 2)), targets=np.ones((2, 2)), boundaries=BOUNDARY, weight_grids=GRIDS, seeds=7),
    "prm_plan_batch": dict(starts=np.zeros((2, 2)), targets=np.ones((2, 2)), boundaries=BOUNDARY, weight_grids=GRIDS, seeds=7, n_samples=30),
}
# what the intake refuses: (the argument, its value); an argument a function does not take is no case of it
REFUSED = [("weight_grids", np.ones(12)), ("weight_grids", np.ones((2, 0, 4))), ("weight_grids", np.ones((0, 4))), ("max_path", -1),
           ("cell_size", 0), ("cell_size", float("nan")), ("origin", (0.0, float("inf"))), ("starts", "one row more"),
           ("seeds", np.arange(3, dtype=np.uint64))]
TAKES = {"plan_batch": (), "astar_plan_batch": ("cell_size", "origin"), "hybrid_plan_batch": ("cell_size", "origin", "starts"),
         "sample_plan_batch": ("cell_size", "origin", "starts", "seeds"), "prm_plan_batch": ("cell_size", "origin", "starts", "seeds")}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_the_intake_refuses_before_any_device_or_library_call(name, monkeypatch):
    from tactics2d_amd import _ffi, search

    def reached(*a, **kw):
        raise AssertionError("the library or the device was reached before the refusal")
    monkeypatch.setattr(_ffi, "lib", reached)
    monkeypatch.setattr(search, "_stream_of", reached)
    fn = getattr(search, name)
    parameters = inspect.signature(fn).parameters
    assert {"weight_grids", "max_path", "hw"} <= set(parameters)
    assert set(TAKES[name]) == {k for k in ("cell_size", "origin", "starts", "seeds") if k in parameters}
    with pytest.raises(AssertionError, match="was reached"):   # (the call in order gets as far as the library)
        fn(**CALLS[name])
    cases = 0
    for key, value in REFUSED:
        if key not in parameters:
            continue
        call = dict(CALLS[name])
        call[key] = np.zeros((3, np.shape(call["starts"])[1])) if key == "starts" else value
        with pytest.raises(ValueError):
            fn(**call)
        cases += 1
    assert cases == 4 + 2 * ("cell_size" in parameters) + sum(k in parameters for k in ("origin", "starts", "seeds"))
