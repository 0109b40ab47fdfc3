"""The _fastcall extension (csrc/pyfast.cpp) against a stub of the ABI: what Engine.optimize / optimize_gather return on the
native path is what the ctypes body returns, input form by input form; fall-back, error code, reference counts, GIL."""
import sys
import threading
import time
import tracemalloc

import numpy as np
import pytest

from blackbox_mpc_amd import _lib as L
from tests.fastcall_util import StubEngine, observation


@pytest.fixture(scope="module", autouse=True)
def extension(built_lib):
    mod = L.fastcall()
    assert mod is not None, "the _fastcall extension must be built by _build.build()"
    return mod


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def assert_same(got, want, A, S, U):
    assert type(got) is tuple and len(got) == 3
    for g, w, shape in zip(got, want, ((A, U), (A, S), (A,))):
        assert type(g) is np.ndarray and g.dtype == np.float32 and g.shape == shape and g.flags.c_contiguous and g.flags.owndata
        assert w.dtype == np.float32 and w.shape == shape
        np.testing.assert_array_equal(bits(g), bits(w))


def took_native_path(eng):
    return bool(eng._fast) and "_io" not in eng.__dict__


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("A", [1, 3])
@pytest.mark.parametrize("S", [3, 20])
def test_input_forms_match_ctypes_body(dtype, A, S):
    U = 1 if S == 3 else 6
    fast, slow = StubEngine(A, S, U), StubEngine(A, S, U, fastcall=False)
    obs = observation(A, S, dtype, seed=A * 100 + S)
    if dtype is np.float64:
        obs[0, 0] = 1.0 / 3.0                      # not representable in float32: the cast has to round as NumPy's does
    keep = obs.copy()
    got, want = fast.optimize(obs, 7, True), slow.optimize(obs, 7, True)
    assert took_native_path(fast) and not slow._fast
    assert_same(got, want, A, S, U)
    np.testing.assert_array_equal(obs, keep)       # the input is read, never written
    # fresh objects on every call: mutating a result does not reach the next call's
    for g in got:
        g[...] = -12345.0
    again = fast.optimize(obs, 7, True)
    assert all(a is not g for a, g in zip(again, got))
    assert_same(again, want, A, S, U)
    assert fast.handle.calls == 2 and slow.handle.calls == 1


def test_large_observation_takes_the_heap_row():
    A, S, U = 20, 20, 6                            # A * S above the extension's on-stack conversion row
    fast, slow = StubEngine(A, S, U), StubEngine(A, S, U, fastcall=False)
    obs = observation(A, S, np.float64, seed=5)
    assert_same(fast.optimize(obs, 1), slow.optimize(obs, 1), A, S, U)
    assert took_native_path(fast)


def test_optimize_gather_matches_ctypes_body():
    A, S, U = 3, 3, 1
    fast, slow = StubEngine(A, S, U), StubEngine(A, S, U, fastcall=False)
    for dtype in (np.float32, np.float64):
        obs = observation(A, S, dtype, seed=2)
        got, want = fast.optimize_gather(obs, 0x7F0012345000, 1, 4, False), slow.optimize_gather(obs, 0x7F0012345000, 1, 4, False)
        assert_same(got, want, A, S, U)
        for e in (fast, slow):
            assert (e.handle.last_gathered, e.handle.last_slot) == (0x7F0012345000, 1)
    assert took_native_path(fast)


def _fallback_inputs(A, S):
    base = observation(A, 2 * S, np.float32, seed=9)
    return {"strided view": base[:, ::2], "int32 array": (observation(A, S, seed=3) * 10).astype(np.int32),
            "list": observation(A, S, seed=4).tolist(), "float16 array": observation(A, S, np.float16, seed=6)}


@pytest.mark.parametrize("form", ["strided view", "int32 array", "list", "float16 array"])
def test_fallback_inputs_go_through_the_python_body(form):
    A, S, U = 3, 3, 1
    fast, slow = StubEngine(A, S, U), StubEngine(A, S, U, fastcall=False)
    x = _fallback_inputs(A, S)[form]
    assert fast._bind_fast().optimize(x, 0, False) is NotImplemented
    assert_same(fast.optimize(x, 2), slow.optimize(x, 2), A, S, U)
    assert "_io" in fast.__dict__                  # the persistent arrays of the Python body were used
    assert_same(fast.optimize_gather(x, 4096, 0, 2), slow.optimize_gather(x, 4096, 0, 2), A, S, U)


@pytest.mark.parametrize("shape", [(3,), (2, 3), (3, 4), (1, 3, 3), (9,)])
def test_wrong_shape_raises_todays_text(shape):
    fast, slow = StubEngine(3, 3, 1), StubEngine(3, 3, 1, fastcall=False)
    x = np.zeros(shape, np.float32)
    texts = []
    for e in (fast, slow):
        for call in (lambda: e.optimize(x), lambda: e.optimize_gather(x, 4096, 0)):
            with pytest.raises(ValueError) as info:
                call()
            texts.append(str(info.value))
        assert e.handle.calls == 0
    assert len(set(texts)) == 1 and texts[0] == "state must be [num_agents, dim_S] = [3, 3], got %s" % (shape,)


def test_time_step_forms():
    A, S, U = 1, 3, 1
    fast, slow = StubEngine(A, S, U), StubEngine(A, S, U, fastcall=False)
    obs = observation(A, S)

    class Indexable:
        def __index__(self):
            return 11

    for t in (np.int64(5), np.int32(6), np.uint8(7), True, Indexable()):
        assert_same(fast.optimize(obs, t), slow.optimize(obs, t), A, S, U)
    assert took_native_path(fast)                  # every index-like t was taken natively
    # a float has no __index__: the Python body truncates it with int(), as it always did
    assert fast._fast.optimize(obs, 2.75, False) is NotImplemented
    assert_same(fast.optimize(obs, 2.75), slow.optimize(obs, 2), A, S, U)
    for bad in ("3x", None):
        for e in (fast, slow):
            with pytest.raises((TypeError, ValueError)):
                e.optimize(obs, bad)


def test_add_noise_by_truth_value():
    A, S, U = 1, 3, 1
    fast, slow = StubEngine(A, S, U), StubEngine(A, S, U, fastcall=False)
    obs = observation(A, S)
    for flag in (0, 1, np.bool_(True), [], [0], None, "x"):
        assert_same(fast.optimize(obs, 0, flag), slow.optimize(obs, 0, flag), A, S, U)
    for e in (fast, slow):
        with pytest.raises(ValueError):
            e.optimize(obs, 0, np.zeros(2))        # an ambiguous truth value raises on both paths
    assert took_native_path(fast)


def test_error_code_surfaces_as_the_same_exception():
    fast, slow = StubEngine(1, 3, 1, code=L.E_STATE), StubEngine(1, 3, 1, fastcall=False, code=L.E_STATE)
    obs = observation(1, 3)
    errs = []
    for e in (fast, slow):
        for call in (lambda: e.optimize(obs), lambda: e.optimize_gather(obs, 4096, 0)):
            with pytest.raises(L.BBMPCError) as info:
                call()
            errs.append((info.value.code, str(info.value)))
    assert len(set(errs)) == 1 and errs[0][0] == L.E_STATE
    assert fast._fast.optimize(obs, 0, False) == L.E_STATE        # the bound object hands the code back as an int
    fast.handle.code = 0
    assert type(fast.optimize(obs)) is tuple                      # and the handle goes on working


def test_overflowing_float64_is_left_to_numpy():
    fast, slow = StubEngine(1, 3, 1), StubEngine(1, 3, 1, fastcall=False)
    obs = np.array([[1e300, -1e300, 0.5]])
    assert fast._bind_fast().optimize(obs, 0, False) is NotImplemented
    with np.errstate(over="ignore"):
        assert_same(fast.optimize(obs), slow.optimize(obs), 1, 3, 1)
    inf = np.array([[np.inf, -np.inf, np.nan]])
    got, want = fast._fast.optimize(inf, 0, False), slow.optimize(inf)       # infinities and NaN are cast natively
    assert_same(got, want, 1, 3, 1)


def test_no_leaks_over_1e5_calls():
    A, S, U = 1, 3, 1
    bad = [[0.0, 0.0, 0.0]]
    # traced from before the first call: what the interpreter keeps per function (its cached frame) is then part of
    # `before`, and the growth below is what 10^5 calls of each kind left behind
    tracemalloc.start()
    try:
        eng = StubEngine(A, S, U)
        obs32, obs64 = observation(A, S), observation(A, S, np.float64)
        bound = eng._bind_fast()
        one = eng.optimize(obs32)
        one_result_bytes = sys.getsizeof(one) + sum(sys.getsizeof(x) for x in one)
        del one

        def loop(n):
            for i in range(n):
                eng.optimize(obs32, i, False)
                eng.optimize(obs64, i, None)
                bound.optimize(bad, i, False)          # NotImplemented
            eng.handle.code = -4
            for i in range(n // 10):
                bound.optimize(obs32, i, False)        # the error-code return: the three arrays are dropped
            eng.handle.code = 0

        loop(3000)
        refs = [sys.getrefcount(x) for x in (obs32, obs64, None, NotImplemented, bad)]
        before = tracemalloc.get_traced_memory()[0]
        loop(100000)
        after = tracemalloc.get_traced_memory()[0]
        refs_after = [sys.getrefcount(x) for x in (obs32, obs64, None, NotImplemented, bad)]
    finally:
        tracemalloc.stop()
    assert refs_after == refs
    assert after - before < one_result_bytes, (before, after, one_result_bytes)


def test_gil_is_released_around_the_library_call():
    n, sleep_us = 20, 1000
    engines = [StubEngine(1, 3, 1, sleep_us=sleep_us) for _ in range(2)]
    obs = observation(1, 3)
    for e in engines:
        e.optimize(obs)

    def drive(e):
        for i in range(n):
            e.optimize(obs, i)

    best = float("inf")
    for _ in range(3):
        threads = [threading.Thread(target=drive, args=(e,)) for e in engines]
        t0 = time.perf_counter()
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        best = min(best, time.perf_counter() - t0)
    # with the GIL held the 2 n sleeps are serial: at least 2 n ms.  Released, the pair overlaps: about n ms.
    serial = 2 * n * sleep_us * 1e-6
    assert best < 0.8 * serial, "two threads took %.1f ms for 2 x %d calls of 1 ms: the calls did not overlap" % (best * 1e3, n)
    assert all(took_native_path(e) for e in engines)


def test_switch_off_keeps_the_ctypes_path(monkeypatch):
    monkeypatch.setenv("BBMPC_FASTCALL", "0")
    off = StubEngine(1, 3, 1)
    monkeypatch.delenv("BBMPC_FASTCALL")
    on = StubEngine(1, 3, 1)
    obs = observation(1, 3)
    assert_same(on.optimize(obs, 3), off.optimize(obs, 3), 1, 3, 1)       # (read at creation: `off` stays off)
    assert off._fast is False and "_io" in off.__dict__ and took_native_path(on)


def test_extension_absent_warns_once_and_falls_back(monkeypatch, tmp_path):
    monkeypatch.setattr(L, "FASTCALL_PATH", str(tmp_path / "_fastcall_missing.so"))
    monkeypatch.setattr(L, "_fastcall_state", [])
    ref = StubEngine(1, 3, 1, fastcall=False)
    obs = observation(1, 3)
    with pytest.warns(RuntimeWarning) as rec:
        a, b = StubEngine(1, 3, 1), StubEngine(1, 3, 1)
        for e in (a, b):
            for t in range(3):
                assert_same(e.optimize(obs, t), ref.optimize(obs, t), 1, 3, 1)
            assert_same(e.optimize_gather(obs, 4096, 1, 2), ref.optimize_gather(obs, 4096, 1, 2), 1, 3, 1)
    assert len([w for w in rec if "_fastcall" in str(w.message)]) == 1
    assert a._fast is False and b._fast is False
