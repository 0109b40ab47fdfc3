"""The walking addresses of the persistent pendulum kernel's prefetched-draws rollout loop (kernels_fused.hpp, INJ == 2).

The loop loads its draws through a per-trajectory pointer that steps once per trip of two blocks, and sigma / mean through
two LDS bases that step with it; none of the three is clamped at its array's end, so the last trip reads up to two float4
past a trajectory's row of the noise buffer (the next row, or the pad behind the chunk buffer: csrc/noise_extent.hpp) and,
with H a multiple of four, one float4 past sigma[] and mean[] in LDS.  Nothing read there may reach a result:

 * CEM and PI2 with two agents (a row behind agent 0's, and a last agent), populations 64 and 512 (no slack rows behind
   the population; 512 and 500 run the compile-time-stride body, 64 and 70 the run-time-stride one) and horizons 3, 4, 7, 8,
   9, 13, 30, 31 (every remainder, an odd and an even block count, no trip at all, and 31 as the last horizon whose sample
   stores are immediate offsets): the resident pass, a launch per call and the in-kernel draws (the generic loop: another
   code path, no noise buffer at all -- the partner of tests/test_gpu_rollout_loop_forms.py) agree bit for bit over 10
   closed-loop calls, which cross a boundary of the 8-step prefetch chunks;
 * the last control step of a chunk at N == Nst = 512, H = 8, on the last agent: its last trajectory's loads end exactly on
   the pad's last float4 (NaNs).  The record is finite and the same in all three runs.
"""
import numpy as np
import pytest

from oracle import oracle_np as O

pytestmark = pytest.mark.gpu
LO, HI = [-2.0], [2.0]
A, ITERS, CALLS, CHUNK = 2, 3, 10, 8

NS = [64, 70, 500, 512]
HS = [3, 4, 7, 8, 9, 13, 30, 31]
MODES = {  # name -> environment
    "resident": {"BBMPC_NOISE_PREFETCH": "1", "BBMPC_LINGER_US": None},
    "launch": {"BBMPC_NOISE_PREFETCH": "1", "BBMPC_LINGER_US": "0"},
    "in_kernel": {"BBMPC_NOISE_PREFETCH": "0", "BBMPC_LINGER_US": "0"},
}


@pytest.fixture(scope="module")
def L():
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib
    assert _lib.device_count() >= 1, "no gfx950 device visible"
    return _lib


_RUNS = {}


def _run(L, opt_name, N, H, mode):
    """[CALLS][A * 5] closed-loop records (actions | next states | rewards) and (served resident, launched); computed once."""
    key = (opt_name, N, H, mode)
    if key not in _RUNS:
        from blackbox_mpc_amd.engine import Engine
        mp = pytest.MonkeyPatch()
        try:
            mp.setenv("BBMPC_FUSED", "1")
            mp.delenv("BBMPC_BALANCE", raising=False)
            for k, v in MODES[mode].items():
                if v is None:
                    mp.delenv(k, raising=False)
                else:
                    mp.setenv(k, v)
            opt = {"CEM": L.OPT_CEM, "PI2": L.OPT_PI2}[opt_name]
            eng = Engine(opt, L.DYN_PENDULUM, L.REW_PENDULUM, LO, HI, dim_s=3, num_agents=A, planning_horizon=H,
                         population_size=N, max_iterations=ITERS, num_elite=max(N // 10, 1), seed=17)
            s = O.pendulum_start_states(A)
            out = []
            for _ in range(CALLS):
                a, s, r = eng.optimize(s)
                out.append(np.concatenate([np.ravel(a), np.ravel(s), np.ravel(r)]).astype(np.float32))
            stats = eng.call_stats()
            eng.close()
        finally:
            mp.undo()
        _RUNS[key] = (np.stack(out), stats)
    return _RUNS[key]


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("opt_name", ["CEM", "PI2"])
def test_resident_launch_and_in_kernel_draws_agree_bit_for_bit(L, opt_name, N, H):
    resident, (served, launched) = _run(L, opt_name, N, H, "resident")
    launch, (served_l, launched_l) = _run(L, opt_name, N, H, "launch")
    partner, _ = _run(L, opt_name, N, H, "in_kernel")
    print("%s N=%d H=%d: resident run served %d launched %d" % (opt_name, N, H, served, launched))
    assert served + launched == CALLS and served > 0              # the resident form did run
    assert (served_l, launched_l) == (0, CALLS)
    assert np.isfinite(partner).all()
    np.testing.assert_array_equal(_bits(launch), _bits(partner))
    np.testing.assert_array_equal(_bits(resident), _bits(launch))


@pytest.mark.parametrize("opt_name", ["CEM", "PI2"])
def test_last_step_of_a_chunk_reads_the_pad_and_uses_none_of_it(L, opt_name):
    # N == Nst and H = 8 (two blocks, no remainder: the one trip loads blocks 2 and 3 of a two-block row): in control step
    # CHUNK - 1 the last agent's last trajectory loads the two float4 of the pad behind the chunk buffer
    N, H, last = 512, 8, A - 1
    resident, (served, _) = _run(L, opt_name, N, H, "resident")
    launch, _ = _run(L, opt_name, N, H, "launch")
    partner, _ = _run(L, opt_name, N, H, "in_kernel")
    cols = [last] + [A + 3 * last + i for i in range(3)] + [A + 3 * A + last]     # action | next state | reward of the last agent
    rec = launch[CHUNK - 1][cols]
    print("%s step %d agent %d: launch %s resident %s" % (opt_name, CHUNK - 1, last, rec, resident[CHUNK - 1][cols]))
    assert served > 0
    assert np.isfinite(rec).all()        # (a NaN draw that was used would make its trajectory's reward -1e6 and move the elite set: the partner below)
    np.testing.assert_array_equal(_bits(resident[CHUNK - 1][cols]), _bits(rec))
    np.testing.assert_array_equal(_bits(partner[CHUNK - 1][cols]), _bits(rec))
