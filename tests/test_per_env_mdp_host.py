"""One MDP per env for the in-kernel learners, without a GPU: the CPU closed loop (tests/per_env_mdp_cpu.py) over the set-up of
tests/test_gpu_per_env_mdp.py meets the conditions that file relies on -- the tables differ from env to env, so a kernel that
reads table 0, table `tid` or a neighbour's table cannot pass; most envs learn something, in both workgroups; episodes end;
explored selections, greedy ties and strict maxima all occur; double Q-learning updates both tables.  The floors are below
the counts measured with exactly this set-up (per_env_mdp_cpu.FLOORS)."""
import ctypes
import os
import re

import numpy as np
import pytest

import per_env_mdp_cpu as pm

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.mark.parametrize("case", list(pm.CASES))
def test_every_env_has_its_own_tables(case):
    mdps = pm.build_mdps(pm.CASES[case][0])
    assert len(mdps) == pm.N == 320
    P = np.stack([np.asarray(m.P) for m in mdps]).reshape(pm.N, -1)
    assert len({p.tobytes() for p in P}) == pm.N             # pairwise different
    assert not np.array_equal(P[0], P[256])                  # same lane, other workgroup
    assert not np.array_equal(P[1], P[0]) and not np.array_equal(P[257], P[1])


@pytest.mark.parametrize("algo", pm.ALGOS)
@pytest.mark.parametrize("case", list(pm.CASES))
def test_the_cpu_loop_meets_the_conditions_the_gpu_test_relies_on(case, algo):
    cfg, kw = pm.CASES[case]
    info, Q, traj = pm.closed_loop(cfg, kw, algo, pm.ALPHA, pm.GAMMA, pm.EPS)
    assert traj["actions"].shape == (pm.LAUNCHES * pm.K, pm.N) == (74, 320)
    counts = pm.check_floors(case, Q, traj["terminated"], algo)
    print(case, algo, "non-zero Q: all, lanes 0-255, lanes 256-319; envs that terminated:", counts,
          {k: v for k, v in info.items() if not isinstance(v, np.ndarray)})
    assert info["explored"] > 0 and info["greedy_ties"] > 0 and info["greedy_strict"] > 0, info
    assert info["updates"] == 74 * 320                       # (same-step autoreset: no reset call)
    if algo == "sarsa":
        assert info["carried"] > 0 and info["carried_differs"] > 0, info
    if algo == "double_q":
        assert info["updates_a"] > 0 and info["updates_b"] > 0 and info["cross_differs"] > 0, info
        assert pm.nonzero_envs(Q[:, 0]).any() and pm.nonzero_envs(Q[:, 1]).any()


def test_env_i_of_the_loop_is_the_one_env_loop_of_its_own_mdp():
    """the loop keys env i's words by off + i and steps it on MDP i: three envs, each against closed_loop_cpu.closed_loop of
    its own MDP alone"""
    import closed_loop_cpu
    cfg, kw = pm.CASES["s8_noise"]
    _, Q, traj = pm.closed_loop(cfg, kw, "sarsa", pm.ALPHA, pm.GAMMA, pm.EPS)
    for i in (0, 255, 256):
        _, q1, t1 = closed_loop_cpu.closed_loop({**cfg, "seed": pm.SEEDS[i]}, kw, "sarsa", pm.ALPHA, pm.GAMMA, pm.EPS, 1, seed=pm.SEED,
                                                K=pm.K, launches=pm.LAUNCHES, philox_seed=pm.PHILOX_SEED, off=pm.OFF + i)
        for k in ("actions", "obs", "terminated", "truncated"):
            assert np.array_equal(traj[k][:, i], t1[k][:, 0]), (i, k)
        assert np.array_equal(traj["reward"][:, i].view(np.int32), t1["reward"][:, 0].view(np.int32)), i
        assert np.array_equal(Q[i].view(np.int32), q1[0].view(np.int32)), i


def test_the_option_bit_and_the_export():
    from mdp_playground_amd import _capi
    assert _capi.OPTIONS["NO_PM_LDS"] == 1 << 21
    assert len(set(_capi.OPTIONS.values())) == len(_capi.OPTIONS)
    assert "mdpp_learner_per_env_mdp" in _capi.EXPORTS
    header = open(os.path.join(ROOT, "include", "mdpp.h")).read()
    assert re.search(r"MDPP_OPT_NO_PM_LDS\s*=\s*1u\s*<<\s*21\b", header)
    assert re.search(r"\bint\s+mdpp_learner_per_env_mdp\s*\(\s*mdpp_env\s*\*\s*h\s*,\s*int\s+on\s*\)\s*;", header)
    lib = ctypes.CDLL(_capi.LIB_PATH)
    assert hasattr(lib, "mdpp_learner_per_env_mdp")
    lib.mdpp_learner_per_env_mdp.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert lib.mdpp_learner_per_env_mdp(None, 1) == -1      # MDPP_EINVAL: no handle (nothing touches the GPU)
