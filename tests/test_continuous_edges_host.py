"""Continuous envs at the edges of float32, on the CPU (tests/continuous_edge_cases.py holds the cases and scripts).

(1) Equivalence: for every move_to_a_point case the C oracle (oracle/mdpp_oracle.c) and the numpy restatement of the
    reference (baseline/py_step.py, pinned to the reference's goldens by tests/test_py_baseline.py) run the scripts of 8 envs:
    states equal by bits, rewards equal as float32 with NaN equal to NaN, flags equal.  This decides what
    tests/test_gpu_continuous_edges.py expects of the kernels; where the two differed, the reference's lines were read and the
    wrong one fixed (the oracle lacked the NaN gate of rl_toy_env.py:1858).
(2) Coverage: per case, from the oracle's trajectories alone, every edge the case is there for occurs -- so that a script
    cannot quietly miss it.
"""
import functools
import warnings

import numpy as np
import pytest

import continuous_edge_cases as cec

N_HOST = 8


def build(name):
    from mdp_playground_amd import mdp as mdp_mod
    return mdp_mod.build_mdp(cec.CASES[name]["config"])


def shared_mdp_streams(name, n):
    """The env and feature-space stream words RLToyVectorEnv gives envs 0 .. n-1 of a shared-MDP handle."""
    from mdp_playground_amd import mdp as mdp_mod
    m = build(name)
    return (mdp_mod.fresh_stream_words(cec.CASES[name]["config"]["seed"], n),
            mdp_mod.fresh_stream_words(m.seed_dict["state_space"], n))


def oracle_for(m):
    from oracle import oracle as ora
    o = ora.ContinuousOracle(m.D, m.relevant_indices, m.order, m.inertia, m.time_unit, m.state_space_max, m.action_space_max,
                             m.target_point, m.target_radius, m.make_denser, m.action_loss_weight, m.transition_noise,
                             m.reward_noise, m.delay, m.reward_every_n_steps, m.reward_scale, m.reward_shift,
                             m.term_state_reward, m.box_lo, m.box_hi)
    if m.reward_function == "move_along_a_line":
        o.set_line_reward(m.sequence_length, m.delay)
    elif m.target_default:
        o.set_target64()
    return o


class OracleEnv:
    """The driver's view of a ContinuousOracle: numpy streams from their words, or Philox streams keyed by the env id."""

    def __init__(self, m, env_words=None, space_words=None, philox=None):
        self.o = oracle_for(m)
        if philox is not None:
            self.o.set_philox(*philox)
        else:
            self.o.set_rng(env_words, space_words)

    def reset(self):
        return self.o.reset()

    def auto_reset(self):
        return self.o.reset(explicit=False)

    def step(self, a):
        obs, r, _, d = self.o.step(a)
        return obs, r, d

    def derivs(self):
        return self.o.derivs()

    def streams(self):
        return self.o.get_rng()


class PyEnv:
    """The driver's view of baseline.py_step.PyContinuousEnv."""

    def __init__(self, m, env_words, space_words):
        from baseline import py_step
        self.e = py_step.from_mdp(m, env_words, space_words)

    def reset(self):
        return self.e.reset()

    auto_reset = reset

    def step(self, a):
        obs, r, d, _ = self.e.step(np.array(a, np.float32))
        return obs, r, d

    def derivs(self):
        return np.array(self.e.state_derivatives, np.float32)

    def streams(self):
        from mdp_playground_amd import mdp as mdp_mod
        return mdp_mod.pcg64_words(self.e.np_random), mdp_mod.pcg64_words(self.e.space_rng)


@functools.lru_cache(maxsize=None)
def oracle_trajectories(name, autoreset, rng, n, philox_seed=23):
    """The oracle's trajectory of envs 0 .. n-1 of a case (computed once per argument tuple; callers must not write to it)."""
    c = cec.CASES[name]
    m = build(name)
    acts = cec.scripts(name, n)
    ew, sw = shared_mdp_streams(name, n)
    out = []
    for i in range(n):
        env = OracleEnv(m, philox=(philox_seed, i)) if rng == "philox" else OracleEnv(m, ew[i], sw[i])
        out.append(cec.drive(env, acts[:, i], c["config"], c["max_episode_steps"], autoreset))
    return acts, out


def _same(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("name,autoreset", [(n, ar) for n in cec.POINT_CASES for ar in cec.CASES[n]["autoreset"]])
def test_oracle_equals_numpy_restatement_at_the_edges(name, autoreset):
    c = cec.CASES[name]
    m = build(name)
    acts, exp = oracle_trajectories(name, autoreset, "numpy", N_HOST)
    ew, sw = shared_mdp_streams(name, N_HOST)
    for i in range(N_HOST):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")          # numpy's "invalid value" on inf - inf and 0 * inf: the values are the point
            got = cec.drive(PyEnv(m, ew[i], sw[i]), acts[:, i], c["config"], c["max_episode_steps"], autoreset)
        e = exp[i]
        assert _same(got["init"], e["init"]), (name, i)
        for t in range(cec.T):
            assert _same(got["obs"][t], e["obs"][t]) and _same(got["final"][t], e["final"][t]), (name, i, t, got["obs"][t], e["obs"][t])
            gr, er = got["reward"][t], e["reward"][t]
            assert (np.isnan(gr) and np.isnan(er)) or gr == er, (name, i, t, gr, er)
            assert got["term"][t] == e["term"][t] and got["trunc"][t] == e["trunc"][t], (name, i, t)
            assert _same(got["derivs_pre"][t], e["derivs_pre"][t]), (name, i, t)
        for k in range(len(cec.LAUNCHES)):
            for s in (0, 1):
                assert np.array_equal(got["streams"][k][s][:4], e["streams"][k][s][:4]), (name, i, k, s)


@pytest.mark.parametrize("name", list(cec.CASES))
def test_scripts_reach_their_edges(name):
    c = cec.CASES[name]
    for autoreset in c["autoreset"]:
        acts, trajs = oracle_trajectories(name, autoreset, "numpy", N_HOST)
        counts = [cec.coverage(name, tr, acts[:, i]) for i, tr in enumerate(trajs)]
        mean = {k: sum(x[k] for x in counts) / N_HOST for k in counts[0]}
        for k, least in c["coverage"].items():
            assert mean[k] >= least, (name, autoreset, k, mean)
        if c["line"]:
            # the absolute tolerance of the line reward must not be all that is tested: the rewards are not all tiny
            L, scale, shift = c["config"]["sequence_length"], c["config"]["reward_scale"], c["config"]["reward_shift"]
            paid = big = 0
            for tr in trajs:
                n = 0
                for t in range(cec.T):
                    n += 1
                    if n >= L:
                        paid += 1
                        big += abs((float(tr["reward"][t]) - shift) / scale) >= 1e-2
                    if tr["trunc"][t]:
                        n = 0
            assert 3 * big >= paid > 0, (name, big, paid)


def test_scripts_share_lanes_0_to_63_and_rotate_the_rest():
    acts = cec.scripts("o2_inertia3", 300)
    assert acts.dtype == np.float32 and acts.shape == (cec.T, 300, 2)
    assert all(_same(acts[:, i], acts[:, 0]) for i in range(64)) and not _same(acts[:, 64], acts[:, 0])
    W = cec.wall_run_steps(cec.CASES["o2_inertia3"]["config"])
    assert (acts[:W] == 1.0).all() and not (acts[W] == 1.0).all()
    # whole waves that hold only admitted, only rejected, and both kinds of actions
    cfg = cec.CASES["o2_inertia3"]["config"]
    ok = np.array([[cec.admitted(cfg, acts[t, i]) for i in range(300)] for t in range(cec.T)])
    assert ok[:, :64].all(axis=1).any() and (~ok[:, :64]).all(axis=1).any()
    mixed = ok[:, 64:128].any(axis=1) & ~ok[:, 64:128].all(axis=1)
    assert mixed.sum() >= 10
