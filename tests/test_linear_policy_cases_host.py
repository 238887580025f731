"""The cases of tests/linear_policy_cases.py meet their honesty conditions -- checked on the CPU: the same closed loop (the
restated policy on the observation, then a step) around the oracle, on Philox streams keyed like the handles', over the
launches of the GPU test.  Seeds and gains are settled here, not on the GPU.  (The handles' numpy streams draw other start
states and noise; the conditions are about what the POLICIES do -- fractions of clipped actions, envs that reach the target or
run into a wall -- and the GPU test asserts them again on what it ran.)"""
import warnings

import numpy as np
import pytest

import linear_policy_cases as lc
import linear_policy_ref as ref
from mdp_playground_amd import mdp as mdp_mod

N_CPU = 64        # a fifth of the GPU test's envs: the first 64 policies of the same draw


def _oracle(m):
    from oracle import oracle as ora
    o = ora.ContinuousOracle(m.D, m.relevant_indices, m.order, m.inertia, m.time_unit, m.state_space_max, m.action_space_max,
                             m.target_point, m.target_radius, m.make_denser, m.action_loss_weight, m.transition_noise,
                             m.reward_noise, m.delay, m.reward_every_n_steps, m.reward_scale, m.reward_shift,
                             m.term_state_reward, m.box_lo, m.box_hi)
    if m.target_default:
        o.set_target64()
    return o


def closed_loop(name, n=N_CPU, T=lc.K * lc.LAUNCHES):
    c = lc.CASES[name]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = mdp_mod.build_mdp(dict(c["config"]))
    theta = lc.theta_of(name)[:n]
    mode = c["kw"].get("autoreset", "same_step")
    max_steps = c["kw"].get("max_episode_steps") or 0
    D = c["D"]
    acts = np.zeros((T, n, D), np.float32)
    obs_out = np.zeros((T, n, D), np.float32)
    term = np.zeros((T, n), bool)
    trunc = np.zeros((T, n), bool)
    for i in range(n):
        o = _oracle(m)
        o.set_philox(77, lc.OFF + i)
        obs = o.reset()
        steps, pending = 0, False
        for t in range(T):
            a = ref.linear_actions(theta[i], obs[None], m.action_space_max)[0]
            acts[t, i] = a
            if pending:
                obs = o.reset(explicit=False)
                steps, pending = 0, False
                obs_out[t, i] = obs
                continue
            obs, _, _, d = o.step(a)
            steps += 1
            tr = bool(max_steps) and steps >= max_steps
            term[t, i], trunc[t, i] = d, tr
            if (d or tr) and mode == "same_step":
                obs = o.reset(explicit=False)
                steps = 0
            elif (d or tr) and mode == "next_step":
                pending = True
            obs_out[t, i] = obs
    return lc.conditions(name, acts, term, trunc, obs_out)


@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_case_meets_its_conditions_on_the_oracle(name):
    fig = closed_loop(name)
    print(name, fig)
    # (a ``near`` case: no env reaches the target from a reset state -- shown here -- and the oracle has no state setter; on the
    #  GPU the envs placed next to the target terminate, which that test asserts)
    if lc.CASES[name]["near"]:
        assert fig["terminations"] == 0, (name, fig)
    lc.assert_conditions(name, fig, terminations=not lc.CASES[name]["near"])


def test_per_env_parameters_differ_between_envs():
    for name in sorted(lc.CASES):
        th = lc.theta_of(name)
        assert th.shape == (lc.N, lc.CASES[name]["D"], lc.CASES[name]["D"] + 1) and th.dtype == np.float32
        o = np.random.default_rng(3).uniform(-0.5, 0.5, (1, lc.CASES[name]["D"])).astype(np.float32)
        assert not np.array_equal(ref.linear_actions(th[0], o, 1.0), ref.linear_actions(th[1], o, 1.0)), name
