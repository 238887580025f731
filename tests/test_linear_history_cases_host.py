"""The cases of tests/linear_history_cases.py meet their honesty conditions -- checked on the CPU: the same closed loop (the
restated policy with memory on the observation, then a step) around the oracle, on Philox streams keyed like the handles', over
the launches of the GPU test.  Seeds and gains are settled here, not on the GPU.  (The handles' numpy streams draw other start
states and noise; the conditions are about what the POLICIES do, and the GPU test asserts them again on what it ran.)

The loop keeps the memory and the step count itself, env by env, as include/mdpp.h states them; the launch-wise restatement of
tests/linear_history_ref.py, fed the loop's outputs cut into the GPU test's launches, must find the same actions."""
import warnings

import numpy as np
import pytest

import linear_history_cases as hc
import linear_history_ref as href
from mdp_playground_amd import mdp as mdp_mod
from test_linear_policy_cases_host import _oracle


def closed_loop(name, n=hc.N, K=hc.K, launches=hc.LAUNCHES):
    c = hc.CASES[name]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = mdp_mod.build_mdp(dict(c["config"]))
    theta = hc.theta_of(name)[:n]
    mode = hc.mode_of(name)
    max_steps = c["kw"].get("max_episode_steps") or 0
    D, T = c["D"], K * launches
    acts, obs_out, os_, ps = (np.zeros((T, n, D), np.float32) for _ in range(4))
    term, trunc, first = (np.zeros((T, n), bool) for _ in range(3))
    obs0 = np.zeros((n, D), np.float32)
    for i in range(n):
        o = _oracle(m)
        o.set_philox(77, hc.OFF + i)
        obs = o.reset()
        obs0[i] = obs
        mem = np.asarray(obs, np.float32).copy()
        steps, pending = 0, False
        for t in range(T):
            cur = np.asarray(obs, np.float32)
            p = cur if steps == 0 else mem
            a = href.history_actions(theta[i], cur[None], p[None], m.action_space_max)[0]
            acts[t, i], os_[t, i], ps[t, i], first[t, i] = a, cur, p, steps == 0
            mem = cur.copy()
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
    # the launch-wise restatement on the same outputs
    carry, start, cut = href.new_carry(obs0), obs0, []
    for l in range(launches):
        s = slice(l * K, (l + 1) * K)
        a2, p2, f2, carry = href.launch(theta, carry, start, obs_out[s], term[s], trunc[s], mode, m.action_space_max)
        assert np.array_equal(a2.view(np.uint32), acts[s].view(np.uint32)), (name, l)
        assert np.array_equal(p2.view(np.uint32), ps[s].view(np.uint32)) and np.array_equal(f2, first[s]), (name, l)
        cut.append((acts[s], obs_out[s], term[s], trunc[s], os_[s], ps[s], first[s]))
        start = obs_out[s][-1]
    return hc.conditions(name, theta, cut, amax=m.action_space_max, smax=m.state_space_max)


@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_case_meets_its_conditions_on_the_oracle(name):
    fig = closed_loop(name)
    print(name, fig)
    # (a ``near`` case: the oracle has no state setter, so the envs the GPU test places next to the target are not placed here;
    #  what hangs on their terminations -- the episode boundaries that fall apart inside a wave -- is asserted on the GPU)
    hc.assert_conditions(name, fig, terminations=not hc.CASES[name]["near"])


def test_parameters_have_the_layout_of_the_header_and_v_is_there():
    for name in sorted(hc.CASES):
        D = hc.CASES[name]["D"]
        th = hc.theta_of(name)
        assert th.shape == (hc.N, D, 2 * D + 1) and th.dtype == np.float32
        assert hc.without_v(th).shape == (hc.N, D, D + 1)
        assert np.array_equal(hc.without_v(th)[..., D], th[..., 2 * D])
        kd = np.float32(hc.CASES[name]["kd"])
        diag = th[:, np.arange(D), D + np.arange(D)]
        assert abs(float(diag.mean()) - float(kd)) < 0.05, name
        if name.endswith("_no_lds"):
            assert np.array_equal(th, hc.theta_of(name[:-len("_no_lds")]))
