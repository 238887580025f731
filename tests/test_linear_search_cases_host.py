"""The cases of tests/linear_search_cases.py meet the conditions that keep a bit-for-bit GPU pass honest -- checked on the CPU: the
same closed loop (the restated policy on the observation, a step, the restated search rule) around the oracle, on Philox
streams keyed like the handles', over the three launches of the GPU test and the first 64 envs (one wave).  Seeds and step
sizes are settled here, not on the GPU.

  every env finishes at least 2 trials;
  of the trials after trial 0 at least 5 % are accepted and at least 5 % rejected;
  at some step some lanes of the wave end a trial and some do not (a ``near`` case: the oracle has no state setter, no env of
  these configs reaches the target from a reset state and every trial of the wave ends at the same step -- shown here; on the
  GPU the placed envs shift theirs, which tests/test_gpu_linear_search.py asserts on what it ran);
  at least one candidate entry differs between best + sigma z with and without a fused multiply-add;
  a trial is in progress across a launch boundary."""
import warnings

import numpy as np
import pytest

import linear_policy_ref as ref
import linear_search_cases as sc
import linear_search_ref as lsr
from mdp_playground_amd import mdp as mdp_mod
from test_linear_policy_cases_host import _oracle

N_CPU = 64


def closed_loop(name, n=N_CPU, steps=sc.K * sc.LAUNCHES):
    c = sc.CASES[name]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = mdp_mod.build_mdp(dict(c["config"]))
    mode = c["kw"].get("autoreset", "same_step")
    max_steps = c["kw"].get("max_episode_steps") or 0
    s = lsr.new_state(sc.theta_of(name)[:n], sc.sigma_of(name, n))
    ended = np.zeros((steps, n), bool)
    drawn = {}

    def normals(seed, env, tick, count):
        drawn["z"] = lsr._normals(seed, env, tick, count)
        return drawn["z"]

    fma_differs = entries = 0
    for i in range(n):
        o = _oracle(m)
        o.set_philox(77, sc.OFF + i)
        obs = o.reset()
        count, pending = 0, False
        for t in range(steps):
            a = ref.linear_actions(s["cand"][i], obs[None], m.action_space_max)[0]
            if pending:
                obs = o.reset(explicit=False)
                count, pending = 0, False
                continue
            obs, r, _, d = o.step(a)
            count += 1
            tr = bool(max_steps) and count >= max_steps
            s["ret"][i] += float(np.float32(r))
            if d or tr:
                if lsr.end_episode(s, i, seed=sc.SEED, env_id=sc.OFF + i, T=c["T"], up=c["up"], down=c["down"],
                                   sigma_max=c["sigma_max"], normals=normals):
                    ended[t, i] = True
                    fused = lsr.perturb_fma(s["best"][:, i], s["sigma"][i], drawn["z"])
                    fma_differs += int((fused.view(np.uint32) != s["cand"][i].reshape(-1).view(np.uint32)).sum())
                    entries += fused.size
                if mode == "same_step":
                    obs = o.reset(explicit=False)
                    count = 0
                elif mode == "next_step":
                    pending = True
    fig = sc.figures(ended, s["trial"], s["accepted"])
    fig.update(fma_differs=fma_differs, entries=entries, sigma_min=float(s["sigma"].min()), sigma_max=float(s["sigma"].max()))
    return fig


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_case_meets_its_conditions_on_the_oracle(name):
    fig = closed_loop(name)
    print(name, fig)
    near = bool(sc.CASES[name]["near"])
    if near:
        assert fig["mixed_wave_steps"] == 0, (name, fig)
    sc.assert_figures(name, fig, mixed=not near)
    assert fig["fma_differs"] > 0, (name, fig)
    if name == "d3_order2_rel20_box":        # the clamp is reached, and sigma has moved both ways
        assert fig["sigma_max"] == 2.0 and fig["sigma_min"] < 0.3, (name, fig)


def test_the_zero_sigma_envs_keep_their_start_policy():
    th = sc.theta_of("c_d2_n0_sigma_zeros")
    sg = sc.sigma_of("c_d2_n0_sigma_zeros")
    assert sg.dtype == np.float32 and (sg[::3] == 0).all() and (np.delete(sg, np.s_[::3]) > 0).all()
    z = lsr._normals(sc.SEED, sc.OFF, 1, 6)
    assert np.array_equal(lsr.perturb(th[0].reshape(-1), sg[0], z), th[0].reshape(-1))
    assert not np.array_equal(lsr.perturb(th[1].reshape(-1), sg[1], z), th[1].reshape(-1))


def test_cases_cover_what_the_gpu_test_needs():
    names = set(sc.CASES)
    assert {"c_d2_n0", "c_d2_n0_no_lds", "d3_order2_rel20_box", "d4_delay3_every2_alw", "d4_delay3_every2_alw_no_lds", "cfg3", "cfg5",
            "autoreset_same_step", "autoreset_next_step", "max5_autoreset_disabled", "c_d2_n0_sigma_zeros"} <= names
    assert (sc.N, sc.K, sc.LAUNCHES) == (320, 37, 3) and sc.RNGS == ("numpy", "philox")
    assert sc.CASES["d3_order2_rel20_box"]["T"] == 2 and sc.CASES["d3_order2_rel20_box"]["up"] != 1 != sc.CASES["d3_order2_rel20_box"]["down"]
    assert sc.CASES["cfg5"]["near"] and sc.CASES["cfg5"]["plds"] == 0 and sc.CASES["cfg3"]["plds"] is None
    for name in ("c_d2_n0_no_lds", "d4_delay3_every2_alw_no_lds"):
        assert sc.CASES[name]["opts"] == ("NO_LINEAR_LDS",) and sc.CASES[name]["plds"] == 0
    for name, c in sc.CASES.items():
        assert c["kw"]["max_episode_steps"] > 0, name
