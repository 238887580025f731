"""The cases of tests/linear_es_cases.py meet the conditions that keep a bit-for-bit GPU pass honest -- checked on the CPU: the same
closed loop (the restated policy on the observation, a step, the restated ES rule) around 64 oracles stepped side by side, on
Philox streams keyed like the handles', over the three launches of the GPU test and the first group.  Seeds, scales and rates are
settled here, not on the GPU.

  the group ends at least 2 generations;
  a generation ends inside a launch, and one is open across a launch boundary;
  some member waits for an episode boundary (eps == -1) and some member runs a spare episode (eps == T) -- a ``near`` case: the
  oracle has no state setter, no env of these configs reaches the target from a reset state, every episode of the group ends at
  the same step and nobody waits: shown here; on the GPU the placed envs terminate early, which tests/test_gpu_linear_es.py
  asserts on what it ran;
  ranks tie in a generation (the sparse-reward case) and differ in a generation;
  a mean entry moves, and some mean or candidate entry differs between the rounded product-then-sum and a fused multiply-add.

The optimisation sanity case (linear_es_cases.OPT) is settled here too: it is deterministic."""
import warnings

import numpy as np
import pytest

import linear_es_cases as ec
import linear_es_ref as ler
import linear_policy_ref as ref
from mdp_playground_amd import mdp as mdp_mod
from test_linear_policy_cases_host import _oracle


def closed_loop(config, kw, state, *, seed, T, steps, launch_len=ec.K):
    """`state`: linear_es_ref.new_state(...) for ONE group (not yet initialised).  Returns (figures, the state after the run)."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = mdp_mod.build_mdp(dict(config))
    mode = kw.get("autoreset", "same_step")
    max_steps = kw.get("max_episode_steps") or 0
    n = ec.GROUP
    s = ler.init({k: v.copy() for k, v in state.items()}, seed=seed, env0=ec.OFF)
    envs = []
    for i in range(n):
        o = _oracle(m)
        o.set_philox(77, ec.OFF + i)
        envs.append(o)
    obs = np.stack([o.reset() for o in envs]).astype(np.float32)
    count, pending = np.zeros(n, int), np.zeros(n, bool)
    ended = np.zeros((steps, 1), bool)
    info = ler.new_info()
    for t in range(steps):
        act = ref.linear_actions(s["cand"], obs, m.action_space_max)
        fresh = np.zeros(n, bool)
        for i, o in enumerate(envs):
            if pending[i]:
                obs[i] = o.reset(explicit=False)
                count[i], pending[i] = 0, False
                continue
            info["waiting"] += int(s["eps"][i] == -1)
            info["spare"] += int(s["eps"][i] == T)
            info["steps"] += 1
            obs[i], r, _, d = o.step(act[i])
            count[i] += 1
            end = bool(d) or (bool(max_steps) and count[i] >= max_steps)
            ler.observe(s, i, np.float32(r), end, T)
            fresh[i] = end
            if end and mode == "same_step":
                obs[i] = o.reset(explicit=False)
                count[i] = 0
            elif end and mode == "next_step":
                pending[i] = True
        ended[t, 0] = ler.vote(s, 0, fresh, seed=seed, env0=ec.OFF, T=T, info=info)
    return ec.figures(ended, s["gen"], info, launch_len), s


def case_loop(name):
    c = ec.CASES[name]
    state = ler.new_state(ec.mean_of(name, 1), ec.sigma_of(name, 1), ec.lr_of(name, 1), ec.ROWS)
    return closed_loop(c["config"], c["kw"], state, seed=ec.SEED, T=c["T"], steps=ec.K * ec.LAUNCHES)


@pytest.mark.parametrize("name", sorted(ec.CASES))
def test_case_meets_its_conditions_on_the_oracle(name):
    fig, s = case_loop(name)
    print(name, fig)
    ec.assert_figures(name, fig, staggered=not ec.CASES[name]["near"])
    assert np.isfinite(s["mean"]).all() and np.isfinite(s["fitness"]).all()


def test_the_strategy_optimises_on_the_dense_reward():
    o = ec.OPT
    c = ec.lc.CASES[o["base"]]
    D = c["D"]
    state = ler.new_state(np.zeros((1, D, D + 1), np.float32), o["sigma"], o["lr"], o["rows"])
    fig, s = closed_loop(c["config"], dict(c["kw"], max_episode_steps=o["limit"]), state, seed=o["seed"], T=o["T"], steps=o["steps"])
    curve = s["log_mean"][:, 0]
    print(fig, curve.tolist())
    assert s["gen"][0] >= o["rows"] >= 10
    assert curve[-5:].mean() > curve[:5].mean()


def test_cases_cover_what_the_gpu_test_needs():
    assert (ec.N, ec.K, ec.LAUNCHES, ec.G) == (320, 37, 3, 5) and ec.RNGS == ("numpy", "philox")
    cs = ec.CASES
    assert len(cs) >= 8
    assert cs["c_d2_n0"]["config"]["make_denser"] and any(c["ties"] and not c["config"]["make_denser"] for c in cs.values())
    assert {c["D"] for c in cs.values()} >= {2, 3, 4, 12} and cs["cfg3"]["near"] and cs["cfg5_T2"]["near"]
    assert cs["cfg5_T2"]["plds"] == 0 and cs["cfg3"]["plds"] is None and cs["c_d2_n0_no_lds_T2"]["opts"] == ("NO_LINEAR_LDS",)
    assert {c["kw"].get("autoreset", "same_step") for c in cs.values()} == {"same_step", "next_step", "disabled"}
    assert cs["d4_delay3_every2_alw"]["config"]["delay"] == 3
    assert any(c["config"].get("reward_noise") or c["config"].get("transition_noise") for c in cs.values())
    assert {c["T"] for c in cs.values()} >= {1, 2}
    for name, c in cs.items():
        assert c["kw"]["max_episode_steps"] > 0, name
    assert len(set(ec.sigma_of("c_d2_n0").tolist())) == ec.G and len(set(ler.gain_of(ec.sigma_of("c_d2_n0"), ec.lr_of("c_d2_n0")).tolist())) == ec.G
