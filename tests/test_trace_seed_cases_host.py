"""Eligibility traces on one MDP per env, on the host (no GPU): the cases of tests/test_gpu_trace_seeds.py as CPU closed loops
(tests/trace_seed_cases.py: 320 oracle envs, env i on the MDP of seed 100 + i and the Philox streams of id 1000 + i, driven by
tests/learner_trace_ref.py; K = 37, two launches), each held to learner_trace_cases.honest()'s conditions -- a cut and a step
without one for q_learning, a carried action and one that differs from a fresh selection for sarsa, a trace above 1 for
accumulating traces, episode ends inside a launch, Z non-zero at every launch boundary, 5 - 95 % explored -- so a GPU pass
has exercised them; the sweep schedule's case; the delay comparison across the seeds of the reference's sweep; and the
header, the binding and the exported name of mdpp_learner_traces_per_env_mdp.

The delay comparison: learner_trace_cases.DELAY_CASE's config (S = A = 8, delay = 4, sequence_length = 1, max_episode_steps =
20) without its seed, ONE set-up of 320 envs on seeds 0 ... 9 (32 each, env ids 0 ... 319), 1 200 steps from zero tables,
q_learning with replacing traces and the cases' own ALPHA, GAMMA, EPS (nothing tuned), lambda = 0 against lambda = 0.8.
Measured mean reward per step over all envs and steps (seeded, so reproducible):
    lambda = 0      0.13525
    lambda = 0.8    0.17617
lambda > 0 wins on 8 of the 10 MDPs and by 0.04092 overall; test_delay_4_across_seeds asserts half that margin, 0.02046."""
import os
import re

import numpy as np
import pytest

import learner_schedule_cases as scases
import learner_trace_cases as cases
import learner_trace_ref as tref
import per_env_mdp_cpu as pm
import trace_seed_cases as tsc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# (the CPU closed loop runs Philox streams: a case that the GPU runs on numpy streams is the same case here)
@pytest.mark.parametrize("handle,algo,kind,rng,form", tsc.all_cases())
def test_every_gpu_case_meets_its_coverage_conditions_on_the_cpu(handle, algo, kind, rng, form):
    cfg, kw = tsc.HANDLES[handle]
    al, ga, ep, lam = cases.params(form, tsc.N)
    agent, traj = tsc.closed_loop(cfg, kw, algo, kind, al, ga, ep, lam)
    assert traj["actions"].shape == (tsc.LAUNCHES * tsc.K, tsc.N)
    cases.honest(handle, algo, kind, agent.info, tsc.LAUNCHES)
    # both workgroups' lanes learn something, and the envs differ: no two of the 320 MDPs share a P
    nz = pm.nonzero_envs(agent.Q)
    assert nz[:256].any() and nz[256:].any()
    P = np.stack([np.asarray(m.P) for m in pm.build_mdps(cfg)])
    assert len({p.tobytes() for p in P}) == tsc.N


def test_the_cases_cover_the_cross():
    got = tsc.all_cases()
    assert len(got) == len(set(got)) == 5 * 2 * 2 + 3
    for h in tsc.MAIN:
        mine = [c for c in got if c[0] == h]
        assert {(a, k) for _, a, k, _, _ in mine} == {(a, k) for a in tsc.ALGOS for k in tsc.KINDS}
        assert {(r, f) for _, _, _, r, f in mine} == {(r, f) for r in tsc.RNGS for f in tsc.FORMS}
    assert {tsc.HANDLES[h][1].get("autoreset", "same_step") for h, _, _ in tsc.TRUNCATION} == {"same_step", "next_step", "disabled"}
    assert all(tsc.HANDLES[h][1]["max_episode_steps"] == 5 for h, _, _ in tsc.TRUNCATION)
    # philox cases exist among the main cross (the GPU test holds them to the CPU loop) for both algorithms
    assert {a for _, a, _, r, _ in got if r == "philox"} == set(tsc.ALGOS)


@pytest.mark.parametrize("algo,kind", [("q_learning", tref.ACCUMULATING), ("sarsa", tref.REPLACING)])
def test_the_sweep_schedule_case_changes_alpha_while_z_is_non_zero(algo, kind):
    cfg, kw = tsc.HANDLES[tsc.SCHED_HANDLE]
    sched = scases.schedule(tsc.SCHED_KIND, tsc.SCHED_M, tsc.N)
    agent, _ = tsc.closed_loop(cfg, kw, algo, kind, cases.ALPHA, cases.GAMMA, cases.EPS, cases.LAMBDA, sched=sched)
    info = agent.info
    assert info["alpha_changes"] > 0 and info["alpha_change_with_z"] > 0 and info["E_changes"] > 0, info
    assert (agent.ep >= tsc.SCHED_M).any() and (agent.ep < tsc.SCHED_M - 1).any(), (agent.ep.min(), agent.ep.max())
    assert info["ends"] > 0 and info["z_nonzero_at_launch_end"] == tsc.LAUNCHES


def _mean_reward(lam):
    agent, traj = tsc.closed_loop(tsc.DELAY_CFG, tsc.DELAY_KW, "q_learning", tref.REPLACING, cases.ALPHA, cases.GAMMA, cases.EPS, lam,
                                  tsc.DELAY_SEEDS, seed=cases.SEED, K=cases.DELAY_STEPS, launches=1, philox_seed=77, off=0)
    live = ~traj["reset_call"]
    return float(traj["reward"].sum() / live.sum())


def test_delay_4_across_seeds():
    """the benefit of traces under reward delay holds across the MDPs of the reference's seed sweep, in one handle-like set-up"""
    assert len(tsc.DELAY_SEEDS) == 320 and sorted(set(tsc.DELAY_SEEDS)) == list(range(10)) and "seed" not in tsc.DELAY_CFG
    r0, r1 = _mean_reward(0.0), _mean_reward(cases.DELAY_LAMBDA)
    print("delay = 4 on seeds 0 ... 9: mean reward per step, lambda = 0: %.5f, lambda = %.1f: %.5f" % (r0, cases.DELAY_LAMBDA, r1))
    assert r1 - r0 >= 0.02046, (r0, r1)


# ---- the header, the binding, the exported name, the build
def test_the_header_states_the_opt_in_and_the_abi_is_bound():
    from mdp_playground_amd import _capi, build
    src = open(os.path.join(ROOT, "include", "mdpp.h")).read()
    flat = re.sub(r"\s*\n \*\s*", " ", src)
    for text in ("Traces on one MDP per env: a lambda x seed sweep in one launch", "mdpp_learner_traces_per_env_mdp(h, on) sets a flag of the handle, off at creation",
                 "With it off every call returns exactly what it returns without the flag",
                 "together with the schedule of mdpp_learner_schedule_sweep, in either order",
                 "Still refused, with or without the flag and in both orders: double_q; per-env noise levels",
                 "the schedule of mdpp_learner_schedule_sweep on a handle with one shared MDP",
                 "{Q + Z, slots}, {Q + Z}, {slots}, {}",
                 "turning it off, or turning mdpp_learner_per_env_mdp off, on a handle with one MDP per env drops the traces",
                 "mdpp_set_learner and mdpp_clear_learner drop the traces as ever and leave the flag",
                 "a captured launch reads every env's table set, Q and Z from the handle's buffers at replay"):
        assert text in flat, text
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    proto = re.search(r"int mdpp_learner_traces_per_env_mdp\s*\(([^)]*)\)", code)
    assert proto and len(proto.group(1).split(",")) == 2
    assert "mdpp_learner_traces_per_env_mdp" in _capi.EXPORTS
    lib = _capi.load()
    assert len(lib.mdpp_learner_traces_per_env_mdp.argtypes) == 2
    assert lib.mdpp_learner_traces_per_env_mdp(None, 1) == -1
    assert _capi.MDPP_ABI_VERSION == 8 and "#define MDPP_ABI_VERSION 8" in src        # (an entry point was added, nothing moved)
    units = ["mdpp_discrete_lambda_pe_pm.hip", "mdpp_discrete_summary_lambda_pe_pm.hip", "mdpp_discrete_lambda_pe_pm_sched.hip",
             "mdpp_discrete_summary_lambda_pe_pm_sched.hip"]
    for u in units:
        assert u in build.SOURCES and u not in build.EXTRA_FLAGS and os.path.exists(os.path.join(build.CSRC, u)), u
        assert build.INCLUDED_SOURCES[u] == ["mdpp_discrete_trace.hpp", "mdpp_discrete_learn.hpp"], u
        assert "launch_trace_form_pm" in open(os.path.join(build.CSRC, u)).read()
    assert len(set(build.SOURCES)) == len(build.SOURCES)


def test_the_python_layer_refuses_a_shared_mdp_before_the_library_is_reached():
    """per_env_mdp=True on a handle with one shared MDP: a ValueError that needs neither a learner nor a device"""
    from mdp_playground_amd import vector_env

    class Shared:
        _per_env = False
    with pytest.raises(ValueError, match="per_env_mdp=True needs one MDP per env"):
        vector_env.RLToyVectorEnv.set_learner_traces(Shared(), 0.5, "replacing", per_env_mdp=True)
