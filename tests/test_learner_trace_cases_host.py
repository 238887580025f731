"""The cases of tests/test_gpu_learn_traces.py on the host (no GPU): every case runs as a CPU closed loop -- 32 oracle envs on
Philox streams driven by the restatement tests/learner_trace_ref.py, K = 37, two launches -- and must meet the conditions
that keep a GPU pass honest (tests/learner_trace_cases.py honest()): a cut and a step without one for q_learning, a trace
above 1 for accumulating traces, episode ends inside a launch, Z non-zero at every launch boundary, a carried action and one
that differs from a fresh selection for sarsa, explored steps between 5 % and 95 %.

The delay = 4 learning-quality case: q_learning with replacing traces on the S = A = 8, delay = 4 env, 32 envs x 1 200 steps
from zero tables, lambda = 0 against lambda = 0.8, all else equal (nothing tuned: the cases' own ALPHA, GAMMA, EPS, LAMBDA).
Measured mean reward per step over all envs and steps (seeded, so reproducible; max_episode_steps = 20, same-step autoreset):
    lambda = 0      0.04604   (second half of the run: 0.07396)
    lambda = 0.8    0.10758   (second half of the run: 0.16250)
lambda > 0 wins by 0.06154; test_delay_4_with_and_without_traces asserts half that margin, 0.03077."""
import numpy as np
import pytest

import learner_trace_cases as cases
import learner_trace_ref as tref

N_CPU = 32


# (the CPU closed loop runs Philox streams: a case and its numpy-stream twin are one case here)
@pytest.mark.parametrize("handle,algo,kind,form", sorted({(h, a, k, f) for h, a, k, _, f in cases.all_cases()}))
def test_every_gpu_case_meets_its_coverage_conditions_on_the_cpu(handle, algo, kind, form):
    cfg, kw = cases.HANDLES[handle]
    al, ga, ep, lam = cases.params(form, N_CPU)
    agent, traj = cases.closed_loop(cfg, kw, algo, kind, al, ga, ep, lam, N_CPU)
    assert traj["actions"].shape == (cases.LAUNCHES * cases.K, N_CPU)
    cases.honest(handle, algo, kind, agent.info, cases.LAUNCHES)
    assert (agent.Q != 0).any()


def _mean_reward(lam):
    cfg, kw = cases.DELAY_CASE
    agent, traj = cases.closed_loop(cfg, kw, "q_learning", tref.REPLACING, cases.ALPHA, cases.GAMMA, cases.EPS, lam, cases.DELAY_ENVS,
                                    K=cases.DELAY_STEPS, launches=1)
    live = ~traj["reset_call"]
    return float(traj["reward"].sum() / live.sum())


def test_delay_4_with_and_without_traces():
    """the one-step learner credits a delayed reward to the wrong (s, a); the trace reaches back to the one that earned it"""
    r0, r1 = _mean_reward(0.0), _mean_reward(cases.DELAY_LAMBDA)
    print("delay = 4: mean reward per step, lambda = 0: %.5f, lambda = %.1f: %.5f" % (r0, cases.DELAY_LAMBDA, r1))
    assert r1 - r0 >= 0.03077, (r0, r1)
