"""Per-episode epsilon / alpha schedules of the learners on the host (no GPU): policy.epsilon_decay and the thresholds by hand,
the refusals of policy.learner_schedule_arrays, the restatement tests/learner_schedule_ref.py against steps worked out by hand
on the 3-state chain of test_learner_host.py (alpha = gamma = 0.5 and powers of two: every figure is exact in float32), a CPU
closed loop (the oracle env driven by the restatement, 32 envs, K = 37, two launches) showing that what
tests/test_gpu_learn_schedule.py asserts about its own coverage can be met by every case it runs, and the names of the C ABI
and of the build."""
import os
import re

import numpy as np
import pytest

import learner_schedule_cases as cases
import learner_schedule_cpu as cpu
import learner_schedule_ref as sref
import learner_sweep_ref as ref
from mdp_playground_amd import _capi, build, policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GREEDY, EXPLORE = 0xFFFFFFFF, 0          # explore words: never below E <= 2^31 - 1 / below every E >= 1
P3 = np.array([[1, 0], [2, 0], [2, 2]])  # 0 -a0-> 1 -a0-> 2 (terminal); action 1 leads back to 0
N_CPU = 32


def _words(*rows):
    return np.array(rows, np.uint32).reshape(len(rows), 1)


def _col(*v, dtype=np.int64):
    return np.array(v, dtype).reshape(len(v), 1)


# ---- (a) the decay rows and the thresholds
def test_epsilon_decay_by_hand():
    assert policy.epsilon_decay("const", 0.25, 4).tolist() == [0.25] * 4
    lin = policy.epsilon_decay("linear", 1.0, 5)
    assert lin.dtype == np.float64 and lin.tolist() == [1.0, 0.75, 0.5, 0.25, 0.0]
    assert policy.epsilon_decay("linear", 0.5, 3, 0.25).tolist() == [0.5, 0.375, 0.25]
    log = policy.epsilon_decay("log", 0.5, 3, 0.125)             # 0.5 (1/4)^x, x = 0, 1/2, 1
    assert log.tolist() == [0.5, 0.25, 0.125]
    log = policy.epsilon_decay("log", 0.5, 6, 0.001)
    assert log[0] == 0.5 and log[-1] == 0.5 * (0.001 / 0.5) ** 1.0 and np.all(np.diff(log) < 0)
    assert log[2] == 0.5 * (0.001 / 0.5) ** (2.0 / 5.0)
    for kind in policy.DECAY_KINDS:                              # one episode: x = 0 / max(0, 1)
        assert policy.epsilon_decay(kind, 0.3, 1, 0.1).tolist() == [0.3]
    for bad in (("cosine", 1.0, 4), ("log", 0.5, 4), ("log", 0.0, 4, 0.1), ("linear", 1.0, 0), ("linear", 1.0, 2.5), ("const", np.nan, 3),
                ("linear", 1.0, 3, np.inf)):
        with pytest.raises(ValueError):
            policy.epsilon_decay(*bad)
    for m in (1, 6, 24):                                         # the rows the cases use are the product's, bit for bit
        for args in (("const", 0.25, m), ("linear", 1.0, m, 0.0), ("log", 0.5, m, 0.001), ("linear", 1.0, m, 0.1)):
            assert np.array_equal(policy.epsilon_decay(*args), cases.decay(*args))


def test_thresholds_of_a_table_by_hand():
    eps = np.array([[0.0, 1.0, 0.25, 2.0 ** -31], [1e-10, 0.5, 2.0 ** -32, 1.0 - 2.0 ** -24]])
    want = np.array([[0, 2 ** 31, 2 ** 29, 1], [1, 2 ** 30, 1, 2 ** 31 - 128]], np.int64)
    assert np.array_equal(policy.epsilon_threshold(eps).astype(np.int64), want)
    e32, _, _, R, M = policy.learner_schedule_arrays(epsilon=eps, row=[0, 1])
    assert (R, M) == (2, 4) and e32.dtype == np.float32
    assert np.array_equal(policy.epsilon_threshold(e32).astype(np.int64), want)
    assert np.array_equal(sref.Schedule(2, eps, None, [0, 1]).T, want)
    # float32 first: 0.1 is rounded to float32 before the float64 product
    assert int(policy.epsilon_threshold(np.array([0.1]))[0]) == int(np.ceil(np.float64(np.float32(0.1)) * 2.0 ** 31))


# ---- (b) validation
def test_learner_schedule_arrays_accepts():
    import torch
    eps, al, row, R, M = policy.learner_schedule_arrays(epsilon=[0.5, 0.25, 0.0], num_envs=7)
    assert eps.shape == (1, 3) and eps.dtype == np.float32 and al is None and row is None and (R, M) == (1, 3)
    t = torch.tensor([[0.5, 1.0], [0.25, 0.125]], dtype=torch.float64)
    eps, al, row, R, M = policy.learner_schedule_arrays(t, t, torch.tensor([0, 1, 1]), 3)
    assert al.dtype == np.float32 and np.array_equal(eps, al) and row.dtype == np.int32 and row.tolist() == [0, 1, 1] and (R, M) == (2, 2)
    assert policy.learner_schedule_arrays(alpha=[1.0], row=np.zeros(4, np.int64), num_envs=4)[2] is None       # R == 1: the row is implied
    big = np.full((2, 2 ** 21), 0.5, np.float32)
    assert policy.learner_schedule_arrays(epsilon=big, row=[0, 1], num_envs=2)[3:] == (2, 2 ** 21)


@pytest.mark.parametrize("bad", [
    dict(), dict(epsilon=np.zeros((2, 2, 2)), row=[0, 1]), dict(epsilon=np.zeros((1, 0))), dict(epsilon=np.zeros(0)), dict(epsilon=0.5),
    dict(epsilon=np.full((2, 2 ** 21 + 1), 0.5, np.float32), row=[0, 1]),
    dict(epsilon=[0.5, 1.5]), dict(epsilon=[-0.1]), dict(epsilon=[0.5, np.nan]), dict(epsilon=[True, False]), dict(epsilon=["a"]),
    dict(alpha=[0.5, 0.0]), dict(alpha=[1e-50]), dict(alpha=[np.nan]), dict(alpha=[1.0001]),
    dict(epsilon=np.zeros((2, 3)), alpha=np.ones((2, 4)), row=[0, 1]), dict(epsilon=np.zeros((2, 3)), alpha=np.ones(3), row=[0, 1]),
    dict(epsilon=np.zeros((2, 3))), dict(epsilon=np.zeros((2, 3)), row=[0.0, 1.0]), dict(epsilon=np.zeros((2, 3)), row=[0, 1, 1]),
    dict(epsilon=np.zeros((2, 3)), row=[0, 2]), dict(epsilon=np.zeros((2, 3)), row=[-1, 0]), dict(epsilon=np.zeros((2, 3)), row=[[0, 1]]),
    dict(epsilon=np.zeros(3), row=[0, 1]), dict(epsilon=np.zeros((2, 3)), row=[True, False]),
])
def test_learner_schedule_arrays_refuses(bad):
    with pytest.raises(ValueError):
        policy.learner_schedule_arrays(num_envs=2, **bad)


# ---- (c) the restatement, by hand
def _agent(algo, sched, autoreset, q=None, eps=0.0):
    Q = np.zeros((1, 3, 2), np.float32) if q is None else np.asarray(q, np.float32).reshape(1, 3, 2)
    return sref.Agent(algo, 1, 0.5, 0.5, eps, sched, Q, autoreset)


def test_hand_alpha_is_looked_up_after_the_update_and_the_last_entry_holds():
    """every step starts in state 1, takes the greedy action 0 into the terminal state 2 with reward 1 (same-step autoreset
    back to 1): q <- q + alpha (1 - q) with alpha = 1/2, 1/4, 1/8 and then 1/8 again"""
    ag = _agent("q_learning", sref.Schedule(1, None, [0.5, 0.25, 0.125]), ref.SAME_STEP)
    K = 4
    act = sref.run(ag, [1], _col(1, 1, 1, 1), _col(1, 1, 1, 1, dtype=np.float32), _col(1, 1, 1, 1, dtype=bool), _col(0, 0, 0, 0, dtype=bool),
                   P3, _words(*[GREEDY] * (K + 1)), _words(*[0] * (K + 1)))
    assert act[:, 0].tolist() == [0, 0, 0, 0]
    assert ag.Q[0, 1, 0] == np.float32(0.712890625) and ag.ep.tolist() == [4]      # .5, .625, .671875, .712890625
    assert ag.info["alpha_changes"] == 2 and ag.info["E_changes"] == 0
    # the first update used entry 0, not entry 1
    one = _agent("q_learning", sref.Schedule(1, None, [0.5, 0.25, 0.125]), ref.SAME_STEP)
    sref.run(one, [1], _col(1), _col(1, dtype=np.float32), _col(1, dtype=bool), _col(0, dtype=bool), P3, _words(GREEDY, GREEDY), _words(0, 0))
    assert one.Q[0, 1, 0] == np.float32(0.5) and one.ep.tolist() == [1]
    # a counter that starts beyond the table: the last entry from the first step on
    late = sref.Agent("q_learning", 1, 0.5, 0.5, 0.0, sref.Schedule(1, None, [0.5, 0.25, 0.125]), np.zeros((1, 3, 2), np.float32), ref.SAME_STEP, ep=[7])
    sref.run(late, [1], _col(1), _col(1, dtype=np.float32), _col(1, dtype=bool), _col(0, dtype=bool), P3, _words(GREEDY, GREEDY), _words(0, 0))
    assert late.Q[0, 1, 0] == np.float32(0.125) and late.ep.tolist() == [8]


def test_hand_sarsa_selects_its_next_action_under_the_old_epsilon_and_carries_it_over_the_boundary():
    """autoreset disabled, step 0 is truncated but not terminated: the counter moves from 0 (epsilon 0) to 1 (epsilon 1).
    a' = sel(1, t + 1) was made under epsilon 0 -- greedy, Q[1] = [0, 1]: action 1 -- although the word of tick t + 1 explores
    under epsilon 1 and would then pick action 0.  Step 1 takes the carried 1."""
    q = [[0, 0], [0, 1], [0, 0]]
    ag = _agent("sarsa", sref.Schedule(1, [0.0, 1.0]), ref.DISABLED, q)
    act = sref.run(ag, [0], _col(1, 0), _col(0, 0, dtype=np.float32), _col(0, 0, dtype=bool), _col(1, 1, dtype=bool), P3,
                   _words(GREEDY, EXPLORE, EXPLORE), _words(0, 0, 0))
    assert act[:, 0].tolist() == [0, 1]
    assert ag.info["carried_old_E"] == 1 and ag.info["carried_old_E_differs"] == 1
    # step 0: y = 0 + 1/2 Q[1][1] = 1/2, Q[0][0] = 0 + 1/2 (1/2 - 0) = 1/4
    assert ag.Q[0, 0, 0] == np.float32(0.25)
    # step 1 (s = 1, a = 1 -> 0): a'' = sel(0, t + 2) under epsilon 1 explores to 0; y = 1/2 Q[0][0] = 1/8; Q[1][1] = 1 + 1/2 (1/8 - 1)
    assert ag.Q[0, 1, 1] == np.float32(0.5625)
    assert ag.ep.tolist() == [2] and ag.info["E_changes"] == 1
    # q_learning on the same arrays selects afresh at step 1: it explores
    ql = _agent("q_learning", sref.Schedule(1, [0.0, 1.0]), ref.DISABLED, q)
    act = sref.run(ql, [0], _col(1, 2), _col(0, 0, dtype=np.float32), _col(0, 1, dtype=bool), _col(1, 1, dtype=bool), P3,
                   _words(GREEDY, EXPLORE, EXPLORE), _words(0, 0, 0))
    assert act[:, 0].tolist() == [0, 0] and ql.info["expl_last_env"].tolist() == [1] and ql.info["expl_before_env"].tolist() == [0]


def test_hand_a_reset_call_selects_with_the_current_epsilon_and_counts_nothing():
    """next-step autoreset: step 0 ends the episode (1 -a0-> 2, terminal): ep = 1, epsilon 1 from now on.  Step 1 is the reset
    call: it explores (word 0x80000000 -> action 1), the action is written and ignored, nothing is learnt or counted.
    Step 2 explores to action 0 from the start state 0."""
    ag = _agent("q_learning", sref.Schedule(1, [0.0, 1.0], [0.5, 0.25]), ref.NEXT_STEP)
    act = sref.run(ag, [1], _col(2, 0, 1), _col(1, 0, 0, dtype=np.float32), _col(1, 0, 0, dtype=bool), _col(0, 0, 0, dtype=bool), P3,
                   _words(GREEDY, GREEDY, GREEDY, GREEDY), _words(0, 0x80000000, 0, 0))
    assert act[:, 0].tolist() == [0, 1, 0]
    assert ag.ep.tolist() == [1] and ag.info["reset_calls"] == 1 and ag.info["updates"] == 2
    assert ag.Q[0, 1, 0] == np.float32(0.5)                      # step 0: y = 1, alpha entry 0
    # step 2 (0 -a0-> 1): y = 0 + 1/2 max Q[1] = 1/4, alpha entry 1: Q[0][0] = 0 + 1/4 (1/4 - 0); the reset call touched nothing
    assert ag.Q[0, 0, 0] == np.float32(0.0625) and ag.Q[0, 0, 1] == 0 and ag.Q[0, 1, 1] == 0 and ag.Q[0, 2].tolist() == [0.0, 0.0]
    assert not ag.pending.any()


def test_hand_the_counter_moves_at_every_step_once_truncated_stays_set():
    ag = _agent("q_learning", sref.Schedule(1, None, [0.5, 0.25, 0.125, 0.0625]), ref.DISABLED)
    K = 5
    sref.run(ag, [0], _col(1, 0, 1, 0, 1), _col(*[0] * K, dtype=np.float32), _col(*[0] * K, dtype=bool), _col(0, 0, 1, 1, 1, dtype=bool), P3,
             _words(*[GREEDY] * (K + 1)), _words(*[0] * (K + 1)))
    assert ag.ep.tolist() == [3] and ag.info["alpha_changes"] == 3


# ---- (d) the CPU closed loop meets every asserted counter of every case
@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("algo", cases.ALGOS)
@pytest.mark.parametrize("handle", list(cases.HANDLES))
def test_cpu_closed_loop_meets_the_asserted_counters(handle, algo, kind):
    cfg, kw, m = cases.HANDLES[handle]
    sched = cases.schedule(kind, m, N_CPU)
    ag, traj = cpu.closed_loop(cfg, kw, algo, cases.ALPHA, cases.GAMMA, cases.EPS, sched, N_CPU, seed=cases.SEED, K=cases.K, launches=cases.LAUNCHES)
    cases.honest(handle, algo, kind, m, ag.info, ag.ep, sched.row)
    # the counter is the number of steps that ended an episode and were no reset call
    ended = ((traj["terminated"] | traj["truncated"]) & ~traj["reset_call"]).sum(axis=0)
    assert np.array_equal(ag.ep, ended)
    if "transition_noise" in cfg:
        return
    # fed with the loop's own outputs, launch by launch, run() reproduces it (the way the GPU test uses the restatement)
    from mdp_playground_amd import mdp as mdp_mod
    P = np.asarray(mdp_mod.build_mdp(dict(cfg)).P)
    K = cases.K
    again = sref.Agent(algo, N_CPU, cases.ALPHA, cases.GAMMA, cases.EPS, sched, np.zeros_like(ag.Q), kw.get("autoreset", ref.SAME_STEP))
    before = traj["obs0"]
    for launch in range(cases.LAUNCHES):
        sl = slice(launch * K, (launch + 1) * K)
        w = [ref.tick_words(cases.SEED, 0, launch * K, K + 1, N_CPU, st) for st in (ref.EXPLORE_STREAM, ref.ACTION_STREAM, ref.UPDATE_STREAM)]
        act = sref.run(again, before, traj["obs"][sl], traj["reward"][sl], traj["terminated"][sl], traj["truncated"][sl], P, *w)
        assert np.array_equal(act, traj["actions"][sl]), (handle, algo, kind, launch)
        before = traj["obs"][sl][-1]
    assert np.array_equal(again.Q.view(np.int32), ag.Q.view(np.int32)) and np.array_equal(again.ep, ag.ep)


def test_a_constant_schedule_is_the_unscheduled_learner():
    cfg, kw, m = cases.HANDLES["cfg2"]
    sched = sref.Schedule(N_CPU, np.full((1, m), cases.EPS), np.full((1, m), cases.ALPHA))
    a, ta = cpu.closed_loop(cfg, kw, "sarsa", 0.7, cases.GAMMA, 0.9, sched, N_CPU, seed=cases.SEED, K=cases.K, launches=2)
    b, tb = cpu.closed_loop(cfg, kw, "sarsa", cases.ALPHA, cases.GAMMA, cases.EPS, None, N_CPU, seed=cases.SEED, K=cases.K, launches=2)
    assert np.array_equal(ta["actions"], tb["actions"]) and np.array_equal(a.Q.view(np.int32), b.Q.view(np.int32))
    assert a.info["E_changes"] == 0 and a.info["alpha_changes"] == 0 and np.array_equal(a.ep, b.ep)


def test_every_third_of_the_gpu_cases_schedules_each_kind():
    kinds = [cases.kind_of(h, a, r) for h in cases.HANDLES for a in cases.ALGOS for r in cases.RNGS]
    assert sorted(set(kinds)) == sorted(cases.KINDS) and all(kinds.count(k) == len(kinds) // 3 for k in cases.KINDS)
    assert cases.kind_of("cfg2_disabled_max5", "sarsa", "numpy") == "eps"      # (sarsa's carry across a boundary needs epsilon scheduled)


# ---- (e) names
SCHED_UNITS = ["mdpp_discrete_learn_pe_sched.hip", "mdpp_discrete_learn_pe_sched_summary.hip", "mdpp_discrete_learn_double_pe_sched.hip",
               "mdpp_discrete_learn_double_pe_sched_summary.hip"]
SCHED_EXPORTS = ["mdpp_set_learner_schedule", "mdpp_clear_learner_schedule", "mdpp_get_learner_episodes", "mdpp_set_learner_episodes"]


def test_the_c_abi_and_the_build_name_the_schedule():
    assert _capi.MDPP_ABI_VERSION == 8
    hdr = open(os.path.join(ROOT, "include", "mdpp.h")).read()
    assert re.search(r"#define\s+MDPP_ABI_VERSION\s+8\b", hdr)
    assert re.search(r"#define\s+MDPP_MAX_SCHEDULE_ENTRIES\s+\(1 << 22\)", hdr) and _capi.MAX_SCHEDULE_ENTRIES == policy.MAX_SCHEDULE_ENTRIES == 1 << 22
    for name in SCHED_EXPORTS:
        assert name in _capi.EXPORTS and re.search(r"\bint %s\(mdpp_env \*h" % name, hdr), name
    learn_hpp = open(os.path.join(build.CSRC, "mdpp_discrete_learn.hpp")).read()
    for unit in SCHED_UNITS:
        assert unit in build.SOURCES and build.INCLUDED_SOURCES[unit] == ["mdpp_discrete_learn.hpp"], unit
        src = open(os.path.join(build.CSRC, unit)).read()
        assert re.search(r"template int mdpp::launch_learn_form<true, (true|false), (true|false), false, true>", src), unit
        assert unit in learn_hpp
    assert len(set(build.SOURCES)) == len(build.SOURCES)
