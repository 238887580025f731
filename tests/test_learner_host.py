"""In-kernel tabular learners on the host (no GPU): the helpers of mdp_playground_amd.policy, parameter validation, the C ABI
names, and the numpy restatement tests/learner_ref.py itself against updates worked out by hand on a 3-state chain
(alpha = gamma = 0.5: every figure below is exact in float32)."""
import os
import re

import numpy as np
import pytest

import learner_ref as ref
from mdp_playground_amd import _capi
from mdp_playground_amd import policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO31 = 2 ** 31
GREEDY, EXPLORE = 0xFFFFFFFF, 0          # explore words: (w >> 1) >= E for every E <= 2^31 - 1 / < E for every E >= 1
LEARN_EXPORTS = ("mdpp_set_learner", "mdpp_clear_learner", "mdpp_set_learner_rates", "mdpp_step_n_learn", "mdpp_get_q",
                 "mdpp_set_q", "mdpp_learn_kernel_name")


def test_epsilon_threshold_known_answers_and_monotone():
    assert policy.epsilon_threshold(0.0) == 0
    assert policy.epsilon_threshold(1.0) == TWO31
    assert policy.epsilon_threshold(0.25) == 2 ** 29
    # epsilon travels as a float32: 0.1f = 0x3DCCCCCD = 13421773 2^-27, times 2^31 an integer
    assert policy.epsilon_threshold(0.1) == 13421773 * 16
    assert policy.epsilon_threshold(1e-3) == int(np.ceil(float(np.float32(1e-3)) * TWO31))
    es = [policy.epsilon_threshold(e) for e in np.linspace(0.0, 1.0, 257)]
    assert all(b >= a for a, b in zip(es, es[1:])) and es[0] == 0 and es[-1] == TWO31
    # the restatement's own
    for e in (0.0, 1.0, 0.25, 0.1, 1e-3, 0.999):
        assert ref.epsilon_threshold(e) == policy.epsilon_threshold(e)
    # never / always: no 31-bit draw is below 0, every one is below 2^31
    m = np.array([0, 1, 0x7FFFFFFF], np.int64)
    assert not (m < policy.epsilon_threshold(0.0)).any() and (m < policy.epsilon_threshold(1.0)).all()


def test_explore_action_against_hand_computed_words():
    words = np.array([0, 0x1FFFFFFF, 0x20000000, 0x7FFFFFFF, 0x80000000, 0xDFFFFFFF, 0xE0000000, 0xFFFFFFFF], np.uint32)
    assert policy.explore_action(words, 8).tolist() == [0, 0, 1, 3, 4, 6, 7, 7]
    assert policy.explore_action(words, 1).tolist() == [0] * 8
    # A = 3: floor(3 w / 2^32); 0x55555555 * 3 = 0xFFFFFFFF (< 2^32), 0x55555556 * 3 = 2^32 + 2
    assert policy.explore_action(np.array([0x55555555, 0x55555556, 0xAAAAAAAA, 0xAAAAAAAB], np.uint32), 3).tolist() == [0, 1, 1, 2]
    assert int(policy.explore_action(0xFFFFFFFF, 20)) == 19
    # the restatement's selection uses the same rule when it explores
    Q = np.zeros((4, 2, 3), np.float32)
    a, x = ref.select(Q, np.zeros(4, np.int64), np.zeros(4, np.uint32), np.array([0x55555555, 0x55555556, 0xAAAAAAAA, 0xAAAAAAAB], np.uint32), 1)
    assert a.tolist() == [0, 1, 1, 2] and x.all()


@pytest.mark.parametrize("bad", [dict(alpha=0.0), dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=float("nan")), dict(gamma=-0.01),
                                 dict(gamma=1.01), dict(epsilon=-1e-3), dict(epsilon=1.1), dict(epsilon=float("nan")),
                                 dict(algo="double_q_learning"), dict(algo="Q")])
def test_parameter_validation(bad):
    kw = dict(algo="q_learning", alpha=0.3, gamma=0.9, epsilon=0.25)
    policy.check_learner_params(**kw)
    policy.check_learner_params("sarsa", 1.0, 0.0, 1.0)
    policy.check_learner_params("sarsa", 1e-3, 1.0, 0.0)
    kw.update(bad)
    with pytest.raises(ValueError):
        policy.check_learner_params(**kw)


def test_epsilon_threshold_rejects_values_outside_the_unit_interval():
    for e in (-0.5, 1.5, float("nan")):
        with pytest.raises(ValueError):
            policy.epsilon_threshold(e)


def _words(*rows):
    return np.array(rows, np.uint32).reshape(len(rows), 1)


P3 = np.array([[1, 0], [2, 0], [2, 2]])      # 0 -a0-> 1 -a0-> 2 (terminal); state 0 loops on action 1


def test_restatement_q_learning_by_hand_tie_explore_strict_and_terminated_target():
    """zeros; greedy tie -> 0; explore -> 1; strict maximum; explore -> 0 into the terminal state (y = r)"""
    w_e = _words(GREEDY, EXPLORE, GREEDY, EXPLORE, GREEDY)
    w_a = _words(0x12345678, 0x80000000, 0x9ABCDEF0, 0x7FFFFFFF, 0)
    obs = np.array([[1], [0], [1], [2]])
    rew = np.array([[1.0], [0.0], [1.0], [2.0]], np.float32)
    term = np.array([[0], [0], [0], [1]], bool)
    act, Q, pend, info = ref.run("q_learning", 0.5, 0.5, 0.25, np.zeros((1, 3, 2), np.float32), np.array([0]), obs, rew, term,
                                 np.zeros_like(term), P3, ref.DISABLED, w_e, w_a)
    assert act[:, 0].tolist() == [0, 1, 0, 0]
    # step 0: y = 1 + .5 * 0,      Q[0][0] = 0 + .5 * 1 = .5
    # step 1: y = 0 + .5 * .5,     Q[1][1] = 0 + .5 * .25 = .125
    # step 2: y = 1 + .5 * .125,   Q[0][0] = .5 + .5 * (1.0625 - .5) = .78125
    # step 3: terminated: y = 2,   Q[1][0] = 0 + .5 * 2 = 1
    assert Q.dtype == np.float32 and Q[0].tolist() == [[0.78125, 0.0], [1.0, 0.125], [0.0, 0.0]]
    assert not pend.any()
    assert info == dict(explored=2, greedy_ties=1, greedy_strict=1, carried=0, carried_differs=0, updates=4)


def _sarsa_case():
    Q0 = np.zeros((1, 3, 2), np.float32)
    Q0[0, 0] = [0.0, 1.0]
    obs = np.array([[0], [0], [1]])                       # twice round the loop 0 -a1-> 0, then 0 -a0-> 1
    rew = np.array([[-4.0], [8.0], [0.0]], np.float32)
    flags = np.zeros((3, 1), bool)
    return Q0, obs, rew, flags


def test_restatement_sarsa_by_hand_the_carry_and_its_drop_at_a_launch_boundary():
    Q0, obs, rew, flags = _sarsa_case()
    w_e, w_a = _words(GREEDY, GREEDY, GREEDY, GREEDY), _words(0, 0, 0, 0)
    # one launch of 3 steps
    act, Q, _, info = ref.run("sarsa", 0.5, 0.5, 0.25, Q0, np.array([0]), obs, rew, flags, flags, P3, ref.SAME_STEP, w_e, w_a)
    # step 0: a = 1 (strict);  a' = sel(0, 1) on Q BEFORE the update = 1;  y = -4 + .5 * 1 = -3.5;  Q[0][1] = 1 + .5 * (-4.5) = -1.25
    # step 1: takes the carried 1 although argmax Q[0] = [0, -1.25] is now 0;  a' = 0;  y = 8 + .5 * 0;  Q[0][1] = -1.25 + .5 * 9.25 = 3.375
    # step 2: takes the carried 0 although argmax Q[0] = [0, 3.375] is now 1;  s' = 1, a' = 0;  y = 0 + .5 * 0;  Q[0][0] = 0
    assert act[:, 0].tolist() == [1, 1, 0]
    assert Q[0, 0].tolist() == [0.0, 3.375]
    assert info["carried"] == 2 and info["carried_differs"] == 2
    # the same three steps as launches of 2 and 1: the second launch selects afresh -> action 1, not the carried 0
    act_a, Q_a, _, info_a = ref.run("sarsa", 0.5, 0.5, 0.25, Q0, np.array([0]), obs[:2], rew[:2], flags[:2], flags[:2], P3, ref.SAME_STEP,
                                    w_e[:3], w_a[:3])
    assert act_a[:, 0].tolist() == [1, 1] and Q_a[0, 0].tolist() == [0.0, 3.375] and info_a["carried"] == 1
    act_b, Q_b, _, info_b = ref.run("sarsa", 0.5, 0.5, 0.25, Q_a, np.array([0]), np.array([[0]]), rew[2:], flags[2:], flags[2:], P3,
                                    ref.SAME_STEP, w_e[2:], w_a[2:])
    assert act_b[:, 0].tolist() == [1] and info_b["carried"] == 0
    # a' = sel(0, 3) = 1 on [0, 3.375]: y = 0 + .5 * 3.375;  Q[0][1] = 3.375 + .5 * (1.6875 - 3.375) = 2.53125
    assert Q_b[0, 0].tolist() == [0.0, 2.53125]


def test_restatement_sarsa_the_carry_stops_at_a_termination_and_at_a_reset():
    Q0 = np.zeros((1, 3, 2), np.float32)
    Q0[0, 1] = [1.0, 0.0]
    w_e, w_a = _words(GREEDY, GREEDY, EXPLORE), _words(0, 0, 0xFFFFFFFF)
    obs = np.array([[0], [1]])                            # 1 -a0-> 2 terminal, same-step autoreset to 0; then 0 -a0-> 1
    rew = np.array([[2.0], [0.0]], np.float32)
    term = np.array([[1], [0]], bool)
    act, Q, _, info = ref.run("sarsa", 0.5, 0.5, 0.25, Q0, np.array([1]), obs, rew, term, np.zeros_like(term), P3, ref.SAME_STEP, w_e, w_a)
    # step 0: terminated: y = 2, Q[1][0] = 1 + .5 * 1 = 1.5, no carry;  step 1: fresh tie -> 0; a' = sel(1, 2) explores -> 1;
    # y = 0 + .5 * Q[1][1] = 0
    assert act[:, 0].tolist() == [0, 0] and info["carried"] == 0
    assert Q[0].tolist() == [[0.0, 0.0], [1.5, 0.0], [0.0, 0.0]]
    # truncated, not terminated, with an autoreset: the target bootstraps from s' = P[s][a], nothing is carried
    trunc = np.array([[1], [0]], bool)
    act, Q, _, info = ref.run("sarsa", 0.5, 0.5, 0.25, Q0, np.array([1]), np.array([[0], [1]]), rew, np.zeros_like(trunc), trunc, P3,
                              ref.SAME_STEP, _words(GREEDY, GREEDY, GREEDY), w_a)
    # step 0: s = 1, a = 0, s' = P[1][0] = 2 (obs shows the new episode's 0);  y = 2 + .5 * Q[2][0] = 2;  Q[1][0] = 1.5
    assert info["carried"] == 0 and Q[0, 1].tolist() == [1.5, 0.0]
    # the same without autoreset: the env goes on from s', so the action is carried
    _, _, _, info = ref.run("sarsa", 0.5, 0.5, 0.25, Q0, np.array([1]), np.array([[2], [2]]), rew, np.zeros_like(trunc), trunc, P3,
                            ref.DISABLED, _words(GREEDY, GREEDY, GREEDY), w_a)
    assert info["carried"] == 1


def test_restatement_next_step_reset_call_selects_an_action_and_learns_nothing():
    Q0 = np.zeros((2, 3, 2), np.float32)
    Q0[0, 1] = [0.0, 1.0]
    Q0[1, 1] = [1.0, 0.0]
    w_e = np.full((3, 2), GREEDY, np.uint32)
    w_a = np.zeros((3, 2), np.uint32)
    obs = np.array([[0, 2], [1, 0]])                      # env 0: its reset call, then a step; env 1: a terminating step, then its reset call
    rew = np.array([[0.0, 2.0], [1.0, 0.0]], np.float32)
    term = np.array([[0, 1], [0, 0]], bool)
    act, Q, pend, info = ref.run("q_learning", 0.5, 0.5, 0.25, Q0, np.array([1, 1]), obs, rew, term, np.zeros_like(term), P3,
                                 ref.NEXT_STEP, w_e, w_a, pending=np.array([True, False]))
    assert act.tolist() == [[1, 0], [0, 0]]               # (selected from the recorded state on the reset call too)
    assert info["updates"] == 2
    assert Q[0].tolist() == [[0.75, 0.0], [0.0, 1.0], [0.0, 0.0]]      # step 1: y = 1 + .5 * max Q[1] = 1.5
    assert Q[1].tolist() == [[0.0, 0.0], [1.5, 0.0], [0.0, 0.0]]       # step 0: terminated, y = 2: 1 + .5 * (2 - 1)
    assert pend.tolist() == [False, False]


def test_learner_entry_points_are_declared_and_bound():
    src = open(os.path.join(ROOT, "include", "mdpp.h")).read()
    for name in LEARN_EXPORTS:
        assert name in _capi.EXPORTS
        assert re.search(r"\b%s\s*\(" % name, src), name
    assert "MDPP_LEARN_Q_LEARNING = 0" in src and "MDPP_LEARN_SARSA = 1" in src
    assert _capi.LEARN_ALGOS == {"q_learning": 0, "sarsa": 1}
    assert "MDPP_OPT_NO_LEARN_LDS = 1u << 18" in src and _capi.OPTIONS["NO_LEARN_LDS"] == 1 << 18
    lib = _capi.load()
    assert len(lib.mdpp_set_learner.argtypes) == 8 and len(lib.mdpp_step_n_learn.argtypes) == 8
    assert len(lib.mdpp_set_learner_rates.argtypes) == 3 and len(lib.mdpp_get_q.argtypes) == 3 and len(lib.mdpp_set_q.argtypes) == 3
    assert lib.mdpp_learn_kernel_name.restype is not None
    assert _capi.MDPP_ABI_VERSION == 8


def test_learner_streams_are_named_and_distinct_from_every_other_stream_id():
    src = open(os.path.join(ROOT, "mdp_playground_amd", "csrc", "mdpp_internal.hpp")).read()
    ids = {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr uint32_t (kPhilox\w+Stream) = (\d+);", src)}
    assert ids["kPhiloxLearnExploreStream"] == ref.EXPLORE_STREAM == 15
    assert ids["kPhiloxLearnActionStream"] == ref.ACTION_STREAM == 16
    assert len(set(ids.values())) == len(ids)
    assert not set(ids.values()) & {6, 7, 8}              # (the post-processor's)
