"""The shape and edge cases of the closed-loop kernels on the host (no GPU): every condition that
tests/test_gpu_closed_loop_shapes.py asserts about its own coverage (tests/closed_loop_shape_cases.py) is met by the 32-env CPU
closed loop (tests/closed_loop_cpu.py: the oracle env driven by the restatement) with the seeds the cases module names; the
cases module's restatement of the LDS carve agrees with the MDPs mdp.build_mdp makes and decides who is refused; and the
restatements' explicit scan and truncation counters are checked by hand."""
import os
import re

import numpy as np
import pytest

import closed_loop_shape_cases as cases
import eval_summary_ref as eref
import learner_sweep_ref as ref
from closed_loop_cpu import closed_loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 32
RUN = dict(seed=cases.SEED, K=cases.K, launches=cases.LAUNCHES)
GREEDY = 0xFFFFFFFF


def _flow(case, cfg, traj):
    cases.flow_honest(case, cfg, traj["state"], traj["actions"], traj["reward"], traj["terminated"], traj["truncated"], traj["reset_call"])


# ---- (a) the learners' conditions
@pytest.mark.parametrize("algo", cases.ALGOS)
@pytest.mark.parametrize("case", list(cases.CASES))
def test_cpu_closed_loop_meets_the_learner_conditions(case, algo):
    cfg, kw = cases.CASES[case]
    q0 = cases.start_tables(case, N, algo == "double_q")
    info, Q, traj = closed_loop(cfg, kw, algo, cases.ALPHA, cases.GAMMA, cases.EPS, N, q0, **RUN)
    print(case, algo, {k: v for k, v in info.items() if not isinstance(v, np.ndarray)})
    cases.learner_honest(case, algo, info, Q, q0)
    _flow(case, cfg, traj)


@pytest.mark.parametrize("case", list(cases.CASES))
@pytest.mark.parametrize("algo", cases.ALGOS)
def test_cpu_closed_loop_meets_the_per_env_parameter_conditions(case, algo):
    cfg, kw = cases.CASES[case]
    al, ga, ep = cases.pe_arrays(N)
    info, _, _ = closed_loop(cfg, kw, algo, al, ga, ep, N, cases.start_tables(case, N, algo == "double_q"), **RUN)
    cases.pe_honest(info, ep)


def test_cpu_closed_loop_meets_the_conditions_of_the_predicted_case():
    name, cfg, kw = cases.PREDICTED_CASE
    for algo in cases.ALGOS:
        info, Q, traj = closed_loop(cfg, kw, algo, cases.ALPHA, cases.GAMMA, cases.EPS, cases.PREDICTED_N, None, **RUN)
        cut = traj["truncated"] & ~traj["terminated"]
        assert cut.any() and info["trunc_resets"] == cut.sum()
        # the state learn() saw at a truncation is not the observation returned (the next episode's first), and not P[s][a] either
        assert (traj["next_state"][cut] != traj["obs"][cut]).any()
        from mdp_playground_amd import mdp as mdp_mod
        P = np.asarray(mdp_mod.build_mdp(dict(cfg)).P)
        assert (traj["next_state"][cut] != P[traj["state"][cut], traj["actions"][cut]]).any()
        assert info["greedy_strict"] > 0 and info["greedy_ties"] > 0 and info["explored"] > 0
        assert (Q != 0).reshape(cases.PREDICTED_N, -1).any(axis=1).sum() > cases.PREDICTED_N // 2
        if algo == "sarsa":
            assert info["trunc_carry_differs"] > 0


@pytest.mark.parametrize("algo", cases.ALGOS)
@pytest.mark.parametrize("case", list(cases.FLOAT_EDGE_CASES))
def test_cpu_closed_loop_meets_the_float_edge_conditions(case, algo):
    cfg, kw = cases.FLOAT_EDGE_CASES[case]
    S, A = cases.shape_of(cfg)[:2]
    q0 = cases.float_edge_tables(3, N, S, A, algo == "double_q")
    info, Q, _ = closed_loop(cfg, kw, algo, cases.ALPHA, cases.GAMMA, cases.EPS, N, q0, **RUN)
    print(case, algo, {k: v for k, v in info.items() if not isinstance(v, np.ndarray)})
    cases.float_edge_honest(info)
    assert np.isnan(Q).any() and not np.isnan(q0).any()


# ---- (b) evaluation and summaries
def _eval_loop(case, double):
    cfg, kw = cases.CASES[case]
    info = eref.new_info()
    _, _, traj = closed_loop(cfg, kw, "double_q" if double else "q_learning", cases.ALPHA, cases.GAMMA, cases.EPS, N,
                             cases.eval_tables(cfg, N, double), greedy=lambda Q, s, live: eref.greedy(Q, s, info, live), **RUN)
    info["terminations"] = int(traj["terminated"].sum())
    info["reset_calls"] = int(traj["reset_call"].sum())
    return info, traj


@pytest.mark.parametrize("algo", cases.EVAL_ALGOS)
@pytest.mark.parametrize("case", list(cases.CASES))
def test_cpu_closed_loop_meets_the_evaluation_conditions(case, algo):
    info, traj = _eval_loop(case, algo == "double_q")
    print(case, algo, info)
    cases.eval_honest(case, info, algo == "double_q")
    if case in cases.DELAY_LINE:
        cases.delay_line_honest(cases.CASES[case][0], traj["reward"], traj["reset_call"])


@pytest.mark.parametrize("algo", cases.ALGOS + ("eval",))
@pytest.mark.parametrize("case", cases.SUMMARY_CASES)
def test_cpu_closed_loop_meets_the_summary_conditions(case, algo):
    cfg, kw = cases.CASES[case]
    if algo == "eval":
        _, traj = _eval_loop(case, False)
    else:
        _, _, traj = closed_loop(cfg, kw, algo, cases.ALPHA, cases.GAMMA, cases.EPS, N, cases.eval_tables(cfg, N, algo == "double_q"), **RUN)
    st, c, total = eref.new_state5(N), eref.new_counters(), np.zeros(N)
    for launch in range(cases.LAUNCHES):
        sl = slice(launch * cases.K, (launch + 1) * cases.K)
        st = eref.summary(traj["reward"][sl], traj["terminated"][sl], traj["truncated"][sl], traj["reset_call"][sl], st, c)
        (_, rs, _), st = eref.pop(st)
        total += rs
    print(case, algo, c)
    cases.summary_honest(c, total, case, algo)


# ---- (c) the cases module's view of the handles
def test_every_case_builds_and_has_the_shape_and_the_reward_form_the_cases_module_says():
    from mdp_playground_amd import mdp as mdp_mod
    for case, (cfg, kw) in list(cases.CASES.items()) + [(cases.PREDICTED_CASE[0], cases.PREDICTED_CASE[1:])]:
        m = mdp_mod.build_mdp(dict(cfg))
        S, A, L, keys, unit, noise = cases.shape_of(cfg)
        assert (m.S, m.A, m.sequence_length) == (S, A, L), case
        assert (m.reward_matrix is not None) == cfg.get("use_custom_mdp", False)
        is_unit = m.reward_matrix is None and m.delay <= 32 and all(v == 1.0 for k, v in m.rewardable_sequences.items() if len(k) == L)
        assert is_unit == unit == (case not in cases.NON_UNIT), case
        assert bool(m.transition_noise) == noise
        assert len(m.reward_table()) == keys
        if case == "a1_s3":
            assert len(m.terminal_states) == 0
    S, A = cases.shape_of(cases.CASES["s255_a85"][0])[:2]
    assert (S, A) == (255, 85)
    assert {cases.shape_of(cases.CASES[c][0])[2] for c in cases.LONG_L} == {4, 7}
    assert all(cases.shape_of(cases.CASES[c][0])[0] != cases.shape_of(cases.CASES[c][0])[1] for c in cases.RECT)


def test_the_carve_is_the_one_mdpp_create_makes_and_decides_the_refusals():
    src = open(os.path.join(ROOT, "mdp_playground_amd", "csrc", "mdpp_capi.hip")).read()
    for line in ("a.lds_P = off; off = align16(off + cfg->S * cfg->A);", "a.lds_term = off; off = align16(off + cfg->S);",
                 "a.lds_init = off; off = align16(off + cfg->S * 8);", "a.rew_in_lds = rew_bytes <= 48u * 1024u;",
                 "a.noise_in_lds = cfg->has_transition_noise && noise_bytes <= 32u * 1024u;"):
        assert line in src, line
    closed = open(os.path.join(ROOT, "mdp_playground_amd", "csrc", "mdpp_discrete_closed.hpp")).read()
    assert "constexpr size_t kZigLdsBytes = 3u * 256u * 8u;" in closed and "> 64u * 1024u" in closed
    assert re.search(r"policy_row_words\(int A\) \{ return A <= 8 \? 8u : \(uint32_t\)A; \}", open(os.path.join(ROOT, "mdp_playground_amd", "csrc", "mdpp_discrete_policy.hip")).read())
    # by hand: cfg2 -- P 64, flags 8 -> 16, cdf 64, 512 keys -> 64 bytes of bits
    assert cases.lds_bytes(cases.CFG2) == 64 + 16 + 64 + 64
    # d4_s24_a6: 144 + 32 + 192 + 16
    assert cases.lds_bytes(cases.CASES["d4_s24_a6"][0]) == 144 + 32 + 192 + 16
    assert cases.q_lds(cases.CASES["d4_s24_a6"][0], False) == 144 * 1024 and cases.q_lds(cases.CASES["custom_79x2_noise"][0], False) == 158 * 1024
    assert cases.lds_bytes(cases.CASES["s6_L7"][0]) > 34 * 1024 and cases.lds_bytes(cases.CASES["s8_L4_rdist"][0]) > 32 * 1024
    # the noise cdfs of 79 states (49 928 bytes) stay in global memory; those of 8 states are staged
    assert cases.lds_bytes(cases.CASES["custom_79x2_noise"][0]) == 160 + 80 + 640 + 1264
    assert cases.lds_bytes(cases.CASES["s8_noise_max5_next"][0]) == 64 + 16 + 64 + 16 + 512
    # who is refused: no case's learner; the policy on noise and where 255 rows of 85 words join the tables
    assert all(cases.learner_refused(cfg) is None for cfg, _ in cases.CASES.values())
    refused = {c: cases.policy_refused(cfg) for c, (cfg, _) in cases.CASES.items() if cases.policy_refused(cfg)}
    assert refused == {"custom_79x2_noise": "transition_noise", "s8_noise_max5_next": "transition_noise", "s255_a85": "64 KiB"}
    assert 4 * 255 * 85 == 86700
    # the QLDS decision at a limit of 160 KiB: which side each edge shape falls on is computed, not assumed
    lim = 160 * 1024
    assert cases.qlds_expected(cases.CASES["d4_s24_a6"][0], False, lim) and not cases.qlds_expected(cases.CASES["d4_s24_a6"][0], True, lim)
    edge = {k: cfg for k, (cfg, _) in cases.QLDS_EDGE.items()}
    # 53 x 3: 159 KiB of tables; the MDP's 160 + 64 + 432 + 1 280 bytes tip it over
    assert cases.q_lds(edge["custom_53x3"], False) == 159 * 1024 and cases.lds_bytes(edge["custom_53x3"]) == 1936
    assert 159 * 1024 + 24 <= lim < 159 * 1024 + 24 + 1936 and not cases.qlds_expected(edge["custom_53x3"], False, lim)
    # 75 x 2 with noise: 150 KiB + 2 048 + 6 144 fits;  78 x 2 with noise: 156 KiB + 2 112 fits, the ziggurat tables' 6 144 do not
    assert cases.lds_bytes(edge["custom_75x2_noise"]) == 2048 and cases.qlds_expected(edge["custom_75x2_noise"], False, lim)
    assert cases.lds_bytes(edge["custom_78x2_noise"]) == 2112 and cases.static_lds(edge["custom_78x2_noise"]) == 6144
    assert 156 * 1024 + 2112 <= lim < 156 * 1024 + 2112 + 6144 and not cases.qlds_expected(edge["custom_78x2_noise"], False, lim)
    assert not cases.qlds_expected(edge["custom_79x2_noise"], False, lim)
    assert cases.qlds_expected(cases.CFG2, True, lim) and not cases.qlds_expected(cases.CASES["s255_a85"][0], False, lim)


def test_every_learner_run_is_listed_and_every_case_runs_every_algorithm():
    for case in cases.CASES:
        for algo in cases.ALGOS:
            assert len(cases.STREAMS[case][algo]) >= 1
        assert any(len(cases.STREAMS[case][a]) == 2 for a in cases.ALGOS)
    assert len(cases.LEARN_RUNS) == sum(len(s) for c in cases.CASES for s in cases.STREAMS[c].values())
    assert set(cases.SUMMARY_CASES) <= set(cases.CASES) and set(cases.HANDOVER_CASES) <= set(cases.CASES)


# ---- (d) the restatements' scan and truncation counters, by hand
def test_scan_best_is_the_strict_greater_scan_not_argmax():
    nan, inf = np.float32("nan"), np.float32("inf")
    rows = np.array([[0.0, -0.0, 0.0], [-0.0, 0.0, -0.0], [nan, 5.0, 6.0], [1.0, nan, 2.0], [1.0, nan, 0.5], [-inf, -inf, -inf],
                     [1e-45, 1e-39, 0.0], [-1e-45, -0.0, 0.0], [inf, inf, 1.0]], np.float32)
    arg, best = ref.scan_best(rows)
    assert arg.tolist() == [0, 0, 0, 2, 0, 0, 1, 1, 0]       # (np.argmax would say 2 -> 0, 3 -> 1, 4 -> 1)
    assert np.isnan(best[2]) and best[3] == 2.0 and best[4] == 1.0
    assert np.signbit(best[1]) and not np.signbit(best[0]) and np.signbit(best[7])     # the value is the scanned entry's own
    assert np.argmax(rows[3]) == 1                           # the difference the scan is there for
    q = np.zeros((1, 1, 3), np.float32)
    q[0, 0] = rows[3]
    assert eref.greedy(q, np.zeros(1, np.int64)).tolist() == [2]
    info = ref.new_info(1)
    a, _ = ref.select("q_learning", q, np.zeros(1, np.int64), np.array([GREEDY], np.uint32), np.zeros(1, np.uint32), np.array([2 ** 29]), info)
    assert a.tolist() == [2] and info["greedy_strict"] == 1


def test_sarsa_truncation_counters_by_hand():
    """one env, same-step autoreset, truncated (not terminated) at step 0: the carry is dropped and step 1 selects afresh from
    the next episode's first state; next-step autoreset: step 1 is the reset call and selects from s' itself"""
    P = np.array([[1, 1], [0, 0]])
    Q0 = np.zeros((1, 2, 2), np.float32)
    Q0[0, 1] = [0.0, 1.0]            # greedy in state 1: action 1; in state 0: the tie's action 0
    w_e = np.full((3, 1), GREEDY, np.uint32)
    w_a = np.zeros((3, 1), np.uint32)
    obs = np.array([[0], [1]])       # step 0: 0 -> 1 truncated, reset to 0;  step 1: 0 -> 1
    rew = np.zeros((2, 1), np.float32)
    term = np.zeros((2, 1), bool)
    trunc = np.array([[True], [False]])
    act, _, _, info = ref.run("sarsa", 0.5, 0.5, 0.25, Q0, np.array([0]), obs, rew, term, trunc, P, ref.SAME_STEP, w_e, w_a)
    # a' = sel(1) = 1 is dropped; step 1 selects from state 0: action 0
    assert act[:, 0].tolist() == [0, 0] and info["trunc_resets"] == 1 and info["trunc_carry_differs"] == 1 and info["carried"] == 0
    act, _, pend, info = ref.run("sarsa", 0.5, 0.5, 0.25, Q0, np.array([0]), np.array([[1], [0]]), rew, term, trunc, P, ref.NEXT_STEP, w_e, w_a)
    assert act[:, 0].tolist() == [0, 1] and info["trunc_resets"] == 1 and info["trunc_carry_differs"] == 0 and not pend.any()
    act, _, _, info = ref.run("sarsa", 0.5, 0.5, 0.25, Q0, np.array([0]), np.array([[1], [0]]), rew, term, trunc, P, ref.DISABLED, w_e, w_a)
    assert act[:, 0].tolist() == [0, 1] and info["trunc_resets"] == 0 and info["carried"] == 1
