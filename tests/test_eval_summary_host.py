"""Greedy evaluation and episode summaries on the host (no GPU): the restatement tests/eval_summary_ref.py on ties and on short
sequences worked out by hand, EpisodeSummary's pop() / clear() on CPU tensors, the restated per-env counts against the host
path of stats_csv.EpisodeStats, the names of the C ABI, and a CPU closed loop (the oracle env driven by the restatement, 32
envs, the GPU test's K, two launches) showing that what tests/test_gpu_eval_summary.py asserts about its own coverage can be
met by every handle it uses."""
import os
import re

import numpy as np
import pytest

import eval_summary_cases as cases
import eval_summary_ref as ref
import learner_sweep_ref as learn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- (a) greedy selection by hand
def test_greedy_takes_the_lowest_index_among_ties_and_the_strict_maximum_otherwise():
    Q = np.zeros((4, 2, 3), np.float32)
    Q[0, 1] = [0.5, 2.0, 2.0]        # tie between 1 and 2 -> 1
    Q[1, 1] = [-1.0, -3.0, -0.5]     # strict -> 2
    Q[2, 1] = [0.0, 0.0, 0.0]        # all equal -> 0
    Q[3, 0] = [9.0, 0.0, 0.0]        # (row 0: not the state asked for)
    Q[3, 1] = [1.0, 3.0, 2.0]        # strict -> 1
    info = ref.new_info()
    a = ref.greedy(Q, np.array([1, 1, 1, 1]), info)
    assert a.tolist() == [1, 2, 0, 1] and a.dtype == np.int64
    assert info["greedy_ties"] == 2 and info["greedy_strict"] == 2 and info["sum_differs"] == 0
    # live: only those envs are counted
    info = ref.new_info()
    ref.greedy(Q, np.array([1, 1, 1, 1]), info, np.array([True, False, False, True]))
    assert info["greedy_ties"] == 1 and info["greedy_strict"] == 1


def test_double_q_greedy_is_the_argmax_of_the_float32_sum_of_the_two_tables():
    Q = np.zeros((4, 2, 2, 2), np.float32)
    Q[0, 0, 0], Q[0, 1, 0] = [1.0, 0.0], [0.0, 1.0]          # sums [1, 1]: tie -> 0 although QB alone says 1
    Q[1, 0, 0], Q[1, 1, 0] = [0.0, 1.0], [1.0, 0.0]          # sums [1, 1]: tie -> 0 although QA alone says 1
    Q[2, 0, 0], Q[2, 1, 0] = [0.5, 0.25], [0.0, 0.5]         # sums [.5, .75] -> 1 although QA alone says 0
    # one float32 addition per entry: 2^24 + 1 is not a float32, so [2^24, 2^24] + [0, 1] ties and the lowest index wins
    Q[3, 0, 0], Q[3, 1, 0] = [2.0 ** 24, 2.0 ** 24], [0.0, 1.0]
    info = ref.new_info()
    a = ref.greedy(Q, np.zeros(4, np.int64), info)
    assert a.tolist() == [0, 0, 1, 0]
    assert info["greedy_ties"] == 3 and info["greedy_strict"] == 1 and info["sum_differs"] == 2
    # the same through the learner's restatement with a word that never explores
    never = np.full(4, 0xFFFFFFFF, np.uint32)
    assert learn.select("double_q", Q, np.zeros(4, np.int64), never, never, np.zeros(4, np.int64))[0].tolist() == a.tolist()


def test_eval_run_selects_on_a_reset_call_from_the_recorded_state_and_counts_it():
    Q = np.zeros((2, 3, 2), np.float32)
    Q[:, 1] = [0.0, 1.0]
    obs = np.array([[1, 2], [0, 1], [1, 1]])
    term = np.array([[0, 1], [0, 0], [0, 0]], bool)
    act, rc, pend, info = ref.eval_run(Q, np.array([0, 1]), obs, term, np.zeros_like(term), ref.NEXT_STEP)
    # env 1: step 0 terminates in state 2; step 1 is its reset call (selected from state 2: all-zero row -> 0); then state 1 -> 1
    assert act.tolist() == [[0, 1], [1, 0], [0, 1]]
    assert rc.tolist() == [[False, False], [False, True], [False, False]] and not pend.any()
    assert info["reset_calls"] == 1 and info["terminations"] == 1
    assert info["greedy_strict"] + info["greedy_ties"] == 5
    rc2, pend2 = ref.reset_calls(term, np.zeros_like(term), ref.NEXT_STEP)
    assert np.array_equal(rc2, rc) and not pend2.any()
    assert not ref.reset_calls(term, np.zeros_like(term), ref.SAME_STEP)[0].any()


# ---- (b) the summary rule by hand
def _f32(*rows):
    return np.array(rows, np.float32)


def test_summary_rule_by_hand_terminated_truncated_a_skipped_reset_call_and_an_episode_across_two_launches():
    # env 0: r = 1, 2 (terminated) | 0.5, 0.25, 4 (truncated) | 8 ...            -> launch 2: 16 (terminated)
    # env 1: r = 1 (terminated) | reset call (its row is skipped) | 2, 3, 0     -> launch 2: 5, then 7 (truncated)
    rew = _f32([1, 1], [2, 0], [0.5, 2], [0.25, 3], [4, 0], [8, 0])
    term = np.array([[0, 1], [1, 0], [0, 0], [0, 0], [0, 0], [0, 0]], bool)
    trunc = np.array([[0, 0], [0, 0], [0, 0], [0, 0], [1, 0], [0, 0]], bool)
    rc = np.array([[0, 0], [0, 1], [0, 0], [0, 0], [0, 0], [0, 0]], bool)
    rew[5, 1], rc[5, 1] = 100.0, True          # (a reset call's row never counts, whatever it holds)
    c = ref.new_counters()
    st = ref.summary(rew, term, trunc, rc, ref.new_state5(2), c)
    assert st["episodes"].tolist() == [2, 1] and st["length_sum"].tolist() == [5, 1]
    assert st["return_sum"].tolist() == [3.0 + 4.75, 1.0]
    assert st["ret"].tolist() == [8.0, 5.0] and st["len"].tolist() == [1, 3]
    assert c == dict(two_in_one_launch=1, spans_boundary=0, ended_terminated=2, ended_truncated=1, reset_calls=2)
    for name, dt in ref.FIELDS:
        assert st[name].dtype == dt
    # pop between the launches: the three sums leave, the running pair carries on
    (ep, rs, ls), st = ref.pop(st)
    assert ep.tolist() == [2, 1] and rs.tolist() == [7.75, 1.0] and ls.tolist() == [5, 1]
    assert st["episodes"].tolist() == [0, 0] and st["ret"].tolist() == [8.0, 5.0] and st["len"].tolist() == [1, 3]
    st2 = ref.summary(_f32([16, 5], [0, 7]), np.array([[1, 0], [0, 0]], bool), np.array([[0, 0], [0, 1]], bool), np.zeros((2, 2), bool), st, c)
    assert st2["episodes"].tolist() == [1, 1] and st2["return_sum"].tolist() == [24.0, 17.0] and st2["length_sum"].tolist() == [2, 5]
    assert st2["ret"].tolist() == [0.0, 0.0] and st2["len"].tolist() == [1, 0]
    assert c["spans_boundary"] == 2 and c["two_in_one_launch"] == 1
    assert st["len"].tolist() == [1, 3]          # (the state handed in is not modified)


def test_summary_adds_float32_rewards_in_float64():
    # 2^24 + 1 + 1: in float32 the ones are lost one by one, in float64 they are not
    rew = _f32([2.0 ** 24], [1], [1])
    z = np.zeros((3, 1), bool)
    st = ref.summary(rew, np.array([[0], [0], [1]], bool), z, z, ref.new_state5(1))
    assert st["return_sum"].tolist() == [2.0 ** 24 + 2.0] and st["return_sum"].dtype == np.float64
    # terminated and truncated on the same step: one episode
    st = ref.summary(_f32([1]), np.ones((1, 1), bool), np.ones((1, 1), bool), np.zeros((1, 1), bool), ref.new_state5(1))
    assert st["episodes"].tolist() == [1] and st["length_sum"].tolist() == [1]


def test_episode_summary_pop_and_clear_on_cpu_tensors():
    import torch
    from mdp_playground_amd.summary import EpisodeSummary
    s = EpisodeSummary(3, "cpu")
    assert [t.dtype for t in s.tensors()] == [torch.float64, torch.int32, torch.int32, torch.float64, torch.int32]
    assert all(tuple(t.shape) == (3,) and not t.any() for t in s.tensors())
    assert [t is x for t, x in zip(s.tensors(), (s.ret, s.len, s.episodes, s.return_sum, s.length_sum))] == [True] * 5
    s.ret += 1.5; s.len += 2; s.episodes += 3; s.return_sum += 4.5; s.length_sum += 6
    ep, rs, ls = s.pop()
    assert ep.tolist() == [3] * 3 and rs.tolist() == [4.5] * 3 and ls.tolist() == [6] * 3
    assert not s.episodes.any() and not s.return_sum.any() and not s.length_sum.any()
    assert s.ret.tolist() == [1.5] * 3 and s.len.tolist() == [2] * 3          # the running episode carries on
    s.episodes += 1
    assert ep.tolist() == [3] * 3                                             # (clones)
    s.clear()
    assert all(not t.any() for t in s.tensors())
    s.check(3, torch.device("cpu"), "t")
    for bad in (lambda: s.check(4, torch.device("cpu"), "t"), lambda: s.check(3, torch.device("meta"), "t")):
        with pytest.raises(ValueError):
            bad()
    s.len = s.len.to(torch.int64)
    with pytest.raises(ValueError, match="summary.len"):
        s.check(3, torch.device("cpu"), "t")


# ---- (c) against the host path of stats_csv.EpisodeStats
def test_restated_counts_add_up_to_what_episode_stats_reports_on_same_step_arrays():
    import torch
    from mdp_playground_amd.stats_csv import EpisodeStats
    rs = np.random.default_rng(3)
    n, K = 13, 29
    st, stats = ref.new_state5(n), EpisodeStats(n, "cpu")
    for launch in range(2):
        rew = rs.normal(size=(K, n)).astype(np.float32)
        term, trunc = rs.random((K, n)) < 0.1, rs.random((K, n)) < 0.07
        st = ref.summary(rew, term, trunc, np.zeros((K, n), bool), st)
        (ep, ret_sum, ls), st = ref.pop(st)
        stats.update(torch.as_tensor(rew), torch.as_tensor(term), torch.as_tensor(trunc))
        count, sum_len, sum_ret = int(stats.count.item()), int(stats.sum_len.item()), float(stats.sum_ret.item())
        assert int(ep.sum()) == count > 10, launch                  # exactly
        assert int(ls.sum()) == sum_len, launch
        assert abs(float(ret_sum.sum()) - sum_ret) <= 1e-9 * max(1.0, abs(sum_ret))     # (float64 sums in another order)
        # the running pair is EpisodeStats's own, element for element
        assert np.array_equal(st["ret"], stats.ret.numpy()) and np.array_equal(st["len"], stats.len.numpy())
        t, mean_ret, mean_len = stats.pop()
        assert t == (launch + 1) * K * n and mean_len == sum_len / count


# ---- (d) names
def test_the_new_entry_points_are_declared_and_bound_and_the_units_are_built():
    from mdp_playground_amd import _capi, build
    src = open(os.path.join(ROOT, "include", "mdpp.h")).read()
    for name in ("mdpp_step_n_eval", "mdpp_eval_kernel_name", "mdpp_step_n_learn_summary", "mdpp_step_n_eval_summary", "mdpp_current_obs"):
        assert name in _capi.EXPORTS
        assert re.search(r"\b%s\s*\(" % name, src), name
    lib = _capi.load()
    assert len(lib.mdpp_step_n_eval.argtypes) == 8
    assert len(lib.mdpp_step_n_learn_summary.argtypes) == 8 and len(lib.mdpp_step_n_eval_summary.argtypes) == 8
    assert _capi.MDPP_ABI_VERSION == 8
    for unit, parent in (("mdpp_discrete_eval.hip", "mdpp_discrete_eval.hpp"), ("mdpp_discrete_eval_summary.hip", "mdpp_discrete_eval.hpp"),
                         ("mdpp_discrete_learn_summary.hip", "mdpp_discrete_learn.hpp"), ("mdpp_discrete_learn_pe_summary.hip", "mdpp_discrete_learn.hpp"),
                         ("mdpp_discrete_learn_double_summary.hip", "mdpp_discrete_learn.hpp"),
                         ("mdpp_discrete_learn_double_pe_summary.hip", "mdpp_discrete_learn.hpp")):
        assert unit in build.SOURCES
        assert build.INCLUDED_SOURCES.get(unit) == ([parent] if parent else None)


# ---- (e) the coverage the GPU test asserts can be met: a closed loop on the CPU
def _closed_loop(cfg, kw, algo, n, q0):
    """n oracle envs (Philox streams; same-step / next-step / no autoreset as the handle) for LAUNCHES x K steps, driven by
    greedy evaluation of q0 (algo None, or "eval:double_q" for two tables) or by the learner's restatement (algo of
    learner_sweep_ref.ALGOS, from q0).  Returns (reward, terminated, truncated, reset_call) [T, n] and the evaluation's info."""
    from oracle import oracle as ora
    from mdp_playground_amd import mdp as mdp_mod
    m = mdp_mod.build_mdp(dict(cfg))
    autoreset, max_steps = kw.get("autoreset", ref.SAME_STEP), kw.get("max_episode_steps", 0)
    envs = []
    for i in range(n):
        o = ora.DiscreteOracle(m.S, m.A, m.sequence_length, m.delay, m.reward_every_n_steps, m.P, m.reward_table(), m.terminal_states,
                               m.init_dist, m.transition_noise, m.reward_noise, m.reward_scale, m.reward_shift, m.term_state_reward)
        o.set_philox(77, i)
        envs.append(o)
    s = np.array([o.reset() for o in envs], np.int64)
    evaluating = algo is None or algo.startswith("eval")
    Q = q0.copy()
    total = cases.LAUNCHES * cases.K
    if not evaluating:
        al, ga, E = learn.per_env(n, cases.ALPHA, cases.GAMMA, cases.EPS)
        w = {st: learn.tick_words(cases.SEED, 0, 0, total + 1, n, st) for st in (learn.EXPLORE_STREAM, learn.ACTION_STREAM, learn.UPDATE_STREAM)}
    pending, steps = np.zeros(n, bool), np.zeros(n, np.int64)
    have_carry, carry = np.zeros(n, bool), np.zeros(n, np.int64)
    info = ref.new_info()
    R, TE, TR, RC = np.zeros((total, n), np.float32), np.zeros((total, n), bool), np.zeros((total, n), bool), np.zeros((total, n), bool)
    for t in range(total):
        live = ~pending
        if evaluating:
            a = ref.greedy(Q, s, info, live)
        else:
            if t % cases.K == 0:
                have_carry[:] = False
            fresh, _ = learn.select(algo, Q, s, w[learn.EXPLORE_STREAM][t], w[learn.ACTION_STREAM][t], E)
            a = np.where(have_carry, carry, fresh)
        s2, r, te = s.copy(), np.zeros(n, np.float32), np.zeros(n, bool)
        for i in np.flatnonzero(live):
            o, rr, d = envs[i].step(int(a[i]))
            s2[i], r[i], te[i] = o, np.float32(rr), d
        steps[live] += 1
        tr = live & (max_steps > 0) & (steps >= max_steps)
        if not evaluating:
            a2 = learn.select(algo, Q, s2, w[learn.EXPLORE_STREAM][t + 1], w[learn.ACTION_STREAM][t + 1], E)[0] if algo == "sarsa" else None
            learn.update(algo, Q, s, a, r, s2, te, live, al, ga, w[learn.UPDATE_STREAM][t], a2)
            have_carry = live & (algo == "sarsa") & ~te & ~(tr & (autoreset != ref.DISABLED))
            carry = a2 if a2 is not None else carry
        R[t], TE[t], TR[t], RC[t] = r, te, tr, pending
        info["terminations"] += int(te.sum())
        info["reset_calls"] += int(pending.sum())
        ended = live & (te | tr)
        for i in np.flatnonzero(pending | (ended & (autoreset == ref.SAME_STEP))):
            s2[i] = envs[i].reset(explicit=False)
            steps[i] = 0
        pending = ended & (autoreset == ref.NEXT_STEP)
        s = s2
    return (R, TE, TR, RC), info


def _tables(cfg, n, double):
    return cases.tie_q(cases.random_q(cases.Q_SEED, n, cfg["state_space_size"], cfg["action_space_size"], double))


@pytest.mark.parametrize("algo", cases.EVAL_ALGOS)
@pytest.mark.parametrize("case", list(cases.EVAL_CASES))
def test_cpu_closed_loop_meets_the_evaluation_coverage_the_gpu_test_asserts(case, algo):
    cfg, kw = cases.EVAL_CASES[case]
    double = algo == "double_q"
    _, info = _closed_loop(cfg, kw, "eval:" + algo, 32, _tables(cfg, 32, double))
    print(case, algo, info)
    cases.eval_honest(info, double)


@pytest.mark.parametrize("algo", cases.SUMMARY_ALGOS + ("eval",))
@pytest.mark.parametrize("case", list(cases.SUMMARY_CASES))
def test_cpu_closed_loop_meets_the_summary_coverage_the_gpu_test_asserts(case, algo):
    cfg, kw = cases.SUMMARY_CASES[case]
    q0 = _tables(cfg, 32, algo == "double_q")
    (R, TE, TR, RC), _ = _closed_loop(cfg, kw, None if algo == "eval" else algo, 32, q0)
    st, c, total = ref.new_state5(32), ref.new_counters(), np.zeros(32)
    for launch in range(cases.LAUNCHES):
        sl = slice(launch * cases.K, (launch + 1) * cases.K)
        st = ref.summary(R[sl], TE[sl], TR[sl], RC[sl], st, c)
        (_, rs, _), st = ref.pop(st)
        total += rs
    print(case, algo, c)
    cases.summary_honest(c, total, case, algo)
    if kw.get("autoreset") != ref.NEXT_STEP:
        assert c["reset_calls"] == 0
