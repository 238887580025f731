"""The grid learners' schedules and episode log without a GPU: the plumbing of the new entry points (header section, exports,
bindings, methods, build units), the conditions that keep a GPU pass of tests/test_gpu_grid_schedule.py honest -- every case's
scheduled closed loop runs here on the CPU (tests/grid_schedule_ref.py), on the Philox streams the GPU test uses, and must meet
them by the restatement alone --, the two exact consequences of the log's text, and what a decaying epsilon buys on a sparse
gridworld."""
import os
import re

import numpy as np
import pytest

import episode_log_ref as lref
import grid_learner_cases as gc
import grid_learner_ref as gref
import grid_schedule_cases as gsc
import grid_schedule_ref as gsr
import learner_schedule_ref as sref

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW_SYMBOLS = ("mdpp_set_grid_learner_schedule", "mdpp_clear_grid_learner_schedule", "mdpp_get_grid_learner_episodes",
               "mdpp_set_grid_learner_episodes", "mdpp_step_n_grid_learn_log")
NEW_UNITS = ("mdpp_grid_sched_learn.hip", "mdpp_grid_summary_sched_learn.hip", "mdpp_grid_episodes_learn.hip", "mdpp_grid_episodes_sched_learn.hip")


# ---- plumbing ----
def test_header_has_the_section_and_every_new_symbol_is_declared_exported_and_bound():
    from mdp_playground_amd import _capi
    src = open(os.path.join(ROOT, "include", "mdpp.h")).read()
    assert "/* Grid learner schedules and the episode log." in src
    assert src.index("/* Grid learners:") < src.index("/* Grid learner schedules and the episode log.") < src.index("/* Linear policies:")
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _capi.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _capi.EXPORTS, name
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.mdpp_step_n_grid_learn_log.argtypes) == 12 and len(lib.mdpp_set_grid_learner_schedule.argtypes) == 7
    assert "A grid learner's schedule (mdpp_set_grid_learner_schedule)" in src     # the HIP graphs section
    assert len(lib.mdpp_grid_learn_kernel_name.argtypes) == 4                      # (its signature stays)


def test_methods_and_build_units():
    from mdp_playground_amd import build
    from mdp_playground_amd.vector_env import RLToyVectorEnv
    import inspect
    for m in ("set_grid_learner_schedule", "clear_grid_learner_schedule", "grid_learner_schedule", "grid_learner_episodes",
              "set_grid_learner_episodes"):
        assert callable(getattr(RLToyVectorEnv, m)), m
    assert "log" in inspect.signature(RLToyVectorEnv.rollout_grid_learn).parameters
    assert "log" not in inspect.signature(RLToyVectorEnv.rollout_grid_eval).parameters
    for u in NEW_UNITS:
        assert u in build.SOURCES and build.INCLUDED_SOURCES[u] == ["mdpp_grid_learn.hpp"] and u not in build.EXTRA_FLAGS
        assert os.path.exists(os.path.join(build.CSRC, u))
    assert "mdpp_grid_learn_body.inc" in build.HEADERS            # (the step loop every grid learner unit includes)


def test_the_cases_are_the_imported_configs_with_the_schedules_of_the_table():
    assert gsc.CASES is gc.CASES and (gsc.N, gsc.K, gsc.LAUNCHES, gsc.LOG_M) == (320, 37, 2, 3)
    assert {c: gsc.shape(c) for c in gsc.CASES} == {
        "g34_dense": (1, 3, True, False), "g55_sparse_limit_i32": (3, 5, True, True), "g55_noop_next_every3": (2, 4, False, True),
        "g17_noise": (1, 1, True, True), "g88_disabled_pnoise": (2, 6, True, False), "g34_noise_next_i32": (3, 7, True, True)}
    from mdp_playground_amd import policy
    for case in gsc.CASES:
        s = gsc.schedule(case)
        R, M, _, _ = gsc.shape(case)
        eps, al, rows, r, m = policy.learner_schedule_arrays(s["epsilon"], s["alpha"], s["row"], gsc.N)      # (what the method validates)
        assert (r, m) == (R, M) and (rows is None) == (R == 1)
        if R > 1:
            assert np.array_equal(rows, np.arange(gsc.N) % R)
        for t in (eps, al):
            if t is not None and M > 1:
                assert (np.diff(t, axis=1) < 0).all(), case                        # decreasing
                assert len({tuple(x) for x in t.tolist()}) == R, case              # distinct rows
    assert gsc.expected_name("g55_sparse_limit_i32", "philox", summary=True) == \
        "k_grid_learn_rollout<PHILOX=1,NOISE=0,QLDS=1,EVAL=0,SUMMARY=1,SCHED=1>"


# ---- the conditions that keep a GPU pass honest ----
@pytest.mark.parametrize("algo", gref.ALGOS)
@pytest.mark.parametrize("case", sorted(gsc.CASES))
def test_case_meets_its_conditions_on_the_cpu(case, algo):
    info, Q, ep, traj = gsc.cpu_run(case, algo)
    R, M, has_eps, has_alpha = gsc.shape(case)
    c = gsc.CASES[case]
    assert info["explored"] > 0 and info["updates"] > 0 and info["terminations"] > 0
    if M > 1:       # (M == 1 has one entry: nothing can change and every selection is made at the clamp; its condition is below)
        if has_eps:
            assert info["E_changes"] > 0
        if has_alpha:
            assert info["alpha_changes"] > 0
        assert info["sel_before_env"].any() and info["sel_last_env"].any()
    else:
        assert info["E_changes"] == 0 and info["alpha_changes"] == 0 and not info["sel_before_env"].any() and info["sel_last_env"].all()
    if c["kw"]["autoreset"] == "next_step":
        assert info["reset_calls"] > 0 and traj["reset_call"].sum() == info["reset_calls"]
    else:
        assert info["reset_calls"] == 0
    # the counters are the episode ends that are no reset calls
    ended = ((traj["terminated"] | traj["truncated"]) & ~traj["reset_call"]).sum(axis=0)
    assert np.array_equal(ep, ended)
    if c["kw"]["autoreset"] == "disabled":
        # the counter moves at every step once the limit is reached, past M - 1
        assert ep.min() >= gsc.LAUNCHES * gsc.K - c["kw"]["max_episode_steps"] + 1 > M - 1
    # the schedule matters: the same launches without it take other actions
    plain = gsc.cpu_run(case, algo, sched=None)
    assert not np.array_equal(plain[3]["actions"], traj["actions"]) or not np.array_equal(plain[1], Q)
    # every row of the tables was followed by some env, and the values a step began with are its row's
    s = gsc.ref_schedule(case)
    e = np.minimum(np.cumsum(np.vstack([np.zeros((1, gsc.N), np.int64), ((traj["terminated"] | traj["truncated"]) & ~traj["reset_call"])[:-1]]), axis=0), M - 1)
    if has_eps:
        assert np.array_equal(traj["E"], s.T[s.row[None, :], e])
    if has_alpha:
        assert np.array_equal(traj["alpha"], s.A[s.row[None, :], e])
    assert len(set(s.row.tolist())) == R


def test_conditions_met_once_over_all_cases():
    carried_old_E_differs = 0
    over = under = spanning = wave = 0
    for case in sorted(gsc.CASES):
        for algo in gref.ALGOS:
            info, Q, ep, traj = gsc.cpu_run(case, algo)
            carried_old_E_differs += info["carried_old_E_differs"]
            if algo == "q_learning":
                assert info["carried"] == 0
            c = lref.new_counters()
            gsr.log_of(traj, gsc.K, gsc.LAUNCHES, gsc.LOG_M, counters=c)
            over, under, spanning, wave = over + c["over_M"], under + c["under_M"], spanning + c["spanning_logged"], wave + c["wave_rows_differ"]
    assert carried_old_E_differs > 0       # a carried SARSA action chosen under another E that a fresh selection would not have taken
    assert over > 0 and under > 0          # envs above and below the log's capacity
    assert spanning > 0                    # a logged episode that spans the launch boundary
    assert wave > 0                        # lanes of one wave writing different rows at one step


@pytest.mark.parametrize("case", sorted(gsc.CASES))
def test_the_two_exact_consequences_of_the_log_text(case):
    info, Q, ep, traj = gsc.cpu_run(case, "sarsa")
    # at the cases' capacity, and at one no env outgrows (two launches of K steps end at most 2 K episodes)
    for M in (gsc.LOG_M, gsc.LAUNCHES * gsc.K):
        log, st, _ = gsr.log_of(traj, gsc.K, gsc.LAUNCHES, M, fill_ret=-7.5, fill_len=-7)
        assert np.array_equal(log["count"], st["episodes"])
        assert np.array_equal(log["count"], ep)               # ... and, from zeroed counters, the schedule's
        fits = np.flatnonzero(log["count"] <= M)
        assert M == gsc.LOG_M or len(fits) == gsc.N
        for i in fits:
            assert lref.left_to_right_sum(log, i).view(np.int64) == st["return_sum"][i].view(np.int64), i
            assert log["len"][:log["count"][i], i].sum() == st["length_sum"][i]
        # unwritten entries keep what they held
        for i in range(gsc.N):
            assert (log["ret"][min(log["count"][i], M):, i] == -7.5).all() and (log["len"][min(log["count"][i], M):, i] == -7).all()


# ---- what the schedule is for ----
LEARN_CFG = dict(state_space_type="grid", reward_function="move_to_a_point", grid_shape=(8, 8), make_denser=False, target_point=[6, 6], seed=3)
LEARN_KW = dict(autoreset="same_step", max_episode_steps=40)
LEARN_N, LEARN_STEPS, LEARN_DECAY_EPISODES = 32, 2000, 40
# reward per step in the second half, measured on the restatement with the shapes above (q_learning, alpha = 0.5, gamma = 0.9,
# learner seed 11, Philox seed 5): epsilon decaying 1 -> 0.05 over each env's first 40 episodes, and constant epsilon at each
# endpoint and at 0.3.  The gaps are 0.11628 (epsilon = 1), 0.02328 (0.3) and 0.09766 (0.05); the bound asserted is HALF the
# smallest of them
MEASURED = {"decay": 0.1266875, 1.0: 0.01040625, 0.3: 0.10340625, 0.05: 0.02903125}
HALF_SMALLEST_GAP = 0.5 * min(MEASURED["decay"] - MEASURED[e] for e in (1.0, 0.3, 0.05))


def _reward_per_step(sched, epsilon):
    info, Q, ep, traj = gsr.closed_loop(LEARN_CFG, LEARN_KW, "q_learning", 0.5, 0.9, epsilon, LEARN_N, None, sched, seed=11, K=LEARN_STEPS,
                                        launches=1, philox_seed=5, off=0)
    return float(traj["reward"][LEARN_STEPS // 2:].astype(np.float64).mean()), ep


def test_a_decaying_epsilon_learns_a_sparse_gridworld_faster_than_any_constant_one():
    from mdp_playground_amd import policy
    table = policy.epsilon_decay("linear", 1.0, LEARN_DECAY_EPISODES, 0.05).astype(np.float32)
    decay, ep = _reward_per_step(sref.Schedule(LEARN_N, epsilon=table), 1.0)
    assert ep.min() > LEARN_DECAY_EPISODES                      # every env reached the last entry
    consts = {e: _reward_per_step(None, e)[0] for e in (1.0, 0.3, 0.05)}
    print("decay", decay, "const", consts)
    for e, v in consts.items():
        assert decay - v >= HALF_SMALLEST_GAP, (e, decay, v)
