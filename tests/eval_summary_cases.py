"""What tests/test_gpu_eval_summary.py runs and what it asserts about its own coverage, shared with
tests/test_eval_summary_host.py, which shows on the CPU (32 envs, the oracle env in a closed loop with the restatement
tests/eval_summary_ref.py) that those counts can be met before any GPU run.

The handles and the MDP seeds are tests/learner_sweep_cases.py's DOUBLE_CASES (without its "cfg2_random_q", which is "cfg2"
with random tables: every evaluation here starts from random tables -- all-zero tables make the greedy choice action 0
everywhere and show nothing).  No seed had to be replaced: the CPU closed loop meets every counter below with them."""
import numpy as np

import learner_sweep_cases as sweep

K, LAUNCHES, SEED = sweep.K, sweep.LAUNCHES, sweep.SEED
ALPHA, GAMMA, EPS = sweep.ALPHA, sweep.GAMMA, sweep.EPS
random_q, pe_arrays = sweep.random_q, sweep.pe_arrays

EVAL_CASES = {k: v for k, v in sweep.DOUBLE_CASES.items() if k != "cfg2_random_q"}
GLOBAL_FORM = sweep.GLOBAL_FORM
EVAL_ALGOS = ("q_learning", "double_q")
Q_SEED = 9                        # random_q's seed of the evaluated tables
TIE_EVERY = 3                     # every third env's tables are rounded to multiples of 1 (ties between actions; see tie_q)

SUMMARY_CASES = {k: sweep.DOUBLE_CASES[k] for k in ("cfg2", "cfg2_next_step", "cfg2_disabled_max5", "s8_noise")}
SUMMARY_ALGOS = ("q_learning", "sarsa", "double_q")


def tie_q(q):
    """random tables in which a tie for the greedy action is common in every TIE_EVERY-th env: those envs' entries are
    rounded to whole numbers (a standard normal rounds to -1, 0 or 1 mostly: rows with several equal maxima), for double Q
    in both tables (their sums tie as well)."""
    q = q.copy()
    q[::TIE_EVERY] = np.round(q[::TIE_EVERY])
    return q


def eval_honest(info, double):
    """what an evaluation pass must have exercised (info summed over the launches of one handle)"""
    assert info["greedy_strict"] > 0 and info["greedy_ties"] > 0, info
    assert info["terminations"] > 0, info
    if double:
        assert info["sum_differs"] > 0, info


def summary_honest(counters, return_sum, case, algo):
    """what a summary pass must have exercised (counters summed over the launches of one handle; return_sum: what the pops
    returned, added up; algo: the learner's, or "eval").  An episode that spans the launch boundary is asked of the handles that reset: with autoreset
    disabled and max_episode_steps = 5 every step from an env's fifth on is truncated -- an episode of one step -- so no
    episode is running when launch 1 ends, whatever the seed.
    A non-zero return_sum is not asked of greedy evaluation on the noise-free cfg2 handles that reset: policy and transitions
    are deterministic there, so an episode that ends walks through distinct states -- at most 7 transitions among 8 states --
    while cfg2's reward needs a sequence of 3 states and arrives 4 steps later, in an episode of 8 steps or more.  An env that
    earns reward under a greedy policy is in a cycle and never finishes its episode (seen on the CPU for 24 table seeds: up to
    66 rewards, none in a finished episode).  The learners explore, s8_noise has noise, and with autoreset disabled every
    late step is an episode: those handles must show a non-zero return_sum."""
    assert counters["two_in_one_launch"] > 0, counters
    if case != "cfg2_disabled_max5":
        assert counters["spans_boundary"] > 0, counters
    if not (algo == "eval" and case in ("cfg2", "cfg2_next_step")):
        assert (return_sum != 0).any()
    if case == "cfg2_disabled_max5":
        assert counters["ended_terminated"] > 0 and counters["ended_truncated"] > 0, counters
    if case == "cfg2_next_step":
        assert counters["reset_calls"] > 0, counters
