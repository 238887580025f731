"""What tests/test_gpu_learn_schedule.py runs and what it asserts about its own coverage, shared with
tests/test_learner_schedule_host.py, which shows on the CPU (32 envs, the oracle env in a closed loop with the restatement
tests/learner_schedule_ref.py) that those counts can be met before any GPU run.

Every schedule has R = 4 rows and env i follows row i % 4:
    row 0  const      0.25                     (alpha: 0.3)
    row 1  linear     1 -> 0                   (alpha: 1 -> 0.1)
    row 2  log        0.5 -> 0.001             (alpha: 0.5 -> 0.01)
    row 3  the step   [0, ..., 0, 1]           (alpha: [0.1, ..., 0.1, 1])
M is chosen per handle from the episodes a constant-epsilon run of 2 x 37 steps gives it (CPU closed loop, 32 envs), so that
some envs run past the table's end (final ep >= M: the clamp) and some stop short of its last entry (final ep < M - 1):
    cfg2, cfg2_next_step    1 - 17 episodes per env, median 5              M = 6
    s8_max5                 max_episode_steps = 5: 17 - 33 per env         M = 24
    s8_noise                5 - 41 per env, median about 14                M = 14
    s20                     9 - 44 per env, median about 30                M = 28
    cfg2_disabled_max5      autoreset disabled: truncated stays set from step 5 on, the counter moves at every step and
                            reaches 70 - 74 on EVERY env: all clamp, none stops short -- the "below M" assertion does not
                            apply to this handle (BELOW_M_EXEMPT); it is the handle of sarsa's carry across a boundary.
The step row on cfg2 and cfg2_next_step (STEP_ROW_STAYS): these handles end an episode at a terminal state only, and the
greedy walk from all-zero tables never reaches one on this MDP: action 0 wins every tie, leads from every start state
into the cycle 3 -> 4 -> 2 -> 5, and rewards are never negative, so Q[s][0] stays the row's maximum -- a step-row env that may not explore never ends its first episode.  There the assertion is its first half:
such an env makes selections, explores at none of them and its counter stays 0.  The four other handles (truncation,
noise, or an MDP whose action-0 walk terminates) carry the whole assertion.
Which tables a case schedules goes by (handle, algo, rng): epsilon alone, alpha alone, or both -- a third of the cases each."""
import numpy as np

import learner_schedule_ref as sref
import learner_sweep_cases as sweep

K, LAUNCHES = sweep.K, sweep.LAUNCHES
SEED, ALPHA, GAMMA, EPS = sweep.SEED, sweep.ALPHA, sweep.GAMMA, sweep.EPS
R = 4

HANDLES = {
    "cfg2": (sweep.CFG2, {}, 6),
    "cfg2_next_step": (sweep.CFG2, dict(autoreset="next_step"), 6),
    "cfg2_disabled_max5": (sweep.CFG2, dict(autoreset="disabled", max_episode_steps=5), 6),
    "s8_noise": (dict(sweep._S8, transition_noise=0.1, reward_noise=0.5), {}, 14),
    "s8_max5": (sweep._S8, dict(max_episode_steps=5), 24),
    "s20": (sweep.S20, {}, 28),
}
GLOBAL_FORM = ("s20",)
BELOW_M_EXEMPT = ("cfg2_disabled_max5",)
STEP_ROW_STAYS = ("cfg2", "cfg2_next_step")
KINDS = ("eps", "alpha", "both")
ALGOS = ("q_learning", "sarsa", "double_q")
RNGS = ("numpy", "philox")


def kind_of(handle, algo, rng):
    return KINDS[(list(HANDLES).index(handle) + ALGOS.index(algo) + RNGS.index(rng)) % 3]


def decay(kind, start, m, final=0.0):
    """policy.epsilon_decay's definitions, restated (tests/test_learner_schedule_host.py holds the product's to them)"""
    x = np.arange(m, dtype=np.float64) / np.float64(max(m - 1, 1))
    if kind == "const":
        return np.full(m, float(start))
    if kind == "linear":
        return start + (final - start) * x
    return start * (final / start) ** x


def step_row(m, low, high):
    return np.array([low] * (m - 1) + [high], np.float64)


def eps_rows(m):
    return np.stack([decay("const", 0.25, m), decay("linear", 1.0, m, 0.0), decay("log", 0.5, m, 0.001), step_row(m, 0.0, 1.0)])


def alpha_rows(m):
    return np.stack([decay("const", 0.3, m), decay("linear", 1.0, m, 0.1), decay("log", 0.5, m, 0.01), step_row(m, 0.1, 1.0)])


def tables(kind, m):
    """(epsilon, alpha) float64 [R, m] or None, of a case's kind"""
    return (eps_rows(m) if kind in ("eps", "both") else None), (alpha_rows(m) if kind in ("alpha", "both") else None)


def rows(n, lo=0):
    return ((np.arange(lo, lo + n)) % R).astype(np.int32)


def schedule(kind, m, n, lo=0):
    eps, al = tables(kind, m)
    return sref.Schedule(n, eps, al, rows(n, lo))


def honest(handle, algo, kind, m, info, ep, row):
    """what a scheduled pass must have exercised: info summed over the launches, ep [n] the final counters"""
    ep = np.asarray(ep)
    assert (ep >= m).any(), ("no env ran past the table's end", handle, ep.min(), ep.max())
    if handle in BELOW_M_EXEMPT:
        assert (ep >= m).all() and ep.min() >= 2 * K - 5, (handle, ep.min())      # (every step from the fifth on counts)
    else:
        assert (ep < m - 1).any(), ("no env stopped short of the last entry", handle, ep.min(), ep.max())
    assert info["updates"] > 0 and info["greedy_strict"] > 0, info
    if kind in ("eps", "both"):
        assert info["E_changes"] > 0, info
        st = np.asarray(row) == 3
        assert st.any()
        assert (info["sel_before_env"][st] > 0).all(), (handle, algo)
        assert (info["expl_before_env"][st] == 0).all(), "the step row explored before its last entry"
        if handle in STEP_ROW_STAYS:
            assert (ep[st] == 0).all(), (handle, ep[st])
        else:
            assert info["sel_last_env"][st].sum() > 0, (handle, algo)
        assert (info["expl_last_env"][st] == info["sel_last_env"][st]).all(), "the step row did not explore at its last entry"
        if algo == "sarsa" and handle == "cfg2_disabled_max5":
            assert info["carried_old_E"] > 0 and info["carried_old_E_differs"] > 0, info
    if kind in ("alpha", "both"):
        assert info["alpha_changes"] > 0, info
    if handle == "cfg2_next_step":
        assert info["reset_calls"] > 0, info
