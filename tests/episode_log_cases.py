"""What tests/test_gpu_episode_log.py runs and what it asserts about its own coverage (the episode log: log= on rollout_learn
with summary=; include/mdpp.h "Episode summaries"), shared with tests/test_episode_log_host.py,
which shows on the CPU (the oracle env in a closed loop, 32 envs, K = 37, two launches, Philox streams) that those conditions
can be met before any GPU run.

The cases.  Four are eval_summary_cases.SUMMARY_CASES -- a shared MDP, form "plain": cfg2, next-step autoreset, autoreset
disabled with max_episode_steps = 5, s8 with noise.  Six are one each per later kernel form, made as
tests/test_gpu_schedule_sweep.py makes its handles (schedule_sweep_cases / closed_forms_shape_cases):
    nlev_d2          per-env noise levels on a shared MDP                              ,NLEV=1
    pm2_d2           one MDP per env, the tables in LDS slots                          ,PM=2
    pm1_d4           one MDP per env read in global memory (d4_s24_a6)                 ,PM=1
    pm_nlev_sched    levels, one MDP per env and a per-episode schedule                ,NLEV=1,PM=2,SCHED=1
    pm_custom_5x3    S != A (5 x 3), custom reward matrix, key ring                    ,PM=2, UNIT=0
    pm_nlev_trunc    truncation (max_episode_steps = 5) under next-step autoreset, with levels, per-env MDPs and a schedule
A run is (case, algo, stream) with algo one of the three learners (rollout_eval keeps no log: DESIGN.md 3.24).

M per case: the median of the per-env finished-episode counts of the case's own 32-env CPU closed loops over both launches,
at least 2.  A case has three such loops, one per learner, and ONE M: the median is taken over the 3 x 32 counts pooled (this
file's reading of "the case's own closed loop").  The values are written down in LOG_M beside the counts they come from;
tests/test_episode_log_host.py recomputes them.

What a pass must have exercised (honest()): some env ends past M and some env short of it; a logged episode that began in the
earlier launch; at one step lanes of one 64-env wave wrote different rows.  SCOPED lists the (case, algo) that cannot meet
one, with the reason: none does."""
import numpy as np

import eval_summary_cases as esc
import eval_summary_ref as eref
import schedule_sweep_cases as ssc
from closed_loop_cpu import closed_loop as shared_closed_loop

N, K, LAUNCHES, OFF = 320, esc.K, esc.LAUNCHES, 1000
assert (K, LAUNCHES) == (ssc.K, ssc.LAUNCHES) == (37, 2) and (N, OFF) == (ssc.N, ssc.OFF)
SEED, ALPHA, GAMMA, EPS = esc.SEED, esc.ALPHA, esc.GAMMA, esc.EPS
assert (SEED, ALPHA, GAMMA, EPS) == (ssc.SEED, ssc.ALPHA, ssc.GAMMA, ssc.EPS)
PHILOX_SEED = ssc.PHILOX_SEED
ALGOS = esc.SUMMARY_ALGOS
RNGS = ("numpy", "philox")
SENTINEL_RET, SENTINEL_LEN = -12345.678, -77          # what the unwritten entries hold before a launch

# case -> (form, the case's name where the form's handles are made, schedule kind or None)
CASES = {
    "cfg2": ("plain", "cfg2", None),
    "cfg2_next_step": ("plain", "cfg2_next_step", None),
    "cfg2_disabled_max5": ("plain", "cfg2_disabled_max5", None),
    "s8_noise": ("plain", "s8_noise", None),
    "nlev_d2": ("nlev", "d2_s12_a6_L2", None),
    "pm2_d2": ("pm", "d2_s12_a6_L2", None),
    "pm1_d4": ("pm", "d4_s24_a6", None),
    "pm_nlev_sched": ("pm_nlev", "d2_s12_a6_L2", "both"),
    "pm_custom_5x3": ("pm", "custom_5x3", None),
    "pm_nlev_trunc": ("pm_nlev", "trunc_next", "both"),
}
RUNS = [(c, a, r) for c in CASES for a in ALGOS for r in RNGS]

# case -> M, beside the pooled counts of the 32 CPU envs x three learners it is the median of: min - max
LOG_M = {
    "cfg2": 12,                 # 3 - 39
    "cfg2_next_step": 9,        # 3 - 27
    "cfg2_disabled_max5": 71,   # 70 - 74: every step from an env's fifth on is an episode
    "s8_noise": 13,             # 4 - 33
    "nlev_d2": 10,              # 2 - 20
    "pm2_d2": 12,               # 1 - 27
    "pm1_d4": 10,               # 1 - 31
    "pm_nlev_sched": 12,        # 1 - 34
    "pm_custom_5x3": 11,        # 0 - 46
    "pm_nlev_trunc": 16,        # 13 - 22 (max_episode_steps = 5, a reset call a step of its own)
}
assert set(LOG_M) == set(CASES)

# (case, algo) -> the conditions it cannot meet and why.  "over": no env ends past M; "under": none short of it; "spans": no
# logged episode began in the earlier launch; "rows": no wave writes two different rows at one step
SCOPED = {}


def autoreset_of(case):
    form, name, _ = CASES[case]
    kw = esc.SUMMARY_CASES[name][1] if form == "plain" else ssc.kw_of(name)
    return kw.get("autoreset", eref.SAME_STEP)


def shape_of(case):
    """(S, A) of the case's MDPs"""
    form, name, _ = CASES[case]
    if form == "plain":
        cfg = esc.SUMMARY_CASES[name][0]
        return cfg["state_space_size"], cfg["action_space_size"]
    m = ssc.mdps_of(form, name, 1)[0]
    return m.S, m.A


def learner_tables(case, algo, n):
    """what a learner starts from: the plain cases as tests/test_gpu_eval_summary.py (random tables), the later forms from zero"""
    form = CASES[case][0]
    if form != "plain":
        return None
    S, A = shape_of(case)
    return esc.tie_q(esc.random_q(esc.Q_SEED, n, S, A, algo == "double_q"))


def cpu_loop(case, algo, n=32):
    """(reward float32, terminated, truncated, reset_call), each [LAUNCHES K, n]: the case's closed loop on the CPU"""
    form, name, kind = CASES[case]
    if form == "plain":
        cfg, kw = esc.SUMMARY_CASES[name]
        _, _, t = shared_closed_loop(cfg, kw, algo, ALPHA, GAMMA, EPS, n, learner_tables(case, algo, n), seed=SEED, K=K, launches=LAUNCHES)
    else:
        _, t = ssc.closed_loop(form, name, algo, kind, n, sched="case" if kind else None)
    return t["reward"], t["terminated"], t["truncated"], t["reset_call"]


def counts_of(term, trunc, reset_call):
    """finished episodes per env"""
    return ((np.asarray(term, bool) | np.asarray(trunc, bool)) & ~np.asarray(reset_call, bool)).sum(axis=0)


def median_m(counts):
    return max(2, int(np.median(np.asarray(counts))))


def honest(case, algo, counters):
    """what a pass with the case's M must have exercised (counters: episode_log_ref.new_counters, after the last launch)"""
    skip = SCOPED.get((case, algo), {})
    if "over" not in skip:
        assert counters["over_M"] > 0, (case, algo, counters)
    if "under" not in skip:
        assert counters["under_M"] > 0, (case, algo, counters)
    # autoreset disabled with max_episode_steps = 5: from an env's fifth step on every step is an episode of its own, so no
    # episode is running when launch 1 ends (eval_summary_cases.summary_honest)
    if case != "cfg2_disabled_max5" and "spans" not in skip:
        assert counters["spanning_logged"] > 0, (case, algo, counters)
    if "rows" not in skip:
        assert counters["wave_rows_differ"] > 0, (case, algo, counters)
    if case == "cfg2_disabled_max5":
        assert counters["ended_terminated"] > 0 and counters["ended_truncated"] > 0, counters
    if case == "pm_nlev_trunc":
        assert counters["ended_truncated"] > 0, counters
    if autoreset_of(case) == eref.NEXT_STEP:
        assert counters["reset_calls"] > 0, counters
