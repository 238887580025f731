"""What tests/test_gpu_schedule_sweep.py runs and what it asserts about its own coverage (per-episode epsilon / alpha schedules on
the noise-level and per-env-MDP learners: set_learner_schedule(..., sweep=True); the SCHED forms of the learner kernels with
NLEV=1 and / or PM != 0; include/mdpp.h "Schedules"), shared with tests/test_schedule_sweep_host.py, which
shows on the CPU that those conditions can be met before any GPU run.

Three forms, named as in closed_forms_shape_cases:
    nlev      a shared MDP with per-env noise levels                  ...,PE=1[,DOUBLE=1],NLEV=1,SCHED=1>
    pm        one MDP per env                                         ...,PE=1[,DOUBLE=1],PM=1|2,SCHED=1>
    pm_nlev   one MDP per env with per-env noise levels               ...,PE=1[,DOUBLE=1],NLEV=1,PM=1|2,SCHED=1>
The set-up is per_env_mdp_cpu's (N = 320, K = 37, two launches, env_id_offset = 1000), the shapes are closed_forms_shape_cases'
and the tabular 8 x 8 with both noise keys, the levels noise_seed_cases' seven pairs by i % 7, the schedules
learner_schedule_cases' four rows by i % 4: 4 and 7 are coprime, so every 28 consecutive envs -- and every wave of 64 -- hold
every (pair, row) combination, on 64 different seeds where the handle has one MDP per env.

M per (form, case): chosen from the case's own CPU episode counts under the schedule (32 envs, Philox streams, 2 x 37 steps,
every algorithm and kind of the case) so that some envs run past the table's end and some stop short of its last entry; the
counts are beside each entry of SCHED_M."""
import numpy as np

import closed_forms_shape_cases as cfs
import learner_schedule_cases as lsc
import learner_schedule_ref as sref
import learner_sweep_cases as sweep
import learner_sweep_ref as ref
import noise_seed_cases as nsc
import per_env_mdp_cpu as pm
from closed_loop_cpu import make_oracles

N, K, LAUNCHES, OFF = cfs.N, cfs.K, cfs.LAUNCHES, cfs.OFF
SEED, PHILOX_SEED = cfs.SEED, cfs.PHILOX_SEED
ALPHA, GAMMA, EPS = cfs.ALPHA, cfs.GAMMA, cfs.EPS
ALGOS, RNGS, KINDS = lsc.ALGOS, lsc.RNGS, lsc.KINDS
CREATED = cfs.CREATED
FORMS = ("nlev", "pm", "pm_nlev")
PER_ENV_FORMS, LEVEL_FORMS = cfs.PER_ENV_FORMS, ("nlev", "pm_nlev")
level_arrays, pairs_present, rows = cfs.level_arrays, cfs.pairs_present, lsc.rows

# the tabular shape of the reference's experiment files with both noise keys.  The levelled forms replace the two values by the
# envs' levels; the pm form keeps them, uniform
S8_NOISE = dict(sweep._S8, transition_noise=0.1, reward_noise=0.5)

# form -> its cases.  One truncation case per form, the one whose autoreset mode lets the restatement see the true next state
# of a truncated step under that form's noise (same-step autoreset hides it: the noise-free pm form has that one)
FORM_CASES = {
    "nlev": ("s8_noise", "d2_s12_a6_L2", "d4_s24_a6", "trunc_disabled"),
    "pm": ("s8_noise", "d2_s12_a6_L2", "d4_s24_a6", "custom_5x3", "trunc_same"),
    "pm_nlev": ("s8_noise", "d2_s12_a6_L2", "d4_s24_a6", "custom_5x3", "trunc_next"),
}
RUNS = [(f, c, a, r) for f in FORMS for c in FORM_CASES[f] for a in ALGOS for r in RNGS]

# (form, case) -> M, beside the final counters of the 32 CPU envs over the case's algorithms and kinds: min - max, and how many
# of the 32 ended at or past M / short of M - 1 in the run with the fewest of each
SCHED_M = {
    ("nlev", "s8_noise"): 14,               # 2 - 37; 12 / 8
    ("nlev", "d2_s12_a6_L2"): 12,           # 2 - 25; 12 / 14
    ("nlev", "d4_s24_a6"): 15,              # 4 - 28; 17 / 9
    ("nlev", "trunc_disabled"): 6,          # 70 - 74; 32 / 0: every step from the fifth on counts (scoped below)
    ("pm", "s8_noise"): 9,                  # 3 - 35; 17 / 11 (at M = 14 the step-row envs of three runs end at most 11 episodes: none at its last entry)
    ("pm", "d2_s12_a6_L2"): 12,             # 0 - 34; 11 / 13
    ("pm", "d4_s24_a6"): 15,                # 0 - 30; 11 / 18
    ("pm", "custom_5x3"): 8,                # 0 - 45; 15 / 9
    ("pm", "trunc_same"): 20,               # 14 - 36; 18 / 9 (max_episode_steps = 5: at least 14 episodes per env)
    ("pm_nlev", "s8_noise"): 14,            # 0 - 34; 10 / 13
    ("pm_nlev", "d2_s12_a6_L2"): 12,        # 1 - 34; 16 / 10
    ("pm_nlev", "d4_s24_a6"): 15,           # 3 - 27; 12 / 16
    ("pm_nlev", "custom_5x3"): 8,           # 0 - 43; 18 / 9
    ("pm_nlev", "trunc_next"): 17,          # 13 - 22; 15 / 12 (a reset call takes a step of its own: fewer episodes than trunc_same)
}
assert set(SCHED_M) == {(f, c) for f in FORMS for c in FORM_CASES[f]}

# ---- scoping: a condition a case cannot meet, with the reason
# sarsa's carry across an episode boundary exists only where an episode ends and the env goes on from s': autoreset disabled
# past max_episode_steps.  Termination ends the carry, and truncation under the two autoreset modes drops it (the reset).  So
# the condition is trunc_disabled's; every other case counts 0 carried_old_E by construction (asserted: it must stay 0 there).
SARSA_CARRY_CASES = ("trunc_disabled",)
# autoreset disabled: the counter moves at every step from the fifth on, every env clamps, none stops short
# (learner_schedule_cases.BELOW_M_EXEMPT, whose handle name the case borrows)
_HONEST_ALIAS = {"trunc_disabled": "cfg2_disabled_max5"}


def base_cfg(case):
    """the case's config without noise keys and seed"""
    return cfs._plain(S8_NOISE if case == "s8_noise" else cfs.CASES[case])


def kw_of(case):
    return cfs.KW.get(case, {})


def autoreset_of(case):
    return kw_of(case).get("autoreset", ref.SAME_STEP)


def shared_seed(case):
    return 0 if case == "s8_noise" else cfs.shared_cfg(case)["seed"]


def seeds_of(case, n=None, lo=0):
    return cfs.seeds_of(case, n, lo)


def handle_cfg(form, case, pair=None):
    """the config a handle of the form is created with.  pair: the (p, sigma) of a uniform twin of a levelled form, else the
    levelled forms' CREATED keys; the pm form keeps the case's own noise keys.  per_env_cfg (custom matrices per seed) stays in
    for the per-env forms: closed_forms_shape_cases.handle_cfg resolves it"""
    src = S8_NOISE if case == "s8_noise" else cfs.CASES[case]
    cfg = {k: v for k, v in src.items() if k not in ("seed", "transition_noise", "reward_noise") and (form in PER_ENV_FORMS or k != "per_env_cfg")}
    if form in LEVEL_FORMS:
        cfg.update(CREATED if pair is None else dict(transition_noise=float(pair[0]), reward_noise=float(pair[1])))
    elif case == "s8_noise":
        cfg.update(transition_noise=S8_NOISE["transition_noise"], reward_noise=S8_NOISE["reward_noise"])
    if form not in PER_ENV_FORMS:
        cfg["seed"] = shared_seed(case)
    return cfg


def kind_of(form, case, algo, rng):
    """epsilon alone, alpha alone or both: a third of the runs each, every form and case with all three"""
    return KINDS[(FORMS.index(form) + FORM_CASES[form].index(case) + ALGOS.index(algo) + RNGS.index(rng)) % 3]


def sched_m(form, case):
    return SCHED_M[(form, case)]


def schedule(form, case, kind, n, lo=0):
    return lsc.schedule(kind, sched_m(form, case), n, lo)


def tables(form, case, kind):
    return lsc.tables(kind, sched_m(form, case))


def levels_of(form, n, lo=0):
    """(tn, rn) of a levelled form's envs, else (None, None)"""
    return level_arrays(n, lo) if form in LEVEL_FORMS else (None, None)


def mdps_of(form, case, n=None, lo=0):
    """the MDP of every env, at its own level and with the case's own noise keys: what the oracle steps.  A list of n"""
    n = N if n is None else n
    if form == "pm":                                     # (the case's own keys, or none: no key, no draw)
        return pm.build_mdps(handle_cfg(form, case), seeds_of(case, n, lo))
    cfg = {k: v for k, v in handle_cfg(form, case).items() if k not in ("seed", "transition_noise", "reward_noise")}
    seeds = seeds_of(case, n, lo) if form in PER_ENV_FORMS else [shared_seed(case)] * n
    return nsc.level_mdps(cfg, *level_arrays(n, lo), seeds)


def P_of(form, case, n=None, lo=0):
    """the P argument of learner_schedule_ref.run"""
    mdps = mdps_of(form, case, n, lo)
    return pm.PerEnvP(mdps) if form in PER_ENV_FORMS else np.asarray(mdps[0].P)


def new_agent(form, case, algo, kind, n, lo=0, sched="case"):
    m = mdps_of(form, case, 1)[0]
    shape = (n, 2, m.S, m.A) if algo == "double_q" else (n, m.S, m.A)
    sc = schedule(form, case, kind, n, lo) if sched == "case" else sched
    return sref.Agent(algo, n, ALPHA, GAMMA, EPS, sc, np.zeros(shape, np.float32), autoreset_of(case))


def kernel_name(form, cfg, algo, rng, qlds, pmv=None, summary=False, sched=True):
    """closed_forms_shape_cases.kernel_name with ",SCHED=1" after everything else"""
    name = cfs.kernel_name("learn", form, cfg, algo, rng, qlds, pmv, summary)
    assert name.endswith(">") and "SCHED" not in name
    return name[:-1] + ",SCHED=1>" if sched else name


def expected_placement(form, case, algo, rng, limit, options=()):
    """(QLDS, PM or None) of the form's handle: a schedule has no LDS placement, so the unscheduled handle's rule holds"""
    double = algo == "double_q"
    if form == "nlev":
        return cfs.nlev_expected(handle_cfg(form, case), double, rng, limit, options)[0], None
    if form == "pm_nlev":
        return cfs.pm_nlev_expected(handle_cfg(form, case), double, rng, limit, options)[:2]
    return cfs.pm_expected(handle_cfg(form, case), double, limit, options)


# ---- the CPU closed loop: learner_schedule_cpu.closed_loop (one MDP for all envs) with the envs made one by one, each the
# oracle of its own MDP at its own level, as per_env_mdp_cpu.closed_loop makes them
def closed_loop(form, case, algo, kind, n, *, sched="case", k=K, launches=LAUNCHES):
    """launches x k steps of n envs under the form's handle and the scheduled learner.  Returns (agent, traj): the Agent at the end
    (Q, ep, info) and [launches k, n] arrays -- actions, obs, reward, terminated, truncated, reset_call, state, next_state (the
    true one) -- and obs0 [n]"""
    mdps = mdps_of(form, case, n)
    kw = kw_of(case)
    autoreset, max_steps = autoreset_of(case), kw.get("max_episode_steps", 0)
    envs = [make_oracles(mi, 1, PHILOX_SEED, OFF + i)[0] for i, mi in enumerate(mdps)]
    s = np.array([o.reset() for o in envs], np.int64)
    agent = new_agent(form, case, algo, kind, n, sched=sched)
    total = launches * k
    w = {st: ref.tick_words(SEED, OFF, 0, total + 1, n, st) for st in (ref.EXPLORE_STREAM, ref.ACTION_STREAM, ref.UPDATE_STREAM)}
    steps = np.zeros(n, np.int64)
    traj = {key: np.zeros((total, n), dt) for key, dt in (("actions", np.int64), ("obs", np.int64), ("reward", np.float32), ("terminated", bool),
                                                          ("truncated", bool), ("reset_call", bool), ("state", np.int64), ("next_state", np.int64))}
    traj["obs0"] = s.copy()
    for t in range(total):
        if t % k == 0:
            agent.launch_start()
        pending = agent.pending.copy()
        live = ~pending
        a = agent.act(s, w[ref.EXPLORE_STREAM][t], w[ref.ACTION_STREAM][t])
        s2, r, te = s.copy(), np.zeros(n, np.float32), np.zeros(n, bool)
        for i in np.flatnonzero(live):
            o, rr, d = envs[i].step(int(a[i]))
            s2[i], r[i], te[i] = o, np.float32(rr), d
        steps[live] += 1
        tr = live & (max_steps > 0) & (steps >= max_steps)
        traj["state"][t], traj["next_state"][t] = s, s2
        agent.learn(s, a, r, s2, te, tr, w[ref.EXPLORE_STREAM][t + 1], w[ref.ACTION_STREAM][t + 1], w[ref.UPDATE_STREAM][t])
        ended = live & (te | tr)
        for i in np.flatnonzero(pending | (ended & (autoreset == ref.SAME_STEP))):
            if pending[i]:
                # (a next-step reset call takes a tick of its own: per_env_mdp_cpu.closed_loop says why)
                envs[i].set_philox(PHILOX_SEED, OFF + i, t + 1, 1)
            s2[i] = envs[i].reset(explicit=False)
            steps[i] = 0
        for key, v in (("actions", a), ("obs", s2), ("reward", r), ("terminated", te), ("truncated", tr), ("reset_call", pending)):
            traj[key][t] = v
        s = s2
    return agent, traj


# ---- what a pass must have exercised
def triples_honest(form, case, n, lo=0):
    """at least two distinct (level pair, seed, row) triples in every wave of 64 lanes (in fact: all different)"""
    tn, rn = levels_of(form, n, lo)
    row = rows(n, lo)
    seeds = seeds_of(case, n, lo) if form in PER_ENV_FORMS else [shared_seed(case)] * n
    for at in range(0, n, 64):
        hi = min(at + 64, n)
        triples = {((tn[i], rn[i]) if tn is not None else None, seeds[i], int(row[i])) for i in range(at, hi)}
        assert len(triples) >= min(2, hi - at), (form, case, at, len(triples))


def honest(form, case, algo, kind, info, ep, row, state=None, actions=None, next_state=None, seen=None, tn=None, P=None):
    """learner_schedule_cases.honest for the case's M (E / alpha changed inside a launch, envs past and short of the table, the
    step row, sarsa's carry across a boundary on the case that has one) and, on a levelled form, the level-0 envs making no
    noisy transition beside envs that make one.  state, actions, next_state, seen [T, n]: every step's state acted from,
    action, next state and whether that next state is known to be the true one; P [S, A] or [n, S, A]"""
    lsc.honest(_HONEST_ALIAS.get(case, "s20"), algo, kind, sched_m(form, case), info, ep, row)
    if algo == "sarsa" and kind in ("eps", "both"):
        if case in SARSA_CARRY_CASES:
            assert info["carried_old_E"] > 0 and info["carried_old_E_differs"] > 0, info
        else:
            assert info["carried_old_E"] == 0, info
    if autoreset_of(case) == ref.NEXT_STEP:
        assert info["reset_calls"] > 0, info
    if form in LEVEL_FORMS and state is not None:
        n = state.shape[1]
        noise_free = P[state, actions] if P.ndim == 2 else P[np.arange(n)[None, :], state, actions]
        noisy = seen & (next_state != noise_free)
        assert (tn == 0).any() and not noisy[:, tn == 0].any(), "level 0 made a noisy transition"
        assert noisy[:, tn > 0.05].any(), "no noisy transition at all"
