"""What tests/test_gpu_closed_forms_shapes.py runs and what it asserts about its own coverage, shared with
tests/test_closed_forms_shapes_host.py, which shows on the CPU (32 envs, the oracle env in a closed loop with the restatement)
that those conditions can be met before any GPU run, and works the LDS placements out by hand.

tests/test_gpu_closed_loop_shapes.py took the closed-loop kernels off the square 8 x 8 MDP; four families of kernel forms came
after it and each brought tests on square, short-history MDPs again:
    pm        one MDP per env: set_learner(..., per_env_mdp=True) on a seeds=[...] / mdps=[...] handle (PM=1 / PM=2)
    nlev      per-env noise levels on a shared MDP: set_noise_levels (NLEV=1)
    pm_nlev   both at once (NLEV=1,PM=...)
    sched     per-episode epsilon / alpha schedules on a shared MDP (SCHED=1)
The cases below are the smallest shapes that reach what those forms added and that is shape-dependent; the table says what
each one is for and which forms run it.  N = 320, K = 37, two launches, env_id_offset = 1000, as in the files extended.

Everything shared is imported: the configs' makers, the LDS carve and the delay-line / learner conditions from
closed_loop_shape_cases, the per-env set-up and CPU loop from per_env_mdp_cpu, the seven level pairs and the levelled CPU loop
from noise_seed_cases, the schedules from learner_schedule_cases / _ref / _cpu.

Seeds.  A shared-MDP form runs a case on the config's seed, a per-env form on the seeds base ... base + N - 1.  As in
closed_loop_shape_cases every case was tried on the CPU (32 envs) from seed 0 upwards -- per-env: from base 100 upwards in
steps of N -- and the first under which every condition below holds for every (form, algorithm) the case runs was kept:
SHARED_SEED and PER_ENV_BASE list them with the seeds tried before and why they were passed over."""
import numpy as np

import closed_loop_shape_cases as shp
import eval_summary_ref as eref
import learner_schedule_cases as lsc
import learner_sweep_ref as ref
import noise_seed_cases as nsc
import per_env_mdp_cpu as pm

N, K, LAUNCHES, OFF = pm.N, pm.K, pm.LAUNCHES, pm.OFF
SEED, PHILOX_SEED = pm.SEED, pm.PHILOX_SEED
ALPHA, GAMMA, EPS = pm.ALPHA, pm.GAMMA, pm.EPS
ALGOS = pm.ALGOS
PAIRS, CREATED = nsc.PAIRS, nsc.CREATED
level_arrays, pairs_present = nsc.level_arrays, nsc.pairs_present
_gen, _custom, shape_of = shp._gen, shp._custom, shp.shape_of
assert (K, LAUNCHES, SEED) == (shp.K, shp.LAUNCHES, shp.SEED) == (lsc.K, lsc.LAUNCHES, lsc.SEED)
assert (ALPHA, GAMMA, EPS) == (shp.ALPHA, shp.GAMMA, shp.EPS)

_MATRIX_KEYS = ("transition_function", "reward_function", "terminal_states", "init_state_dist")


class CustomPerSeed:
    """per_env_mdp_cpu.build_mdps' "per_env_cfg": env of seed s has its own closed_loop_shape_cases._custom matrices, drawn
    from numpy seed s (so a shard of the seeds has the whole's matrices)"""

    def __init__(self, S, A, terminal):
        self.S, self.A, self.terminal = S, A, tuple(terminal)

    def __call__(self, s):
        c = _custom(self.S, self.A, self.terminal, s)
        return {k: c[k] for k in _MATRIX_KEYS}

    def __repr__(self):
        return "CustomPerSeed(%d, %d, %r)" % (self.S, self.A, self.terminal)


def _custom_per_env(S, A, terminal, **kw):
    c = {k: v for k, v in _custom(S, A, terminal, 0, **kw).items() if k not in _MATRIX_KEYS}
    return dict(c, per_env_cfg=CustomPerSeed(S, A, terminal))


# case -> config.  The "seed" key is the shared-MDP forms'; per-env handles drop it (per_env_cfg).
CASES = {
    "d2_s12_a6_L2": _gen(12, 6, L=2, delay=1, diameter=2),               # S = 2 A; 224 B per lane: slots 56 KiB + Q 72 KiB: PM=2,QLDS=1; A < 8
    "d4_s24_a6": _gen(24, 6, diameter=4),                                # 384 B per lane: PM=1; Q 144 KiB; cdfs of 22.5 / 31.5 KiB against Q
    "custom_5x3": _custom_per_env(5, 3, (3,), delay=2),                  # rew_sa keys read from the slots; 208 B per lane: PM=2,UNIT=0; key ring
    "custom_13x12": _custom_per_env(13, 12, (3, 7), delay=2),            # rew_sa through a.rtable + i S A in global memory (PM=1); S, A coprime
    "custom_13x12_noise": _custom(13, 12, (3, 7), 131),                  # (shared MDP) NLEV with rew_sa: s' moves, the reward does not
    "s4_L4": _gen(4, 4, L=4, delay=2, repeats_in_sequences=True),        # history byte 4 in a PM=2 slot handle (96 B per lane); reward bits beyond byte 0
    "s2_L7": _gen(2, 2, L=7, repeats_in_sequences=True),                 # the gate at byte 7 with PM=2 (64 B per lane, 16 B of reward bits)
    "s4_L7": _gen(4, 4, L=7, delay=2, repeats_in_sequences=True),        # rbits_stride = 2 KiB per env in global memory (PM=1)
    "delay32_affine": dict(shp.CASES["delay32_affine"][0]),              # ringbits >> 31; scale / shift / terminal reward / every-n (under per-env sigma)
    "delay33": _gen(8, 8, delay=33),                                     # UNIT=0 key ring of 33 rows, one set of 8 doubles per lane (208 B: PM=2)
    "a1_s3": _gen(3, 1, diameter=3),                                     # A = 1; no terminal state; a schedule whose counter never moves
    "s255_a85": _gen(255, 85, diameter=3),                               # state byte 0xFE; PM=1 with 21 KiB of P per env; cdfs of 2.5 MB in global memory
    "s10": _gen(10, 10), "s11": _gen(11, 11), "s12": _gen(12, 12),        # the placement edges (see pm_expected)
    "trunc_same": _gen(12, 6, L=2, delay=1, diameter=2),                 # d2_s12_a6_L2 with max_episode_steps = 5 ...
    "trunc_next": _gen(12, 6, L=2, delay=1, diameter=2),
    "trunc_disabled": _gen(12, 6, L=2, delay=1, diameter=2),
}
KW = {c: {} for c in CASES}
KW.update(trunc_same=dict(max_episode_steps=5), trunc_next=dict(max_episode_steps=5, autoreset="next_step"),
          trunc_disabled=dict(max_episode_steps=5, autoreset="disabled"))

RECT = ("d2_s12_a6_L2", "d4_s24_a6", "custom_5x3", "custom_13x12", "custom_13x12_noise", "s255_a85", "a1_s3", "trunc_same", "trunc_next", "trunc_disabled")
REW_SA = ("custom_5x3", "custom_13x12", "custom_13x12_noise")
LONG_L = ("s4_L4", "s2_L7", "s4_L7")
KEY_64 = ("s4_L4", "s2_L7")                  # a rewarded key >= 64: a reward bit beyond byte 7 of the table
DELAY_LINE = ("delay32_affine", "delay33")
TRUNC = ("trunc_same", "trunc_next", "trunc_disabled")
NO_TERMINAL = ("a1_s3", "s2_L7")              # terminal_state_density 0.25 of one action, or of two states: no terminal state
NO_Q_FLOOR = ("a1_s3",) + DELAY_LINE         # (closed_loop_shape_cases.learner_honest's exemptions, for its reasons)

# (Host-built per-env MDPs of S = 255 -- the restatement and the CPU loop need them, whoever built the handle's -- take 10.7 s for
# the 320 seeds, measured on one core, within the 20 s the set-up allows, once per session: s255_a85 runs at N = 320 like the others.)

# ---- which form runs which case on which (algorithm, stream).  The economy of closed_loop_shape_cases.STREAMS: q_learning on
# both streams, sarsa and double_q on one each; the cases with slow restatements (s255_a85 and everything with noise levels:
# seven uniform twins per case) one algorithm per stream
_FULL = (("q_learning", "numpy"), ("q_learning", "philox"), ("sarsa", "numpy"), ("double_q", "philox"))
_Q2 = (("q_learning", "numpy"), ("q_learning", "philox"))
_NOISE_A = (("q_learning", "numpy"), ("sarsa", "philox"))
_NOISE_B = (("double_q", "numpy"), ("q_learning", "philox"))
FORMS = {
    "pm": {"d2_s12_a6_L2": _FULL, "d4_s24_a6": _FULL, "custom_5x3": _FULL, "custom_13x12": _FULL, "s4_L4": _FULL, "s2_L7": _FULL, "s4_L7": _FULL,
           "delay32_affine": _FULL, "delay33": _FULL, "a1_s3": _FULL, "s255_a85": _Q2, "s10": _Q2[:1], "s11": _Q2[:1], "s12": _Q2[:1],
           "trunc_same": _FULL},
    "pm_nlev": {"d2_s12_a6_L2": _NOISE_A, "d4_s24_a6": _NOISE_B, "custom_5x3": _NOISE_B, "custom_13x12": _NOISE_A, "s4_L4": _NOISE_A,
                "delay32_affine": _NOISE_B, "s10": _NOISE_A[:1], "s11": _NOISE_A[:1], "s12": _NOISE_A[:1], "trunc_next": _NOISE_A},
    "nlev": {"d2_s12_a6_L2": _NOISE_B, "d4_s24_a6": _NOISE_A, "custom_13x12_noise": _NOISE_A, "s4_L7": _NOISE_B, "delay32_affine": _NOISE_A,
             "a1_s3": _NOISE_B, "s255_a85": _NOISE_A},
    "sched": {"d2_s12_a6_L2": _FULL, "d4_s24_a6": _FULL, "s4_L4": _FULL, "delay33": _FULL, "a1_s3": _FULL, "trunc_disabled": _FULL},
}
RUNS = {form: [(c, a, r) for c, pairs in cs.items() for a, r in pairs] for form, cs in FORMS.items()}
PER_ENV_FORMS = ("pm", "pm_nlev")
# the whole launch predicted on the CPU (Philox streams): every Philox run of the per-env forms (as the files extended do), and
# two cases each of the shared-MDP forms
CPU_LOOP_SHARED = {"nlev": ("custom_13x12_noise", "s4_L7"), "sched": ("d2_s12_a6_L2", "trunc_disabled")}

# ---- seeds
# shared-MDP forms: the config's seed.  0 unless listed: (seed, the seeds tried before it and why they were passed over)
SHARED_SEED = {
    "d4_s24_a6": (2, "0, 1: under a schedule the step-row envs end at most two episodes, so no table length has one of them at its last entry and another env short of it"),
    "s4_L4": (7, "0, 1: the step-row envs of q_learning and double_q end no episode at all; 2 ... 6: the tables of at most half the envs moved, or no table length meets the schedule's counts for every run"),
    "delay32_affine": (1, "0: under greedy evaluation no reward leaves the delay line in the sigma == 0 envs of 32"),
    "delay33": (6, "0 ... 2, 5: no reward leaves the delay line; 3, 4: no table length meets the four counts of the schedule for every run"),
}
# per-env forms: seeds base ... base + n - 1
PER_ENV_BASE = {
    "delay32_affine": (420, "100: under greedy evaluation with levels no reward leaves the delay line in the sigma == 0 envs of 32"),
    "s4_L7": (420, "100 (at 74 steps per launch; at 37 none of 100, 420 ... 2340): the tables of at most half the envs moved"),
}
# steps per launch where 37 leave a floor out of reach (K is raised for a case, never a floor lowered).  A sequence of 4 or 7
# states is rarely paid from all-zero tables.  s4_L7: see PER_ENV_BASE.  s4_L4 at 37 steps: under bases 100 and 420 the tables of
# at most half the 32 CPU envs moved, and under 740, which met that, 158 of the device's 320 envs on numpy streams did -- two
# short of more than half; at 74 steps base 100 meets it everywhere (200 of 320 on the CPU's Philox streams)
K_OF = {("pm", "s4_L7"): 74, ("pm", "s4_L4"): 74}


def shared_cfg(case):
    return dict(CASES[case], seed=SHARED_SEED.get(case, (0,))[0])


def per_env_cfg(case):
    """the config of a per-env handle: no "seed" key"""
    return {k: v for k, v in CASES[case].items() if k != "seed"}


def seeds_of(case, n=None, lo=0):
    base = PER_ENV_BASE.get(case, (100,))[0]
    return list(range(base + lo, base + lo + (N if n is None else n)))


def handle_cfg(cfg, seeds):
    """what RLToyVectorEnv takes beside seeds=: the config, and mdps=[...] where the envs differ by more than the seed"""
    if "per_env_cfg" not in cfg:
        return cfg, {}
    base = {k: v for k, v in cfg.items() if k != "per_env_cfg"}
    return dict(base, **cfg["per_env_cfg"](seeds[0])), dict(mdps=pm.build_mdps(cfg, seeds))


# ---- the schedules of the SCHED cases: learner_schedule_cases' four rows, M chosen per case from its own CPU episode counts
# under the schedule (32 envs, 2 x 37 steps; every M in the range given met the four counts for every run of the case, the one
# near the median was kept) so that some envs run past the table's end and some stop short of its last entry
SCHED_M = {
    "d2_s12_a6_L2": 12,             # 1 - 27 episodes per env, median 10 - 15 by algorithm (any M of 3 ... 24 meets the counts)
    "d4_s24_a6": 15,                # (seed 2) 6 - 34 per env, median 15 (8 ... 25)
    "s4_L4": 5,                     # (seed 7) 0 - 25 per env, median 4 (2 ... 7)
    # delay33 (seed 6): a reward leaves a delay line of 33 only in an episode of 34 steps or more, so the MDP has to let episodes
    # run on, and a step-row env -- which may not explore before its last entry -- ends two episodes at the most: a table that
    # schedules epsilon has 3 entries (2 or 3 meet the counts), one that schedules alpha alone 9 (2 - 16 episodes per env: 4 ... 16)
    "delay33": {"eps": 3, "both": 3, "alpha": 9},
    "a1_s3": 4,                     # no terminal state, no truncation: the counter stays 0 on every env (the stated exemption)
    "trunc_disabled": 6,            # autoreset disabled: the counter moves at every step from the fifth on (learner_schedule_cases.BELOW_M_EXEMPT)
}
# learner_schedule_cases.honest goes by its own handles' names; a case here borrows the one that has its exemption
_SCHED_ALIAS = {"trunc_disabled": "cfg2_disabled_max5"}


def sched_m(case, kind):
    m = SCHED_M[case]
    return m[kind] if isinstance(m, dict) else m


def sched_kind(case, algo, rng):
    return lsc.KINDS[(list(SCHED_M).index(case) + lsc.ALGOS.index(algo) + lsc.RNGS.index(rng)) % 3]


def sched_honest(case, algo, kind, info, ep, row):
    if case == "a1_s3":
        assert not np.asarray(ep).any(), ep                  # nothing ends an episode: the counter never moves ...
        assert info["updates"] > 0 and info["E_changes"] == 0 and info["alpha_changes"] == 0, info
        return
    lsc.honest(_SCHED_ALIAS.get(case, "s20"), algo, kind, sched_m(case, kind), info, ep, row)


# ---- the LDS placements, restated from the carve numbers (include/mdpp.h; closed_agent_lds of
# mdpp_discrete_closed.hpp, on a shared MDP and on one MDP per env, without and with levels)
ZIG_BYTES = 3 * 256 * 8              # a NOISE kernel's static LDS; 24 bytes otherwise (closed_loop_shape_cases.static_lds)
Q_BOUND, SLOT_BOUND, CDF_BOUND = 160 * 1024, 64 * 1024, 32 * 1024


def _plain(cfg):
    return {k: v for k, v in cfg.items() if k not in ("transition_noise", "reward_noise", "per_env_cfg", "seed")}


def lane_bytes(cfg):
    """a lane's MDP slot: the carve without a noise cdf"""
    return shp.lds_bytes(_plain(cfg))


def cdf_bytes(cfg, levels):
    S = shape_of(cfg)[0]
    return (levels * S * S * 8 + 15) // 16 * 16


def _granted(static, dynamic, limit):
    """dynamic_lds_ok: up to 32 KiB of dynamic LDS is never asked about"""
    return dynamic <= 32 * 1024 or static + dynamic <= limit


def pm_expected(cfg, double, limit, options=()):
    """(QLDS, PM) of a per-env handle without levels: Q and the slots, Q alone, the slots alone, neither.  cfg with its noise
    keys if the handle has them: the shared cdf (within 32 KiB) is in every sum, the ziggurat tables are static"""
    noise = "transition_noise" in cfg or "reward_noise" in cfg
    static = ZIG_BYTES if noise else 24
    slots, q = 256 * lane_bytes(cfg), shp.q_lds(cfg, double)
    S = shape_of(cfg)[0]
    fixed = (S * S * 8 + 15) // 16 * 16 if "transition_noise" in cfg and S * S * 8 <= 32 * 1024 else 0
    m_ok = slots <= SLOT_BOUND and "NO_PM_LDS" not in options
    q_ok = q <= Q_BOUND and "NO_LEARN_LDS" not in options
    if q_ok and m_ok and _granted(static, fixed + slots + q, limit):
        return 1, 2
    if q_ok and _granted(static, fixed + q, limit):
        return 1, 1
    if m_ok and _granted(static, fixed + slots, limit):
        return 0, 2
    return 0, 1


def pm_nlev_expected(cfg, double, rng, limit, options=(), levels=5):
    """(QLDS, PM, cdfs staged) of a per-env handle with levels: the first of {Q, slots, cdfs}, {Q, slots}, {Q, cdfs}, {Q},
    {slots, cdfs}, {slots}, {cdfs}, {} that is allowed and fits beside the ziggurat tables"""
    size = dict(q=shp.q_lds(cfg, double), m=256 * lane_bytes(cfg), c=cdf_bytes(cfg, levels))
    ok = dict(q=size["q"] <= Q_BOUND and "NO_LEARN_LDS" not in options, m=size["m"] <= SLOT_BOUND and "NO_PM_LDS" not in options,
              c=rng == "numpy" and size["c"] <= CDF_BOUND and "NO_PM_NLEV_LDS" not in options)
    for subset in ("qmc", "qm", "qc", "q", "mc", "m", "c", ""):
        if all(ok[k] for k in subset) and (subset == "" or _granted(ZIG_BYTES, sum(size[k] for k in subset), limit)):
            return int("q" in subset), 2 if "m" in subset else 1, "c" in subset
    raise AssertionError("the empty subset is always taken")


def nlev_expected(cfg, double, rng, limit, options=(), levels=5):
    """(QLDS, cdfs staged) of a shared-MDP handle with levels (created with both noise keys: its own cdf keeps its room in the
    carve): both, Q alone, the cdfs alone, neither"""
    created = dict(_plain(cfg), **CREATED)
    carve, q, cdf = shp.lds_bytes(created), shp.q_lds(cfg, double), cdf_bytes(cfg, levels)
    q_ok = q <= Q_BOUND and "NO_LEARN_LDS" not in options
    c_ok = rng == "numpy" and cdf <= CDF_BOUND and "NO_NLEV_LDS" not in options
    if q_ok and c_ok and _granted(ZIG_BYTES, carve + cdf + q, limit):
        return 1, True
    if q_ok and _granted(ZIG_BYTES, carve + q, limit):
        return 1, False
    if c_ok and _granted(ZIG_BYTES, carve + cdf, limit):
        return 0, True
    return 0, False


def kernel_name(kind, form, cfg, algo, rng, qlds, pmv=None, summary=False):
    """the name the library reports: the template arguments in template order"""
    dbl = algo == "double_q"
    noise = form in ("nlev", "pm_nlev") or "reward_noise" in cfg or "transition_noise" in cfg
    head = "PHILOX=%d,NOISE=%d,UNIT=%d,QLDS=%d" % (rng == "philox", noise, shape_of(_plain(cfg))[4], qlds)
    tail = (",NLEV=1" if form in ("nlev", "pm_nlev") else "") + (",PM=%d" % pmv if form in PER_ENV_FORMS else "")
    stem = "summary" if summary else "rollout"
    if kind == "learn":
        return "k_discrete_learn_%s<%s,PE=1%s%s%s>" % (stem, head, ",DOUBLE=1" if dbl else "", tail, ",SCHED=1" if form == "sched" else "")
    return "k_discrete_eval_%s<%s,DOUBLE=%d%s>" % (stem, head, dbl, tail)


# ---- honesty conditions
# per-env floors (per_env_mdp_cpu.FLOORS' kind): (envs with non-zero Q in all, ... in each workgroup's lanes, envs that
# terminate at least once), beside the values measured on the CPU with exactly the GPU set-up (Philox streams, q_learning; the
# other algorithms within a few envs of them)
_F = {   # case: pm floor (measured: all, lanes 0-255, lanes 256-319, terminated), pm_nlev floor (measured)
    "d2_s12_a6_L2": ((250, 48, 300), (297, 237, 60, 318), (280, 50, 300), (317, 254, 63, 319)),
    "d4_s24_a6": ((290, 52, 300), (320, 256, 64, 319), (290, 52, 300), (320, 256, 64, 320)),
    "custom_5x3": ((290, 52, 230), (320, 256, 64, 274), (290, 52, 260), (320, 256, 64, 301)),
    "custom_13x12": ((290, 52, 290), (320, 256, 64, 316), (290, 52, 300), (320, 256, 64, 319)),
    "s4_L4": ((170, 32, 300), (200, 160, 40, 320), (240, 44, 300), (278, 221, 57, 320)),                    # (pm: at 74 steps per launch)
    "s2_L7": ((220, 40, 0), (260, 209, 51, 0), None, None),                              # (no terminal state)
    "s4_L7": ((150, 28, 300), (181, 146, 35, 320), None, None),                          # (at 74 steps per launch)
    "delay32_affine": ((290, 52, 300), (320, 256, 64, 320), (290, 52, 300), (320, 256, 64, 320)),
    "delay33": ((12, 4, 300), (19, 11, 8, 319), None, None),                             # (few rewards leave a delay line of 33 in 74 steps)
    "a1_s3": ((290, 52, 0), (320, 256, 64, 0), None, None),                              # (no terminal state)
    "s255_a85": ((290, 52, 300), (320, 256, 64, 320), None, None),
    "s10": ((290, 50, 290), (320, 256, 64, 316), (290, 50, 300), (320, 256, 64, 319)),
    "s11": ((290, 50, 290), (319, 255, 64, 312), (290, 50, 300), (320, 256, 64, 318)),
    "s12": ((290, 50, 290), (316, 254, 62, 320), (290, 50, 300), (319, 256, 63, 320)),
    "trunc_same": ((220, 40, 300), (261, 211, 50, 319), None, None),
    "trunc_next": (None, None, (260, 48, 300), (301, 241, 60, 318)),
}
FLOORS = {(form, c): v[j] for c, v in _F.items() for form, j in (("pm", 0), ("pm_nlev", 2)) if v[j] is not None}
MEASURED = {(form, c): v[j] for c, v in _F.items() for form, j in (("pm", 1), ("pm_nlev", 3)) if v[j] is not None}


def learner_honest(case, algo, info, Q, Q0=None):
    """closed_loop_shape_cases.learner_honest, which goes by its own cases' names: a case here borrows the name there that has
    its exemptions (A = 1: strict choices only; a1_s3 and the delay-line cases: no floor on moved tables; truncation with
    sarsa's dropped carry).  trunc_next is not held to the dropped carry: closed_loop_shape_cases.SARSA_DROP_SHOWS says why it
    shows under next-step autoreset only where s' == s, and no state of these MDPs that is acted from leads to itself (asserted on
    the host); the
    same-step case trunc_same carries that condition.  trunc_disabled has no floor on moved tables either (it borrows delay33's
    name): nothing resets, so within a few steps nearly every env sits in a terminal state (over 250 of 320 at the end, under
    every seed of 0 ... 5) and is paid nothing more -- at most 155 of 320 tables move, at 37 steps per launch as at 74"""
    alias = case if case in NO_Q_FLOOR else "s8_noise_max5_next" if case == "trunc_same" else "delay33" if case == "trunc_disabled" else "a9"
    shp.learner_honest(alias, algo, info, Q, Q0)
    if case in TRUNC:
        assert info["trunc_resets"] > 0 or KW[case].get("autoreset") == "disabled", info


def flow(state, actions, obs, reward, term, trunc, autoreset, P):
    """the steps of a pass as a dict of [T, n] arrays: reset_call, live, next_state (the true one where an output or the
    noise-free P tells it, else P[s, a]), seen (next_state is known to be true).  P [S, A] or [n, S, A]"""
    term, trunc = np.asarray(term, bool), np.asarray(trunc, bool)
    rc, _ = eref.reset_calls(term, trunc, autoreset)
    live = ~rc
    n = state.shape[1]
    noise_free = P[state, actions] if P.ndim == 2 else P[np.arange(n)[None, :], state, actions]
    hidden = (term | trunc) & (autoreset == ref.SAME_STEP)            # obs is the next episode's first state
    return dict(state=state, actions=actions, obs=obs, reward=reward, term=term, trunc=trunc, reset_call=rc, live=live,
                next_state=np.where(hidden | rc, noise_free, obs), seen=live & ~hidden, noise_free=noise_free)


def paid_keys(f, S, L, delay, autoreset):
    """the reward-table keys of the steps that paid (reward != 0), rebuilt from the states of the episode so far: the L
    states that end `delay` steps before the step's next state, first state most significant.  Noise-free passes only."""
    T, n = f["state"].shape
    keys = []
    for i in range(n):
        seq = [int(f["state"][0, i])]
        for t in range(T):
            if f["reset_call"][t, i]:
                seq = [int(f["obs"][t, i])]
                continue
            seq.append(int(f["next_state"][t, i]))
            if f["reward"][t, i] != 0 and len(seq) >= L + delay:
                k = 0
                for s in seq[len(seq) - delay - L:len(seq) - delay]:
                    k = k * S + s
                keys.append((i, t, k))
            if (f["term"][t, i] or f["trunc"][t, i]) and autoreset == ref.SAME_STEP:
                seq = [int(f["obs"][t, i])]
    return keys


def flow_honest(case, form, cfg, f, mdps, autoreset=ref.SAME_STEP, tn=None, rn=None):
    """what the steps of a learner's pass must have shown.  f: flow(); mdps: the MDP of every env (one: shared)"""
    S, A, L = shape_of(_plain(cfg))[:3]
    live, state, act = f["live"], f["state"], f["actions"]
    n = state.shape[1]
    per_env = len(mdps) > 1
    if case in NO_TERMINAL:
        assert not f["term"].any()
    else:
        assert (f["term"] & live).any()
    if case in RECT:
        assert S > A and (state[live] >= A).any()
        assert (state[live] * A + act[live] != state[live] * S + act[live]).any()
    quiet = np.ones(n, bool) if rn is None else rn == 0                  # the envs whose rewards carry no noise
    if case == "delay33":
        shp.delay_line_honest(cfg, f["reward"], f["reset_call"])
    # (delay32_affine: a learner ends its episodes long before a reward leaves a line of 32, under every form -- the longest of
    # 320 envs x 74 steps ran 29 steps; evaluation shows the line: EVAL_RUNS and eval_flow_honest)
    if case in LONG_L:
        assert (f["reward"][:, quiet][live[:, quiet]] != 0).any()        # (no shift, no noise: the gate has opened and a key has hit)
    if case in KEY_64 and form in ("pm", "sched"):
        keys = paid_keys(f, S, L, cfg["delay"], autoreset)
        assert keys
        for i, t, k in keys:                             # (the rebuilt key is a rewarded key of the env's own table)
            assert mdps[i if per_env else 0].reward_table()[k] != 0, (i, t, k)
        assert max(k for _, _, k in keys) >= 64
    if per_env:
        P = np.stack([np.asarray(m.P) for m in mdps])
        if case == "a1_s3":                               # (one action, diameter 3: the one chain 0 -> 1 -> 2 -> 0 under every seed)
            assert (P == P[0]).all()
        else:
            assert (P[:, state, act] != f["noise_free"][None])[:, live].any()      # two envs' P differ at an (s, a) one of them visited
    if case in REW_SA:
        R = np.stack([np.asarray(m.reward_matrix) for m in mdps])
        d = cfg.get("delay", 0)
        if per_env and form == "pm":
            # two envs that took the same (s, a) and were paid differently for it (the reward arrives d steps later, within the episode)
            key = state * A + act
            paid = {}
            ended = f["term"] | f["trunc"] | f["reset_call"]
            for t in range(d, state.shape[0]):
                ok = ~ended[t - d:t].any(axis=0) & live[t] & live[t - d]
                for i in np.flatnonzero(ok):
                    paid.setdefault(int(key[t - d, i]), set()).add(float(f["reward"][t, i]))
            assert any(len(v) > 1 for v in paid.values())
        if form in ("nlev", "pm_nlev"):
            # an env without reward noise, a step of it whose s' is not the noise-free P[s, a], and the reward it was paid for that
            # (s, a) d steps later: R(s, a) all the same
            moved = f["seen"] & (f["next_state"] != f["noise_free"]) & (rn == 0)[None, :]
            ended = f["term"] | f["trunc"] | f["reset_call"]
            hits = 0
            for t, i in zip(*np.nonzero(moved)):
                if t + d < state.shape[0] and not ended[t:t + d, i].any() and live[t + d, i]:
                    want = np.float32(R[i if per_env else 0][state[t, i], act[t, i]])
                    assert f["reward"][t + d, i] == want, (t, i, f["reward"][t + d, i], want)
                    hits += 1
            assert hits > 0
    if case in TRUNC:
        cut = live & f["trunc"] & ~f["term"]
        assert cut.any()
        if autoreset == ref.NEXT_STEP:
            assert (f["reset_call"][1:] & cut[:-1]).any()    # a reset call right after a truncation
    if form in ("nlev", "pm_nlev"):
        levels_honest(tn, rn)
        noisy = f["seen"] & (f["next_state"] != f["noise_free"])
        assert not noisy[:, tn == 0].any(), "level 0 made a noisy transition"
        if S > 1 and case != "a1_s3":
            for p in sorted(set(nsc.TN) - {0.0, 0.01, 0.02}):       # (the two smallest levels: a handful of draws, no floor)
                assert noisy[:, tn == p].any(), ("no noisy transition at level", p)


def levels_honest(tn, rn):
    """all seven pairs in every wave of 64 lanes, and in each a lane of level 0 (no space-stream draw) beside one that draws"""
    n = len(tn)
    for lo in range(0, n, 64):
        hi = min(lo + 64, n)
        if hi - lo >= 7:
            assert len(pairs_present(tn[lo:hi], rn[lo:hi])) == 7
        if hi - lo >= 2:
            z = tn[lo:hi] == 0
            assert (z[1:] & ~z[:-1]).any() or (z[:-1] & ~z[1:]).any()


def check_floors(case, form, Q, terminated, what=""):
    total, per_wg, term_floor = FLOORS[(form, case)]
    nz = pm.nonzero_envs(Q)
    counts = (int(nz.sum()), int(nz[:256].sum()), int(nz[256:].sum()), int(np.asarray(terminated).any(axis=0).sum()))
    assert counts[0] >= total and counts[1] >= per_wg and (len(nz) <= 256 or counts[2] >= per_wg) and counts[3] >= term_floor, (what, case, counts)
    return counts


# ---- further tests of the GPU file
# rollout_eval from tie-laden random tables and the summary= forms: (form, case, algorithm, stream).  delay32_affine is here for
# the delay line: greedy walks of random tables miss the terminal states long enough for a reward to leave a line of 32
# (closed_loop_shape_cases.DELAY_LINE_UNDER_EVALUATION_ONLY), which no learner's episode does
EVAL_RUNS = [("pm", c, a, r) for c in ("d2_s12_a6_L2", "custom_5x3", "custom_13x12", "s4_L4", "trunc_same", "delay32_affine")
             for a, r in (("q_learning", "numpy"), ("double_q", "philox"))] + [
    ("pm_nlev", "d2_s12_a6_L2", "q_learning", "numpy"), ("pm_nlev", "custom_5x3", "double_q", "numpy"), ("pm_nlev", "custom_13x12", "double_q", "philox"),
    ("pm_nlev", "s4_L4", "q_learning", "philox"), ("pm_nlev", "trunc_next", "q_learning", "numpy"), ("pm_nlev", "delay32_affine", "q_learning", "philox"),
    ("nlev", "d2_s12_a6_L2", "double_q", "numpy"), ("nlev", "custom_13x12_noise", "q_learning", "philox"), ("nlev", "delay32_affine", "double_q", "numpy")]
DOUBLE_PM2 = ("custom_5x3", "s4_L4", "s2_L7")        # Q fits twice beside the slots: DOUBLE=1 with PM=2
N_EDGES = shp.N_EDGES


def eval_tables(cfg, n, double):
    S, A = shape_of(_plain(cfg))[:2]
    return shp.tie_q(shp.random_q(shp.Q_SEED, n, S, A, double))


# ---- the CPU closed loops (Philox streams), one call for every form
def mdps_of(form, case, n=None, lo=0):
    """the MDP of every env of the case's handle under a form (a shared-MDP form: a list of one)"""
    if form in PER_ENV_FORMS:
        return pm.build_mdps(per_env_cfg(case), seeds_of(case, n, lo))
    return pm.build_mdps(_plain(CASES[case]), [shared_cfg(case)["seed"]])


def cpu_loop(form, case, algo, n=None, k=None, rng="philox"):
    """The whole of both launches predicted without a GPU: (Q, traj, extra) with traj as closed_loop_cpu.closed_loop's and
    extra the levels (tn, rn) or the scheduled Agent.  pm: per_env_mdp_cpu.closed_loop; nlev / pm_nlev:
    noise_seed_cases.closed_loop (a shared MDP: every env on the config's seed); sched: learner_schedule_cpu.closed_loop"""
    import learner_schedule_cpu as scpu
    k = K_OF.get((form, case), K) if k is None else k
    kw = KW[case]
    n = N if n is None else n
    if form == "pm":
        _, Q, traj = pm.closed_loop(per_env_cfg(case), kw, algo, ALPHA, GAMMA, EPS, seeds_of(case, n), K=k)
        return Q, traj, None
    if form in ("nlev", "pm_nlev"):
        tn, rn = level_arrays(n)
        per_env = form == "pm_nlev"
        cfg = per_env_cfg(case) if per_env else _plain(CASES[case])
        seeds = seeds_of(case, n) if per_env else [shared_cfg(case)["seed"]] * n
        _, Q, traj = nsc.closed_loop(cfg, kw, algo, tn, rn, seeds=seeds, K=k)
        return Q, traj, (tn, rn)
    assert form == "sched"
    kind = sched_kind(case, algo, rng)                   # (rng: whose run's kind of schedule; the loop's streams are Philox streams)
    agent, traj = scpu.closed_loop(shared_cfg(case), kw, algo, ALPHA, GAMMA, EPS, lsc.schedule(kind, sched_m(case, kind), n), n,
                                   seed=SEED, K=k, launches=LAUNCHES, philox_seed=PHILOX_SEED, off=OFF)
    return agent.Q, traj, agent


def states_of(traj):
    """the state every step was acted from"""
    return np.concatenate([traj["obs0"][None], traj["obs"][:-1]])


def eval_flow_honest(form, case, info, double, reward, reset_call, rn=None):
    """what an evaluation pass must have shown: eval_summary_cases.eval_honest's counts, and on delay32_affine a reward that
    came out of the delay line -- read on rewards that carry no noise (all envs, or the sigma == 0 envs of a levelled handle)"""
    shp.evalc.eval_honest(info, double)
    if case in DELAY_LINE:
        quiet = np.ones(reward.shape[1], bool) if rn is None else rn == 0
        assert quiet.any()
        shp.delay_line_honest(_plain(CASES[case]), reward[:, quiet], reset_call[:, quiet])


def cpu_eval_loop(form, case, double, n):
    """greedy evaluation of eval_tables on the CPU (Philox streams), under a form's handle (levels: env i at its pair): (info as
    eval_summary_ref.new_info, episodes ended, reward float32 [T, n], reset_call [T, n], rn or None)"""
    from closed_loop_cpu import make_oracles
    kw = KW[case]
    autoreset, max_steps = kw.get("autoreset", ref.SAME_STEP), kw.get("max_episode_steps", 0)
    tn = rn = None
    if form == "pm":
        mdps = mdps_of("pm", case, n)
    else:
        tn, rn = level_arrays(n)
        per_env = form == "pm_nlev"
        mdps = nsc.level_mdps(per_env_cfg(case) if per_env else _plain(CASES[case]), tn, rn, seeds_of(case, n) if per_env else [shared_cfg(case)["seed"]] * n)
    envs = [make_oracles(m, 1, PHILOX_SEED, OFF + i)[0] for i, m in enumerate(mdps)]
    Q = eval_tables(CASES[case], n, double)
    s = np.array([o.reset() for o in envs], np.int64)
    steps, pending, info, ended = np.zeros(n, np.int64), np.zeros(n, bool), eref.new_info(), 0
    T = LAUNCHES * K
    reward, reset_call = np.zeros((T, n), np.float32), np.zeros((T, n), bool)
    for t in range(T):
        a = eref.greedy(Q, s, info, ~pending)
        reset_call[t] = pending
        info["reset_calls"] += int(pending.sum())
        for i in range(n):
            if pending[i]:                               # (a next-step reset call takes a tick of its own: per_env_mdp_cpu.closed_loop)
                envs[i].set_philox(PHILOX_SEED, OFF + i, t + 1, 1)
                s[i], steps[i], pending[i] = envs[i].reset(explicit=False), 0, False
                continue
            o, r, te = envs[i].step(int(a[i]))
            reward[t, i] = np.float32(r)
            steps[i] += 1
            info["terminations"] += int(te)
            if te or (max_steps and steps[i] >= max_steps):
                ended += 1
                if autoreset == ref.SAME_STEP:
                    o, steps[i] = envs[i].reset(explicit=False), 0
                else:
                    pending[i] = autoreset == ref.NEXT_STEP
            s[i] = o
    return info, ended, reward, reset_call, rn
