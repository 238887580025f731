"""What tests/test_gpu_closed_loop_shapes.py runs and what it asserts about its own coverage, shared with
tests/test_closed_loop_shapes_host.py, which shows on the CPU (32 envs, the oracle env in a closed loop with the restatement,
tests/closed_loop_cpu.py) that those conditions can be met before any GPU run.

The closed-loop kernels (policy, learners, greedy evaluation, summaries) were tested on square MDPs of 8, 20, 50 or 70 states
with sequence_length <= 3, and never with a truncation that resets.  The cases here are the shapes and edges those tests do
not reach; the table says what each one is for.  N = 320, K = 37, two launches, as in the tests they extend.

MDP seeds: every generated case was tried on the CPU from seed 0 upwards (cfg2: the seed 40 the other tests use) and the
first seed whose 32-env closed loop meets every condition below -- the three learners, per-env parameters, evaluation of one and
two tables, the summaries -- was kept: seed 0 everywhere but s4_L7 (4: under seeds 0 ... 3 no evaluated episode of the summary pass
ran across the launch boundary or too few envs earned a reward), s8_L4_rdist (29: a sequence of 4 states is so rarely paid from
all-zero tables that under seeds 0 ... 28 the tables of at most half the envs moved, or no greedy choice was ever strict) and
delay33 (3: under seeds 0 ... 2 no reward left the delay line, so no greedy choice was strict).  The custom matrices come from a
fixed numpy seed each."""
import numpy as np

import learner_sweep_cases as sweep
import eval_summary_cases as evalc

K, LAUNCHES, SEED = sweep.K, sweep.LAUNCHES, sweep.SEED
ALPHA, GAMMA, EPS = sweep.ALPHA, sweep.GAMMA, sweep.EPS
random_q, pe_arrays, tie_q = sweep.random_q, sweep.pe_arrays, evalc.tie_q
double_honest, pe_honest, Q_SEED = sweep.double_honest, sweep.pe_honest, evalc.Q_SEED
ALGOS = ("q_learning", "sarsa", "double_q")
EVAL_ALGOS = evalc.EVAL_ALGOS

_D = dict(state_space_type="discrete", action_space_type="discrete")


def _gen(S, A, L=1, delay=0, seed=0, **kw):
    return dict(_D, state_space_size=S, action_space_size=A, sequence_length=L, delay=delay, seed=seed, **kw)


def _custom(S, A, terminal, mseed, **kw):
    """use_custom_mdp with matrices: integer P [S, A], float64 R [S, A] ~ N(0, 1), no start in a terminal state"""
    r = np.random.default_rng(mseed)
    P = r.integers(0, S, (S, A))
    R = r.normal(size=(S, A))
    init = np.ones(S)
    init[list(terminal)] = 0.0
    return dict(_D, use_custom_mdp=True, state_space_size=S, action_space_size=A, transition_function=P, reward_function=R,
                terminal_states=list(terminal), init_state_dist=init / init.sum(), sequence_length=1, seed=0, **kw)


CFG2 = sweep.CFG2
_NOISE = dict(transition_noise=0.1, reward_noise=0.5)
CASES = {
    "d2_s12_a6": (_gen(12, 6, L=2, delay=1, diameter=2, seed=0), {}),            # S = 2 A; A < 8: padded policy rows
    "d4_s24_a6": (_gen(24, 6, diameter=4, seed=0), {}),                           # S = 4 A; 144 KiB of Q per workgroup
    "custom_13x12": (_custom(13, 12, (3, 7), 131, delay=2), {}),                  # rew_sa keys through the key ring; S, A coprime
    "custom_79x2_noise": (_custom(79, 2, (3, 7), 792, **_NOISE), {}),             # S >> A; noise on a rew_sa handle; 158 KiB of Q
    "s4_L7": (_gen(4, 4, L=7, delay=2, repeats_in_sequences=True, seed=4), {}),   # history bytes 4-7; the gate at byte 7
    "s6_L7": (_gen(6, 6, L=7, delay=0, repeats_in_sequences=True, seed=0), {}),   # 279 936 keys: a 35 KiB bit table in LDS
    "s8_L4_rdist": (_gen(8, 8, L=4, delay=3, reward_dist=[0.5, 1.0], seed=29), {}),   # a non-unit table of 32 KiB; key ring with L > 3
    "s255_a85": (_gen(255, 85, diameter=3, seed=0), {}),                          # state byte 0xFE; global-form Q; policy rows of 85
    "a9": (_gen(9, 9, seed=0), {}),                                               # the first searched policy row; odd A
    "a1_s3": (_gen(3, 1, diameter=3, seed=0), {}),                                # A = 1: empty scan loops, (w 1) >> 32
    "delay32_affine": (_gen(8, 8, delay=32, reward_scale=2.5, reward_shift=-0.5, term_state_reward=3.0, reward_every_n_steps=2, seed=0), {}),
    "delay33": (_gen(8, 8, delay=33, seed=3), {}),                                # unit values through the key ring
    "cfg2_max5_same": (CFG2, dict(max_episode_steps=5)),                          # truncated_with_reset
    "cfg2_max5_next": (CFG2, dict(max_episode_steps=5, autoreset="next_step")),   # truncation, then a reset call
    "s8_noise_max5_next": (_gen(8, 8, seed=0, **_NOISE), dict(max_episode_steps=5, autoreset="next_step")),
}
# truncation, noise and same-step autoreset together: learn() sees a next state that no output shows, so the whole launch is
# predicted on the CPU (closed_loop_cpu.closed_loop on the oracle env's Philox streams): N = 64, Philox streams only
PREDICTED_CASE = ("s8_noise_max5_same", _gen(8, 8, seed=0, **_NOISE), dict(max_episode_steps=5))
PREDICTED_N = 64

NOISE = ("custom_79x2_noise", "s8_noise_max5_next")
RECT = ("d2_s12_a6", "d4_s24_a6", "custom_13x12", "custom_79x2_noise", "s255_a85", "a1_s3")
LONG_L = ("s4_L7", "s6_L7", "s8_L4_rdist")
DELAY_LINE = ("delay32_affine", "delay33")
TRUNC = ("cfg2_max5_same", "cfg2_max5_next", "s8_noise_max5_next")
NON_UNIT = ("custom_13x12", "custom_79x2_noise", "s8_L4_rdist", "delay33")       # UNIT=0 in the kernel's name
SUMMARY_CASES = ("d2_s12_a6", "custom_13x12", "s4_L7", "cfg2_max5_same", "cfg2_max5_next", "s8_noise_max5_next")
HANDOVER_CASES = ("s4_L7", "custom_13x12")
# cfg2's reward needs a sequence of 3 states and arrives 4 steps later: the seventh step of an episode at the earliest.  With
# max_episode_steps = 5 and a reset at every truncation no episode gets there -- every reward is 0 whatever the seed, and from
# all-zero tables nothing would ever be learnt.  These two handles start from random tables instead (tie_q(random_q), as
# "cfg2_random_q" of learner_sweep_cases does): the true next state then shows in every update.
RANDOM_START = ("cfg2_max5_same", "cfg2_max5_next")
NO_REWARD = RANDOM_START

# which streams each learner runs on: the noise cases and s255_a85 (the slowest restatements) run both streams for
# q_learning and one each for the other two
_SHORT = {"q_learning": ("numpy", "philox"), "sarsa": ("numpy",), "double_q": ("philox",)}
STREAMS = {c: (_SHORT if c in NOISE or c == "s255_a85" else {a: ("numpy", "philox") for a in ALGOS}) for c in CASES}
LEARN_RUNS = [(c, a, r) for c in CASES for a in ALGOS for r in STREAMS[c][a]]


# ---- the LDS carve of a shared-table discrete handle (mdpp_create) and what follows from it
def _align16(x):
    return (x + 15) // 16 * 16


def shape_of(cfg):
    """(S, A, L, keys, unit, noise) as the library sees the config (keys: S A for a reward matrix, else S^L)"""
    A = cfg["action_space_size"]
    custom = cfg.get("use_custom_mdp", False)
    S = cfg["state_space_size"] if custom else A * cfg.get("diameter", 1)
    L = cfg["sequence_length"]
    unit = not custom and "reward_dist" not in cfg and cfg["delay"] <= 32
    return S, A, L, (S * A if custom else S ** L), unit, "transition_noise" in cfg


def lds_bytes(cfg):
    """the MDP's own dynamic LDS: P, the terminal flags, the start cdf, the rewards (when within 48 KiB), the noise cdfs
    (when within 32 KiB), each rounded up to 16 bytes"""
    S, A, L, keys, unit, noise = shape_of(cfg)
    off = _align16(S * A)
    off = _align16(off + S)
    off = _align16(off + S * 8)
    rew = (keys + 7) // 8 if unit else keys * 8
    assert rew <= 48 * 1024
    off = _align16(off + rew)
    if noise and S * S * 8 <= 32 * 1024:
        off = _align16(off + S * S * 8)
    return off


def static_lds(cfg):
    """a closed-loop kernel's static LDS: numpy's ziggurat tables, 3 x 256 x 8 bytes, in a NOISE kernel (one entry each otherwise)"""
    return 3 * 8 * (256 if shape_of(cfg)[5] else 1)


def q_lds(cfg, double):
    S, A = shape_of(cfg)[:2]
    return 256 * S * A * 4 * (2 if double else 1)


def qlds_expected(cfg, double, limit):
    """QLDS= of the learner's and the evaluation's kernel name: the workgroup's 256 tables fit beside everything else"""
    return static_lds(cfg) + lds_bytes(cfg) + q_lds(cfg, double) <= limit


def policy_refused(cfg):
    """rollout_policy's refusal, or None: noise is not served, and the thresholds ([S][max(A, 8)] words) join the MDP's tables
    within 64 KiB"""
    S, A = shape_of(cfg)[:2]
    if "transition_noise" in cfg:
        return "transition_noise"
    if lds_bytes(cfg) + 4 * S * max(A, 8) > 64 * 1024:
        return "64 KiB"
    return None


def learner_refused(cfg):
    """the learner's (and the evaluation's) refusal, or None: the MDP's tables, with a NOISE kernel's static LDS, within 64 KiB"""
    noise = "transition_noise" in cfg or "reward_noise" in cfg
    return "64 KiB" if lds_bytes(cfg) + (3 * 256 * 8 if noise else 0) > 64 * 1024 else None


def start_tables(case, n, double):
    S, A = shape_of(CASES[case][0])[:2]
    return tie_q(random_q(Q_SEED, n, S, A, double)) if case in RANDOM_START else None


def eval_tables(cfg, n, double):
    S, A = shape_of(cfg)[:2]
    return tie_q(random_q(Q_SEED, n, S, A, double))


# ---- honesty conditions
def learner_honest(case, algo, info, Q, Q0=None):
    """what a learner's pass must have exercised (info summed over the launches; Q the tables at the end, Q0 at the start)"""
    cfg = CASES[case][0]
    S, A = shape_of(cfg)[:2]
    assert info["explored"] > 0, info
    if A > 1:
        assert info["greedy_strict"] > 0 and info["greedy_ties"] > 0, info
    else:
        # a1_s3: a row of one entry has no tie to resolve and nothing to compare; the scan loops are empty
        assert info["greedy_ties"] == 0 and info["greedy_strict"] > 0, info
    n = Q.shape[0]
    changed = (Q != (0 if Q0 is None else Q0)).reshape(n, -1).any(axis=1)
    if case != "a1_s3" and case not in DELAY_LINE:       # (74 steps pay little behind a delay of 32: see flow_honest)
        assert changed.sum() > n // 2, int(changed.sum())
    if case in TRUNC:
        assert info["trunc_resets"] > 0, info
        if algo == "sarsa" and case in SARSA_DROP_SHOWS:
            assert info["trunc_carry_differs"] > 0, info
    if algo == "double_q":
        double_honest(info, Q, case in RANDOM_START)


# SARSA's carry dropped at a truncation differs from what the next step selects afresh.  Same-step autoreset: the next step
# starts from another episode's first state, so it mostly does.  Next-step autoreset: the next call is the env's reset call,
# which selects from the SAME state with the SAME words -- on the tables after the update instead of before it; the two differ
# only where that one update changed the greedy choice of the row of s', that is where s' == s and no exploration.
SARSA_DROP_SHOWS = ("cfg2_max5_same", "cfg2_max5_next", "s8_noise_max5_next")


# A reward leaves a delay line of 32 only in an episode of 33 steps or more (a reset empties the line).  In these generated
# MDPs every state has an action into each of the 2 terminal states of 8, and delay32_affine pays 3.0 x 2.5 for terminating
# while every other step costs 0.5: a learner that explores a quarter of the time ends its episodes within a few steps and
# soon seeks the end (no seed of 0 ... 40 showed one paid reward in 32 envs x 74 steps).  Greedy evaluation of random tables
# does walk cycles that miss the terminal states: there the condition is asserted for both delay cases.
DELAY_LINE_UNDER_EVALUATION_ONLY = ("delay32_affine",)


def delay_line_honest(cfg, reward, reset_call):
    """at least one reward that came out of the delay line: not the value an unpaid step has, at a terminal state or not"""
    shift = np.float32(cfg.get("reward_shift", 0.0))
    at_term = np.float32(cfg.get("reward_shift", 0.0) + cfg.get("term_state_reward", 0.0) * cfg.get("reward_scale", 1.0))
    assert (~reset_call & (reward != shift) & (reward != at_term)).any()


def flow_honest(case, cfg, state, actions, reward, term, trunc, reset_call):
    """what the steps of a learner's pass must have shown ([T, n] arrays over both launches; state: the state acted from)"""
    S, A = shape_of(cfg)[:2]
    live = ~reset_call
    if case == "a1_s3":
        assert not term.any()                            # (terminal_state_density 0.25 of one action: no terminal state)
    else:
        assert (term & live).any()
    if case in RECT:
        assert S > A                                     # (every rectangular case here; A > S would ask for an action >= S)
        assert (state[live] >= A).any()
        assert (state[live] * A + actions[live] != state[live] * S + actions[live]).any()
    if case in DELAY_LINE and case not in DELAY_LINE_UNDER_EVALUATION_ONLY:
        delay_line_honest(cfg, reward, reset_call)
    if case in LONG_L:
        assert (reward[live] != 0).any()                 # (no shift, no noise: the gate has opened and a key has hit)
    if case in TRUNC:
        cut = live & trunc & ~term
        assert cut.any()
        if case == "cfg2_max5_next":
            assert (reset_call[1:] & cut[:-1]).any()     # a reset call right after a truncation
    if case in NO_REWARD:
        assert not reward.any()


def eval_honest(case, info, double):
    if case == "a1_s3":                                  # (one action: no tie, no terminal state, nothing for the sum to change)
        assert info["greedy_strict"] > 0 and info["greedy_ties"] == 0 and info["terminations"] == 0, info
        return
    evalc.eval_honest(info, double and shape_of(CASES[case][0])[1] > 1)


def summary_honest(counters, return_sum, case, algo):
    """eval_summary_cases.summary_honest, whose exemptions go by its own cases' names: a non-zero return_sum is not asked where
    no reward can be earned (NO_REWARD) nor of greedy evaluation on noise-free handles (the reason given there: a deterministic
    walk that ends has passed through distinct states only)."""
    quiet = case in NO_REWARD or (algo == "eval" and case not in NOISE)
    evalc.summary_honest(counters, return_sum if not quiet else np.ones(1), "shape:" + case, algo)
    if case in TRUNC:
        assert counters["ended_truncated"] > 0, counters
    if case in ("cfg2_max5_next", "s8_noise_max5_next"):
        assert counters["reset_calls"] > 0, counters


# ---- further tests of the GPU file
# the QLDS decision near the device's limit: 256 tables of these shapes are 144, 288, 158, 159, 150 and 156 KiB.  At a limit of
# 160 KiB the MDP's own carve tips 53 x 3 over, 75 x 2 fits with a NOISE kernel's 6 KiB of static LDS, and 78 x 2 fits without
# them only: there the static LDS decides (tests/test_closed_loop_shapes_host.py works the three out by hand)
QLDS_EDGE = {
    "d4_s24_a6": (CASES["d4_s24_a6"][0], False),
    "d4_s24_a6_double": (CASES["d4_s24_a6"][0], True),
    "custom_79x2_noise": (CASES["custom_79x2_noise"][0], False),
    "custom_53x3": (_custom(53, 3, (3, 7), 533, delay=0), False),
    "custom_75x2_noise": (_custom(75, 2, (3, 7), 752, **_NOISE), False),
    "custom_78x2_noise": (_custom(78, 2, (3, 7), 782, **_NOISE), False),
}

# float edges of the tables: every entry is drawn from this pool
FLOAT_EDGE_CASES = {"cfg2": (CFG2, {}), "d2_s12_a6": CASES["d2_s12_a6"]}
_FMAX, _FMIN = np.finfo(np.float32).max, np.finfo(np.float32).tiny
FLOAT_POOL = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, _FMIN, -_FMIN, 1.0, -1.0, _FMAX, -_FMAX, np.inf, -np.inf], np.float32)


def float_edge_tables(seed, n, S, A, double):
    shape = (n, 2, S, A) if double else (n, S, A)
    q = FLOAT_POOL[np.random.default_rng(seed).integers(0, len(FLOAT_POOL), shape)]
    # every fourth env: zeros of either sign only (the strict > scan between -0.0 and +0.0) with a few denormals
    z = np.random.default_rng(seed + 1).integers(0, 4, shape)
    q[::4] = FLOAT_POOL[z][::4]
    assert q.dtype == np.float32 and np.signbit(q[q == 0]).any() and not np.isnan(q).any()
    return q


def float_edge_honest(info):
    """a selection decided between -0.0 and +0.0, an update whose result is denormal, a NaN produced (inf - inf)"""
    assert info["zero_sign_ties"] > 0 and info["denormal_results"] > 0 and info["nans_made"] > 0, info
    assert info["explored"] > 0 and info["greedy_strict"] > 0, info


N_EDGES = (1, 63, 257)
