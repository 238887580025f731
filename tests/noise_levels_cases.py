"""What tests/test_gpu_noise_levels.py runs and what it asserts about its own coverage (per-env noise levels:
RLToyVectorEnv.set_noise_levels), shared with tests/test_noise_levels_host.py, which shows on the CPU -- the oracle env per
level in a closed loop with the learner's restatement -- that those conditions can be met before any GPU run.

The levels are the values of the reference's six noise sweeps (experiments/*_tabular_p_noise.py, *_r_noise.py) and cycle by
env index: the transition level is i % 5, the reward level (i // 5) % 5, so any 25 consecutive envs -- and every wave of 64 --
hold all 25 pairs, and lanes that skip the space-stream draw (level 0) sit beside lanes that make it."""
import numpy as np

import learner_sweep_cases as sweep

K, LAUNCHES, SEED = sweep.K, sweep.LAUNCHES, sweep.SEED
ALPHA, GAMMA, EPS = sweep.ALPHA, sweep.GAMMA, sweep.EPS
TN = (0.0, 0.01, 0.02, 0.10, 0.25)
RN = (0.0, 1.0, 5.0, 10.0, 25.0)
# what a handle that is given levels is created with: both keys present, transition_noise > 0 (any values: the levels replace them)
CREATED = dict(transition_noise=0.5, reward_noise=3.0)

_D = dict(state_space_type="discrete", action_space_type="discrete")
TABULAR = dict(_D, state_space_size=8, action_space_size=8, delay=0, sequence_length=1, seed=0)
RDIST = dict(_D, state_space_size=8, action_space_size=8, delay=3, sequence_length=2, reward_dist=[0.5, 1.0], seed=40)
# five levels of [29][29] float64 cdfs are 33 640 B: beyond the 32 KiB the cdfs may take in LDS, they stay in global memory
S29 = dict(_D, state_space_size=29, action_space_size=29, delay=0, sequence_length=1, seed=0)
assert 5 * 29 * 29 * 8 == 33640 > 32 * 1024 >= 5 * 20 * 20 * 8

# case -> (config without noise keys, handle keywords, the (algo, rng) pairs the twin rule runs over)
_ALL = tuple((a, r) for a in ("q_learning", "sarsa", "double_q") for r in ("numpy", "philox"))
CASES = {
    "tabular": (TABULAR, {}, _ALL),
    "cfg2": (sweep.CFG2, {}, _ALL),
    "rdist_delay3": (RDIST, {}, (("double_q", "numpy"), ("sarsa", "philox"))),                 # non-unit rewards behind a delay: the key ring
    "s20": (sweep.S20, {}, (("q_learning", "numpy"), ("double_q", "philox"))),                  # QLDS=0
    "s29": (S29, {}, (("sarsa", "numpy"), ("q_learning", "philox"))),                           # ... and the cdfs in global memory
    "cfg2_next_step": (sweep.CFG2, dict(autoreset="next_step"), (("sarsa", "numpy"), ("double_q", "philox"))),
    "cfg2_disabled_max5": (sweep.CFG2, dict(autoreset="disabled", max_episode_steps=5), (("double_q", "numpy"), ("q_learning", "philox"))),
}
GLOBAL_Q = ("s20", "s29")            # a workgroup's 256 Q-tables do not fit in LDS
TWIN_PARAMS = [(c, a, r) for c, (_, _, pairs) in CASES.items() for a, r in pairs]


def level_arrays(n, lo=0):
    """(transition_noise, reward_noise) float64 [n] of envs lo ... lo + n - 1"""
    i = np.arange(lo, lo + n)
    return np.asarray(TN)[i % 5], np.asarray(RN)[(i // 5) % 5]


def mixed_cfg(cfg):
    return dict(cfg, **CREATED)


def twin_cfg(cfg, p, sigma):
    """the config of the uniform handle env i of a mixed handle must equal: created at (p, sigma), everything else equal
    (p == 0: the library sees no transition_noise key)"""
    return dict(cfg, transition_noise=float(p), reward_noise=float(sigma))


def pairs_present(tn, rn):
    return sorted(set(zip(tn.tolist(), rn.tolist())))


def honest(tn, rn, state, action, next_state, reward, terminated, explored_env, P, live):
    """What a pass over mixed levels must have exercised.  tn, rn [n]: the envs' levels; state, action, next_state, reward,
    terminated [T, n]: every step's state acted from, action, TRUE next state, float32 reward and flag; live [T, n]: the step is
    a step of the env (not a reset call); explored_env [n]: exploring selections per env; P [S, A]."""
    noisy = live & (next_state != P[state, action])
    for p in TN:
        at = tn == p
        assert at.any()
        if p == 0.0:
            assert not noisy[:, at].any(), "level 0 made a noisy transition"
        else:
            assert noisy[:, at].any(), ("no noisy transition at level", p)
        assert terminated[:, at].any(), ("no termination at level", p)
        assert (explored_env[at] > 0).any(), ("no explored step at level", p)
    # rewards of different sigma differ: sigma = 0 pays the MDP's few noise-free values, the mean |reward| grows with sigma
    spread = []
    for s in RN:
        at = rn == s
        assert at.any()
        r = reward[:, at][live[:, at]]
        if s == 0.0:
            assert len(np.unique(r)) <= 8, np.unique(r)
        else:
            assert len(np.unique(r)) > 100
        spread.append(np.abs(r.astype(np.float64)).mean())
    assert all(a < b for a, b in zip(spread, spread[1:])), spread
