"""What tests/test_gpu_learn_sweep.py runs and what it asserts about its own coverage, shared with
tests/test_learner_sweep_host.py, which checks on the CPU (32 envs, the oracle env in a closed loop with the restatement)
that those counts can be met before any GPU run."""
import numpy as np

K = 37
LAUNCHES = 2
SEED = (7 << 32) + 4321           # the learner's seed, beyond 32 bits
ALPHA, GAMMA, EPS = 0.3, 0.9, 0.25

_D = dict(state_space_type="discrete", action_space_type="discrete")
# (MDP seed 40 for the delayed-reward shapes: see tests/test_gpu_learn_rollout.py)
CFG2 = dict(_D, state_space_size=8, action_space_size=8, delay=4, sequence_length=3, seed=40)
_S8 = dict(_D, state_space_size=8, action_space_size=8, delay=0, sequence_length=1, seed=0)
S20 = dict(_D, state_space_size=20, action_space_size=20, delay=0, sequence_length=1, seed=0)
# double Q-learning: the handles of the one-table learners' test; "cfg2_random_q" starts from random tables (q=)
DOUBLE_CASES = {
    "cfg2": (CFG2, {}),
    "rdist_delay3": (dict(_D, state_space_size=8, action_space_size=8, delay=3, sequence_length=2, reward_dist=[0.5, 1.0], seed=40), {}),
    "cfg2_next_step": (CFG2, dict(autoreset="next_step")),
    "cfg2_disabled_max5": (CFG2, dict(autoreset="disabled", max_episode_steps=5)),
    "s8_noise_keys_at_0": (dict(_S8, transition_noise=0.0, reward_noise=0.0), {}),
    "s8_noise": (dict(_S8, transition_noise=0.1, reward_noise=0.5), {}),
    "s20": (S20, {}),
    "cfg2_random_q": (CFG2, {}),
}
GLOBAL_FORM = ("s20",)
PE_CASES = {"cfg2": (CFG2, {}), "s20": (S20, {})}

# per-env parameters: cycles by env index -- alpha by i % 4, epsilon by (i // 4) % 4, gamma by (i // 16) % 3 -- so any 48
# consecutive envs, and so every wave of 64, hold all 48 combinations
PE_ALPHA, PE_EPS, PE_GAMMA = (0.1, 0.3, 0.5, 1.0), (0.0, 0.01, 0.25, 1.0), (0.0, 0.9, 1.0)


def pe_arrays(n, lo=0):
    """(alpha, gamma, epsilon) float32 [n] of envs lo ... lo + n - 1"""
    i = np.arange(lo, lo + n)
    return (np.asarray(PE_ALPHA, np.float32)[i % 4], np.asarray(PE_GAMMA, np.float32)[(i // 16) % 3], np.asarray(PE_EPS, np.float32)[(i // 4) % 4])


def random_q(seed, n, S, A, double):
    shape = (n, 2, S, A) if double else (n, S, A)
    return np.random.default_rng(seed).normal(size=shape).astype(np.float32)


def double_honest(info, Q, random_tables):
    """what a double-Q pass must have exercised (info summed over the launches; Q [n, 2, S, A] at the end)"""
    assert info["updates_a"] > 0 and info["updates_b"] > 0, info
    assert info["explored"] > 0 and info["greedy_strict"] > 0, info
    assert (Q[:, 0] != Q[:, 1]).any()
    assert (Q[:, 0] != 0).any() and (Q[:, 1] != 0).any()
    if random_tables:
        assert info["cross_differs"] > 0 and info["sum_differs"] > 0, info


def pe_honest(info, eps):
    """per-env parameters: epsilon = 0 never explores, epsilon = 1 always does on selecting steps; both kinds select"""
    e0, e1 = eps == 0.0, eps == 1.0
    assert e0.any() and e1.any()
    assert (info["selections_env"][e0] > 0).all() and (info["selections_env"][e1] > 0).all()
    assert (info["explored_env"][e0] == 0).all()
    assert (info["explored_env"][e1] == info["selections_env"][e1]).all()
    mid = ~e0 & ~e1
    assert 0 < info["explored_env"][mid].sum() < info["selections_env"][mid].sum()
    assert info["greedy_strict"] > 0 and info["updates"] > 0, info
