"""The cases of the grid handles' per-env noise levels (RLToyVectorEnv.set_grid_noise_levels; include/mdpp.h "Grid noise levels";
tests/test_grid_noise_levels_host.py runs each on the CPU and asserts the conditions that keep a GPU pass honest;
tests/test_gpu_grid_noise_levels.py runs each on the GPU against uniform twins and tests/grid_noise_levels_ref.py).

N = 320, K = 37 and two launches, with the Philox seed, env-id offset and learner seed of tests/grid_learner_cases.py.  A case
is a creation config plus a short list of (p, sigma) PAIRS -- None where the handle has no such key.  The pair of env i is
i % len(pairs), so every wave mixes levels -- except envs 64 ... 127, one whole wave at the first pair, and envs 128 ... 191,
one at the last.

  g34_both              (3, 4) dense, created with p = 0.2, sigma = 0.25; same-step, limit 9; A = 4 (QLDS=1)
  g55_noop_next_ponly   (5, 5) sparse, created with p = 0.25, no reward key; next-step, limit 7; A = 5 (QLDS=0)
  g88_disabled_ronly    (8, 8) dense, reward_noise = 0.0 named, terminal reward -0.5, no transition key; disabled, limit 29 (QLDS=0)
  g17_both_i32          (1, 7) dense, created with p = 0.3, sigma = 0.5, int32 observations; same-step, limit 11 (QLDS=1)

Every case starts from zero tables."""
import numpy as np

import grid_learner_cases as gc

N, K, LAUNCHES = gc.N, gc.K, gc.LAUNCHES
PHILOX_SEED, ENV_ID_OFFSET, LEARNER_SEED = gc.PHILOX_SEED, gc.ENV_ID_OFFSET, gc.LEARNER_SEED

_BASE = dict(state_space_type="grid", reward_function="move_to_a_point", seed=5)

CASES = {
    # name: creation config, handle kwargs, noop, the table placement the launch must report, (alpha, gamma, epsilon), pairs (p, sigma)
    "g34_both": dict(cfg=dict(_BASE, grid_shape=(3, 4), make_denser=True, target_point=[1, 2], transition_noise=0.2, reward_noise=0.25),
                     kw=dict(autoreset="same_step", max_episode_steps=9), noop=False, qlds=1, rates=(0.5, 0.9, 0.3),
                     pairs=((0.0, 0.0), (0.1, 0.5), (0.5, 0.0), (1.0, 2.0))),
    "g55_noop_next_ponly": dict(cfg=dict(_BASE, grid_shape=(5, 5), make_denser=False, target_point=[2, 2], transition_noise=0.25),
                                kw=dict(autoreset="next_step", max_episode_steps=7), noop=True, qlds=0, rates=(0.5, 0.75, 0.35),
                                pairs=((0.0, None), (0.25, None), (0.6, None))),
    "g88_disabled_ronly": dict(cfg=dict(_BASE, grid_shape=(8, 8), make_denser=True, target_point=[1, 1], reward_noise=0.0,
                                        term_state_reward=-0.5),
                               kw=dict(autoreset="disabled", max_episode_steps=29), noop=False, qlds=0, rates=(0.75, 0.5, 0.5),
                               pairs=((None, 0.0), (None, 1.0), (None, 5.0))),
    "g17_both_i32": dict(cfg=dict(_BASE, grid_shape=(1, 7), make_denser=True, target_point=[0, 4], transition_noise=0.3, reward_noise=0.5,
                                  dtype_s=np.int32),
                         kw=dict(autoreset="same_step", max_episode_steps=11), noop=False, qlds=1, rates=(0.5, 0.9, 0.3),
                         pairs=((0.0, 0.5), (0.3, 0.0), (0.05, 3.0))),
}


def n_actions(case):
    return 5 if CASES[case]["noop"] else 4


def pair_index(case, n=N):
    """int64 [n]: the pair of every env"""
    m = len(CASES[case]["pairs"])
    idx = np.arange(n) % m
    idx[64:128] = 0
    idx[128:192] = m - 1
    return idx


def levels(case, n=N):
    """dict(transition_noise=, reward_noise=): what the case hands set_grid_noise_levels on a handle of n envs (None: a key the
    handle does not have)"""
    idx = pair_index(case, n)
    p, s = zip(*CASES[case]["pairs"])
    return dict(transition_noise=None if p[0] is None else np.asarray(p, np.float64)[idx],
                reward_noise=None if s[0] is None else np.asarray(s, np.float64)[idx])


def uniform_cfg(case, pair):
    """the config of a handle created uniformly at `pair`: transition_noise = 0 is a config without the key (the library sees
    none); reward_noise stays named at any value, 0 included"""
    cfg = dict(CASES[case]["cfg"])
    p, s = pair
    if p is not None:
        if p == 0.0:
            del cfg["transition_noise"]
        else:
            cfg["transition_noise"] = p
    if s is not None:
        cfg["reward_noise"] = s
    return cfg


def expected_name(case, rng, eval=False, summary=False, qlds=None, sched=False):
    c = CASES[case]
    return "k_grid_learn_rollout<PHILOX=%d,NOISE=1,QLDS=%d,EVAL=%d,SUMMARY=%d,NLEV=1%s>" % (
        int(rng == "philox"), c["qlds"] if qlds is None else qlds, int(eval), int(summary), ",SCHED=1" if sched else "")


def uniform_name(case, pair, rng, eval=False, summary=False, qlds=None):
    """the existing kernel of a handle created at `pair`"""
    cfg = uniform_cfg(case, pair)
    noise = int("transition_noise" in cfg or "reward_noise" in cfg)
    return "k_grid_learn_rollout<PHILOX=%d,NOISE=%d,QLDS=%d,EVAL=%d,SUMMARY=%d>" % (
        int(rng == "philox"), noise, CASES[case]["qlds"] if qlds is None else qlds, int(eval), int(summary))


# ---- the scheduled case: g17_both_i32 under an epsilon-and-alpha schedule, R = 2, M = 4, row[i] = i % 2
SCHED_CASE = "g17_both_i32"


def schedule(n=N):
    from mdp_playground_amd import policy
    d = policy.epsilon_decay
    rows = lambda *r: np.array(r, np.float64).astype(np.float32)
    return dict(epsilon=rows(d("linear", 0.9, 4, 0.1), [0.6, 0.4, 0.25, 0.05]), alpha=rows(d("log", 1.0, 4, 0.125), [0.75, 0.5, 0.375, 0.25]),
                row=(np.arange(n) % 2).astype(np.int32))


def ref_schedule(n=N):
    import learner_schedule_ref as sref
    return sref.Schedule(n, **schedule(n))
