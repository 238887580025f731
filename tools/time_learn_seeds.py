"""A seed sweep of the in-kernel learners in ONE launch -- RLToyVectorEnv(seeds=[...]).set_learner(..., per_env_mdp=True), every
agent on its own env's MDP -- against what it replaces: ten shared-MDP handles of a tenth of the envs each, ten launches.

    python tools/time_learn_seeds.py [--envs 65536] [--steps 512] [--repeats 5] [--out profiles/learn_per_env_mdp.json]

Shapes: the reference's tabular-agent shape (S = A = 8, sequence_length 1, delay 0, transition_noise and reward_noise named at
0) and BASELINE cfg2 (S = A = 8, delay 4, sequence_length 3), numpy streams, Q-learning.  Each figure is the median of
--repeats timings after a warm-up of every timed form, taken with the library's HIP events on the caller's stream:
  per_env_us            (a) one rollout_learn(K) launch of --envs envs, one MDP per env (seeds 0 ... envs - 1), default placement
  per_env_<options>_us  ... in each placement the kernel options reach: NO_PM_LDS (the MDPs in global memory), NO_LEARN_LDS
                        (the Q-tables in global memory), both
  ten_handles_us        (b) ten shared-MDP handles of ceil(envs / 10) envs (seeds 0 ... 9), ten rollout_learn(K) launches in a row
  shared_us             (c) one rollout_learn(K) launch of --envs envs on one shared MDP: what per-lane tables cost (no bar)
The bar is (a) in its default placement faster than (b); the tool exits with status 1 otherwise.  Nothing else is gated.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mdp_playground_amd import RLToyVectorEnv  # noqa: E402

BASE = dict(state_space_type="discrete", action_space_type="discrete")
CONFIGS = {
    "tabular_s8_noise_keys_at_0": dict(BASE, state_space_size=8, action_space_size=8, delay=0, sequence_length=1,
                                       transition_noise=0.0, reward_noise=0.0),
    "cfg2": dict(BASE, state_space_size=8, action_space_size=8, delay=4, sequence_length=3),
}
ALPHA, GAMMA, EPS = 0.3, 0.9, 0.1
HANDLES = 10
PLACEMENTS = [(), ("NO_PM_LDS",), ("NO_LEARN_LDS",), ("NO_PM_LDS", "NO_LEARN_LDS")]


def timed_us(env, fn, repeats):
    """median and all timings of fn(), by env's HIP events on the current stream"""
    fn()                                    # warm-up: code objects, allocator, the kernel's LDS attribute
    torch.cuda.synchronize(env.device)
    out = []
    for _ in range(repeats):
        env.timer_begin()
        fn()
        out.append(env.timer_end() * 1e3)
    return statistics.median(out), [round(x, 1) for x in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    N, K = args.envs, args.steps
    n_small = -(-N // HANDLES)
    learner = dict(alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=1)
    rows, ok = [], True
    for name, cfg in CONFIGS.items():
        row = dict(config=name, num_envs=N, steps=K, handles=HANDLES, envs_per_handle=n_small)
        # (a) one MDP per env, one launch
        env = RLToyVectorEnv(seeds=list(range(N)), device=dev, **cfg)
        row["tables_built_on"] = env.tables_built_on
        out = env.alloc_rollout_learn(K)
        env.set_learner("q_learning", per_env_mdp=True, **learner)
        for options in PLACEMENTS:
            env.set_kernel_options(*options)
            key = "per_env" + "".join("_" + o.lower() for o in options)
            t, t_all = timed_us(env, lambda: env.rollout_learn(K, out=out), args.repeats)
            row[key + "_us"], row[key + "_all_us"], row[key + "_kernel"] = round(t, 1), t_all, env.learn_kernel_name(K)
        env.set_kernel_options()
        assert not env.status().any()
        env.close()
        del out
        # (b) ten shared-MDP handles, ten launches
        small = [RLToyVectorEnv(num_envs=n_small, device=dev, seed=s, **cfg) for s in range(HANDLES)]
        outs = [e.alloc_rollout_learn(K) for e in small]
        for e in small:
            e.set_learner("q_learning", **learner)

        def ten():
            for e, o in zip(small, outs):
                e.rollout_learn(K, out=o)
        t, t_all = timed_us(small[0], ten, args.repeats)
        row["ten_handles_us"], row["ten_handles_all_us"], row["ten_handles_kernel"] = round(t, 1), t_all, small[0].learn_kernel_name(K)
        for e in small:
            assert not e.status().any()
            e.close()
        del outs
        # (c) one shared MDP, one launch of the same size
        env = RLToyVectorEnv(num_envs=N, device=dev, seed=0, **cfg)
        out = env.alloc_rollout_learn(K)
        env.set_learner("q_learning", **learner)
        t, t_all = timed_us(env, lambda: env.rollout_learn(K, out=out), args.repeats)
        row["shared_us"], row["shared_all_us"], row["shared_kernel"] = round(t, 1), t_all, env.learn_kernel_name(K)
        env.close()
        del out
        row["ten_handles_over_per_env"] = round(row["ten_handles_us"] / row["per_env_us"], 2)
        row["per_env_over_shared"] = round(row["per_env_us"] / row["shared_us"], 2)
        row["env_steps_per_s"] = round(N * K / (row["per_env_us"] * 1e-6), 0)
        ok = ok and row["per_env_us"] < row["ten_handles_us"]
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(dev), alpha=ALPHA, gamma=GAMMA, epsilon=EPS, algo="q_learning",
                           bar="per_env_us < ten_handles_us", accepted=ok, rows=rows), f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
