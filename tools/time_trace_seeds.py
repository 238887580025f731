"""A lambda x seed sweep of the in-kernel trace learners in ONE launch -- RLToyVectorEnv(seeds=[...]) with
set_learner(..., per_env_mdp=True) and set_learner_traces(..., per_env_mdp=True), every agent on its own env's MDP -- against
what it replaces: ten shared-MDP trace handles of a tenth of the envs each, ten launches.

    python tools/time_trace_seeds.py [--envs 65536] [--steps 512] [--repeats 5] [--out profiles/trace_seeds.json]

Shapes: the reference's delay experiment (S = A = 8, sequence_length 1, delay 4, transition_noise and reward_noise named at 0)
and BASELINE cfg2 (S = A = 8, delay 4, sequence_length 3); numpy streams, Q-learning, replacing traces, lambda 0.8,
epsilon 0.1.  Each figure is the median of --repeats timings after a warm-up of every timed form, taken with the library's
HIP events on the caller's stream; every run is kept:
  per_env_us            (a) one rollout_learn(K) launch of --envs envs on seeds 0 ... 9 repeated over the envs (env i on seed
                        i % 10), default placement
  per_env_<options>_us  (b) ... in each placement the kernel options force: NO_PM_LDS (the MDPs in global memory), NO_LEARN_LDS
                        (Q and Z in global memory), both
  ten_handles_us        (c) ten shared-MDP trace handles of ceil(envs / 10) envs (seeds 0 ... 9), ten rollout_learn(K) launches
                        in a row
  shared_us             (d) one shared-MDP trace launch of --envs envs (seed 0): what per-lane tables cost (no bar)
  traceless_us          (e) the handle of (a) without traces: the traceless per-env-MDP learner (no bar)
  sched_us              (f) (a) with a set_learner_schedule(..., sweep=True) schedule: epsilon and alpha decaying per episode (no bar)
The bar, DESIGN.md 3.17's and 3.25's: the SLOWEST run of (a) is faster than the FASTEST run of (c), on every shape; the tool
exits with status 1 otherwise.  Nothing else is gated.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mdp_playground_amd import RLToyVectorEnv  # noqa: E402

BASE = dict(state_space_type="discrete", action_space_type="discrete")
CONFIGS = {
    "s8_delay4_noise_keys_at_0": dict(BASE, state_space_size=8, action_space_size=8, delay=4, sequence_length=1,
                                      transition_noise=0.0, reward_noise=0.0),
    "cfg2": dict(BASE, state_space_size=8, action_space_size=8, delay=4, sequence_length=3),
}
ALPHA, GAMMA, EPS, LAMBDA = 0.3, 0.9, 0.1, 0.8
HANDLES = 10
FORCED = [("NO_PM_LDS",), ("NO_LEARN_LDS",), ("NO_PM_LDS", "NO_LEARN_LDS")]
SCHED_M = 64


def timed_us(env, fn, repeats):
    """median and all timings of fn(), by env's HIP events on the current stream"""
    fn()                                    # warm-up: code objects, allocator, the kernel's LDS attribute, the parameter arrays' fill
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

        def put(key, env, fn):
            t, t_all = timed_us(env, fn, args.repeats)
            row[key + "_us"], row[key + "_all_us"], row[key + "_kernel"] = round(t, 1), t_all, env.learn_kernel_name(K)

        # (a), (b), (e), (f): one MDP per env, one launch
        env = RLToyVectorEnv(seeds=[i % HANDLES for i in range(N)], device=dev, **cfg)
        row["tables_built_on"] = env.tables_built_on
        out = env.alloc_rollout_learn(K)
        learn = lambda: env.rollout_learn(K, out=out)                       # noqa: E731
        env.set_learner("q_learning", per_env_mdp=True, **learner)
        put("traceless", env, learn)
        env.set_learner_traces(LAMBDA, "replacing", per_env_mdp=True)
        put("per_env", env, learn)
        for options in FORCED:
            env.set_kernel_options(*options)
            put("per_env" + "".join("_" + o.lower() for o in options), env, learn)
        env.set_kernel_options()
        env.set_learner_schedule(epsilon=np.linspace(1.0, 0.05, SCHED_M), alpha=np.linspace(0.5, 0.1, SCHED_M), sweep=True)
        put("sched", env, learn)
        assert not env.status().any()
        env.close()
        del out
        # (c) ten shared-MDP trace handles, ten launches
        small = [RLToyVectorEnv(num_envs=n_small, device=dev, seed=s, **cfg) for s in range(HANDLES)]
        outs = [e.alloc_rollout_learn(K) for e in small]
        for e in small:
            e.set_learner("q_learning", **learner)
            e.set_learner_traces(LAMBDA, "replacing")

        def ten():
            for e, o in zip(small, outs):
                e.rollout_learn(K, out=o)
        put("ten_handles", small[0], ten)
        for e in small:
            assert not e.status().any()
            e.close()
        del outs
        # (d) one shared MDP, one trace launch of the same size
        env = RLToyVectorEnv(num_envs=N, device=dev, seed=0, **cfg)
        out = env.alloc_rollout_learn(K)
        env.set_learner("q_learning", **learner)
        env.set_learner_traces(LAMBDA, "replacing")
        put("shared", env, lambda: env.rollout_learn(K, out=out))
        env.close()
        del out
        row["ten_handles_over_per_env"] = round(row["ten_handles_us"] / row["per_env_us"], 2)
        row["per_env_over_shared"] = round(row["per_env_us"] / row["shared_us"], 3)
        row["per_env_over_traceless"] = round(row["per_env_us"] / row["traceless_us"], 3)
        row["sched_over_per_env"] = round(row["sched_us"] / row["per_env_us"], 3)
        for options in FORCED:
            key = "per_env" + "".join("_" + o.lower() for o in options)
            row[key + "_over_default"] = round(row[key + "_us"] / row["per_env_us"], 3)
        row["env_steps_per_s"] = round(N * K / (row["per_env_us"] * 1e-6), 0)
        row["slowest_per_env_us"], row["fastest_ten_handles_us"] = max(row["per_env_all_us"]), min(row["ten_handles_all_us"])
        row["accepted"] = row["slowest_per_env_us"] < row["fastest_ten_handles_us"]
        ok = ok and row["accepted"]
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(dev), alpha=ALPHA, gamma=GAMMA, epsilon=EPS, lam=LAMBDA, algo="q_learning",
                           kind="replacing", repeats=args.repeats,
                           bar="the slowest run of per_env is faster than the fastest run of ten_handles, on every shape",
                           accepted=ok, rows=rows), f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
