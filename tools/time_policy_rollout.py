"""Closed-loop rollouts under a tabular policy: the fused launch (rollout_policy) against the open-loop launch of the same
handle and against the closed loop a user had before it -- one step() per step plus torch sampling from the same table.

    python tools/time_policy_rollout.py [--envs 65536] [--steps 512] [--repeats 5] [--out profiles/policy_rollout.json]

Shapes: BASELINE cfg2 (S = A = 8, delay 4, sequence_length 3) and S = A = 50, sequence_length 1, numpy streams, default
dispatch.  Each figure is the median of --repeats timings after a warm-up of every timed form, taken with the library's
HIP events on the caller's stream (mdpp_timer_begin / mdpp_timer_end):
  closed_loop_us   one rollout_policy(K) launch
  open_loop_us     one rollout(actions) launch fed with the actions of a closed-loop launch
  step_loop_us     K x { a = searchsorted(cdf[obs], u, right=True) in torch;  obs = step(a) }
The tool exits with status 1 unless the fused launch is at least --min-speedup (2) times faster than the step() loop
on every shape; the ratio to the open-loop launch is recorded, not gated.
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

BASE = dict(state_space_type="discrete", action_space_type="discrete", seed=0)
CONFIGS = {
    "cfg2": dict(BASE, state_space_size=8, action_space_size=8, delay=4, sequence_length=3),
    "s50_l1": dict(BASE, state_space_size=50, action_space_size=50, sequence_length=1),
}


def random_policy(S, A, seed=0):
    r = np.random.default_rng(seed)
    p = r.random((S, A))
    return p / p.sum(axis=1, keepdims=True)


def timed_us(env, fn, repeats):
    fn()                                    # warm-up: code objects, allocator
    torch.cuda.synchronize(env.device)
    out = []
    for _ in range(repeats):
        env.timer_begin()
        fn()
        out.append(env.timer_end() * 1e3)
    return statistics.median(out), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-speedup", type=float, default=2.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    N, K = args.envs, args.steps
    rows, ok = [], True
    for name, cfg in CONFIGS.items():
        env = RLToyVectorEnv(num_envs=N, device=dev, **cfg)
        S, A = env.mdps[0].S, env.mdps[0].A
        p = random_policy(S, A)
        env.set_policy(p, seed=1)
        out = env.alloc_rollout_policy(K)
        closed, closed_all = timed_us(env, lambda: env.rollout_policy(K, out=out), args.repeats)
        actions = out[4].clone()
        open_, open_all = timed_us(env, lambda: env.rollout(actions, out=out[:4]), args.repeats)
        cdf = torch.as_tensor(p.cumsum(axis=1) / p.sum(axis=1, keepdims=True), device=dev)
        cdf[:, -1] = 2.0                    # (a uniform below 1 never passes the last entry)

        def step_loop():
            obs = env._obs
            for _ in range(K):
                u = torch.rand((N, 1), dtype=torch.float64, device=dev)
                a = torch.searchsorted(cdf[obs], u, right=True).squeeze(1).to(torch.int32)
                obs = env.step(a)[0]
        loop, loop_all = timed_us(env, step_loop, args.repeats)
        row = dict(config=name, num_envs=N, steps=K, closed_loop_us=round(closed, 1), open_loop_us=round(open_, 1),
                   step_loop_us=round(loop, 1), speedup_vs_step_loop=round(loop / closed, 2),
                   closed_over_open=round(closed / open_, 2), env_steps_per_s=round(N * K / (closed * 1e-6), 0),
                   closed_loop_kernel=env.policy_kernel_name(K), open_loop_kernel=env.rollout_kernel_name(K),
                   closed_loop_all_us=[round(x, 1) for x in closed_all], open_loop_all_us=[round(x, 1) for x in open_all],
                   step_loop_all_us=[round(x, 1) for x in loop_all])
        assert not env.status().any()
        ok = ok and loop / closed >= args.min_speedup
        print(json.dumps(row), flush=True)
        rows.append(row)
        env.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(dev), min_speedup=args.min_speedup, accepted=ok, rows=rows), f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
