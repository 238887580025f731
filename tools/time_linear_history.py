"""Closed-loop continuous rollouts under a linear policy WITH MEMORY (set_linear_policy(theta, history=2)): the fused launch
against the history = 1 launch of the same handle and against the loop it replaces -- one step() per step, with p, the per-env
episode-boundary test and the W and V products in torch.

    python tools/time_linear_history.py [--envs 65536] [--steps 512] [--repeats 5] [--out profiles/linear_history.json]

Shapes and method: tools/time_linear_rollout.py's (bench.py's c_d2_n0, cfg3 and cfg5, numpy streams; the median of --repeats
timings after a warm-up of the timed form, taken with the library's HIP events on the caller's stream; every run is kept).
Legs per shape:
  history2_us          one rollout_linear(K) launch, one [D, 2 D + 1] parameter set per env (the kernel's name says the placement)
  history2_summary_us  rollout_linear(K, summary=): no [K, N] output
  history1_us          the same handle under the history = 1 policy with the same W and b
  step_loop_us         K x { p = where(first, obs, mem); a = clamp(b + W obs + V p) in torch; mem = obs; obs, .., = step(a);
                             first = terminated | truncated }
The loop timed is step(a) per step with the action formed in torch, as tools/time_linear_rollout.py's step_loop: the only loop
that runs THIS policy without the feature.  A rollout_linear(1, summary=) launch per step forms its action in the kernel from o
alone, so p could enter it only through a new parameter set at every step (set_linear_policy with V p folded into b); that loop
was not built or timed.  For scale: tools/time_linear_es.py measured per-step launches with torch bookkeeping at 175-203 ms per
512 steps on these shapes (profiles/linear_es.json), several times the slowest run here.
Acceptance: on every shape the slowest of the history2 runs is faster than the fastest of the step-loop runs.  The ratio to
history = 1 is recorded, not bounded.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mdp_playground_amd import RLToyVectorEnv  # noqa: E402
from time_linear_rollout import CONFIGS, draw_theta, timed_us  # noqa: E402


def draw_theta2(n, d, seed=0):
    """time_linear_rollout's W and b, and V = 0.5 I plus a small random part: [n, d, 2 d + 1]"""
    wb = draw_theta(n, d, seed)
    v = np.random.default_rng(seed + 1).uniform(-0.2, 0.2, (n, d, d))
    v[:, np.arange(d), np.arange(d)] += 0.5
    return np.ascontiguousarray(np.concatenate([wb[:, :, :d], v.astype(np.float32), wb[:, :, d:]], axis=2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    N, K = args.envs, args.steps
    rows, ok = [], True
    for name in args.configs.split(","):
        env = RLToyVectorEnv(num_envs=N, device=dev, **CONFIGS[name])
        D, amax = env.mdps[0].D, float(env.mdps[0].action_space_max)
        th2 = draw_theta2(N, D)
        theta2 = torch.from_numpy(th2).to(dev)
        theta1 = torch.from_numpy(np.ascontiguousarray(np.concatenate([th2[:, :, :D], th2[:, :, 2 * D:]], axis=2))).to(dev)
        env.reset()
        out = env.alloc_rollout_linear(K)
        row = dict(config=name, num_envs=N, steps=K, D=D, order=int(env.mdps[0].order))

        env.set_linear_policy(theta2, history=2)
        row["history2_kernel"] = env.linear_kernel_name(K)
        h2, row["history2_all_us"] = timed_us(env, lambda: env.rollout_linear(K, out=out), args.repeats)
        row["history2_summary_kernel"] = env.linear_kernel_name(K, summary=True)
        summary = env.episode_summary()
        h2s, row["history2_summary_all_us"] = timed_us(env, lambda: env.rollout_linear(K, summary=summary), args.repeats)
        env.set_linear_policy(theta1)
        row["history1_kernel"] = env.linear_kernel_name(K)
        h1, row["history1_all_us"] = timed_us(env, lambda: env.rollout_linear(K, out=out), args.repeats)

        W, V, b = theta2[:, :, :D].contiguous(), theta2[:, :, D:2 * D].contiguous(), theta2[:, :, 2 * D:].contiguous()

        def step_loop():
            obs = env.reset()[0]
            mem = obs.clone()                # (step() returns views of the handle's own buffers: the memory is a copy)
            first = torch.ones(N, dtype=torch.bool, device=dev)
            for _ in range(K):
                p = torch.where(first.unsqueeze(1), obs, mem)
                a = torch.baddbmm(torch.baddbmm(b, W, obs.unsqueeze(2)), V, p.unsqueeze(2)).squeeze(2).clamp_(-amax, amax)
                mem.copy_(obs)
                obs, _, term, trunc = env.step(a)[:4]
                first = term.bool() | trunc.bool()
        loop, row["step_loop_all_us"] = timed_us(env, step_loop, args.repeats)

        E1, E2 = D * (D + 1), D * (2 * D + 1)
        row.update(history2_us=round(h2, 1), history2_summary_us=round(h2s, 1), history1_us=round(h1, 1), step_loop_us=round(loop, 1),
                   speedup_vs_step_loop=round(loop / h2, 2), history2_over_history1=round(h2 / h1, 3),
                   summary_over_full=round(h2s / h2, 3), env_steps_per_s=round(N * K / (h2 * 1e-6), 0),
                   param_bytes_per_env_step=dict(history1=4 * E1, history2=4 * E2), memory_bytes_per_env_step=8 * D,
                   accepted=max(row["history2_all_us"]) < min(row["step_loop_all_us"]))
        ok = ok and row["accepted"]
        print(json.dumps(row), flush=True)
        rows.append(row)
        env.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(dev), accepted=ok, rows=rows), f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
