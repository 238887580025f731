"""Closed-loop continuous rollouts under a linear policy per env: the fused launch (rollout_linear) against the loop it
replaces -- one step() per step plus torch's baddbmm + clamp on the handle's observation -- and against the open-loop launch of
the same handle on precomputed actions.

    python tools/time_linear_rollout.py [--envs 65536] [--steps 512] [--repeats 5] [--out profiles/linear_rollout.json]

Shapes: bench.py's c_d2_n0, cfg3 and cfg5, numpy streams.  Each figure is the median of --repeats timings after a warm-up of
the timed form, taken with the library's HIP events on the caller's stream (mdpp_timer_begin / mdpp_timer_end); every run is
kept in the record.  Legs per shape:
  per_env_us        one rollout_linear(K) launch, one parameter set per env, the default placement (the kernel's name says which)
  per_env_no_lds_us the same under MDPP_OPT_NO_LINEAR_LDS (PLDS=0: the parameters are re-read from memory at every step)
  shared_us         one policy shared by every env
  summary_us        rollout_linear(K, summary=): no [K, N] output
  step_loop_us      K x { a = clamp(baddbmm(b, W, obs)) in torch;  obs = step(a) }
  open_loop_us      one rollout(actions) launch fed with the actions of a closed-loop launch
Acceptance: on every shape the slowest of the per_env runs is faster than the fastest of the step-loop runs (the fused launch
wins by more than the spread of the runs).  No ratio is fixed in advance; the ratios are recorded.
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

_C12 = dict(state_space_type="continuous", state_space_dim=12, relevant_indices=[0, 1, 2, 3], irrelevant_features=True,
            target_point=[0, 0, 0, 0], target_radius=0.05, state_space_max=10, action_space_max=1, inertia=1, make_denser=True,
            reward_function="move_to_a_point", seed=0)
CONFIGS = {
    "c_d2_n0": dict(state_space_type="continuous", action_space_type="continuous", state_space_dim=2, action_space_dim=2,
                    transition_dynamics_order=1, inertia=1, time_unit=1.0, state_space_max=10, action_space_max=1,
                    target_point=[0, 0], target_radius=0.5, make_denser=True, reward_function="move_to_a_point",
                    action_loss_weight=0.01, delay=0, reward_scale=1.0, transition_noise=0, reward_noise=0, seed=0),
    "cfg3": dict(_C12, transition_dynamics_order=1, time_unit=1),
    "cfg5": dict(_C12, transition_dynamics_order=2, time_unit=0.1, transition_noise=0.05, reward_noise=0.05),
}


def draw_theta(n, d, seed=0):
    """a contracting part -g I, g in [0, 2] per env, plus a small random part (as the tests draw their policies)"""
    r = np.random.default_rng(seed)
    th = np.zeros((n, d, d + 1))
    th[:, :, :d] = r.uniform(-0.2, 0.2, (n, d, d))
    th[:, :, d] = r.uniform(-0.01, 0.01, (n, d))
    th[:, np.arange(d), np.arange(d)] -= r.uniform(0.0, 2.0, n)[:, None]
    return th.astype(np.float32)


def timed_us(env, fn, repeats):
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
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    N, K = args.envs, args.steps
    rows, ok = [], True
    for name in args.configs.split(","):
        cfg = CONFIGS[name]
        env = RLToyVectorEnv(num_envs=N, device=dev, **cfg)
        D, amax = env.mdps[0].D, float(env.mdps[0].action_space_max)
        theta = torch.from_numpy(draw_theta(N, D)).to(dev)
        env.reset()
        out = env.alloc_rollout_linear(K)
        row = dict(config=name, num_envs=N, steps=K, D=D)

        env.set_linear_policy(theta)
        row["per_env_kernel"] = env.linear_kernel_name(K)
        per_env, row["per_env_all_us"] = timed_us(env, lambda: env.rollout_linear(K, out=out), args.repeats)
        actions = out[4].clone()
        row["summary_kernel"] = env.linear_kernel_name(K, summary=True)
        summary = env.episode_summary()
        summ, row["summary_all_us"] = timed_us(env, lambda: env.rollout_linear(K, summary=summary), args.repeats)
        env.set_kernel_options("NO_LINEAR_LDS")
        row["per_env_no_lds_kernel"] = env.linear_kernel_name(K)
        no_lds, row["per_env_no_lds_all_us"] = timed_us(env, lambda: env.rollout_linear(K, out=out), args.repeats)
        env.set_kernel_options()
        env.set_linear_policy(theta[0])
        row["shared_kernel"] = env.linear_kernel_name(K)
        shared, row["shared_all_us"] = timed_us(env, lambda: env.rollout_linear(K, out=out), args.repeats)
        row["open_loop_kernel"] = env.rollout_kernel_name(K)
        open_, row["open_loop_all_us"] = timed_us(env, lambda: env.rollout(actions, out=out[:4]), args.repeats)

        W, b = theta[:, :, :D].contiguous(), theta[:, :, D:].contiguous()

        def step_loop():
            obs = env.reset()[0]
            for _ in range(K):
                a = torch.baddbmm(b, W, obs.unsqueeze(2)).squeeze(2).clamp_(-amax, amax)
                obs = env.step(a)[0]
        loop, row["step_loop_all_us"] = timed_us(env, step_loop, args.repeats)

        # bytes per env step: the PLDS=0 form re-reads D (D + 1) float32 parameters at every step
        row.update(per_env_us=round(per_env, 1), per_env_no_lds_us=round(no_lds, 1), shared_us=round(shared, 1),
                   summary_us=round(summ, 1), step_loop_us=round(loop, 1), open_loop_us=round(open_, 1),
                   speedup_vs_step_loop=round(loop / per_env, 2), closed_over_open=round(per_env / open_, 2),
                   no_lds_over_default=round(no_lds / per_env, 2), summary_over_full=round(summ / per_env, 2),
                   env_steps_per_s=round(N * K / (per_env * 1e-6), 0),
                   no_lds_param_bytes_per_env_step=4 * D * (D + 1),
                   no_lds_param_GBps=round(4 * D * (D + 1) * N * K / (no_lds * 1e-6) / 1e9, 1),
                   accepted=max(row["per_env_all_us"]) < min(row["step_loop_all_us"]))
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
