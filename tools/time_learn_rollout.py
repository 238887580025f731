"""In-kernel tabular learners: the one-launch learner (rollout_learn) against the loop a user had before it -- one step() per
step plus torch kernels doing the same epsilon-greedy Q-learning on an [N, S, A] tensor -- and against the closed-loop
policy launch of the noise-free handle.

    python tools/time_learn_rollout.py [--envs 65536] [--steps 512] [--repeats 5] [--out profiles/learn_rollout.json]

Shapes: BASELINE cfg2 (S = A = 8, delay 4, sequence_length 3) and the reference's tabular-agent shape (S = A = 8,
sequence_length 1, delay 0, transition_noise and reward_noise named at 0), numpy streams.  Each figure is the median of
--repeats timings after a warm-up of every timed form, taken with the library's HIP events on the caller's stream:
  learn_us          one rollout_learn(K) launch, Q-learning, default form (Q-tables staged in LDS)
  learn_global_us   the same with the tables left in global memory (kernel option NO_LEARN_LDS)
  sarsa_us          one rollout_learn(K) launch, SARSA
  policy_us         one rollout_policy(K) launch of the noise-free handle of the same shape (uniform policy)
  step_loop_us      K x { epsilon-greedy action from Q in torch;  step();  Q-learning update in torch }
The tool exits with status 1 unless the Q-learning launch is at least --min-speedup (2) times faster than the step() loop on
every shape; the other ratios are recorded, not gated.
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
_TAB = dict(BASE, state_space_size=8, action_space_size=8, delay=0, sequence_length=1)
CONFIGS = {
    "cfg2": (dict(BASE, state_space_size=8, action_space_size=8, delay=4, sequence_length=3), None),
    "tabular_s8_noise_keys_at_0": (dict(_TAB, transition_noise=0.0, reward_noise=0.0), _TAB),    # (config, its noise-free form)
}
ALPHA, GAMMA, EPS = 0.3, 0.9, 0.1


def timed_us(env, fn, repeats):
    fn()                                    # warm-up: code objects, allocator
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
    ap.add_argument("--min-speedup", type=float, default=2.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    N, K = args.envs, args.steps
    rows, ok = [], True
    for name, (cfg, quiet_cfg) in CONFIGS.items():
        env = RLToyVectorEnv(num_envs=N, device=dev, **cfg)
        S, A = env.mdps[0].S, env.mdps[0].A
        out = env.alloc_rollout_learn(K)
        env.set_learner("q_learning", alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=1)
        learn, learn_all = timed_us(env, lambda: env.rollout_learn(K, out=out), args.repeats)
        kernel = env.learn_kernel_name(K)
        env.set_kernel_options("NO_LEARN_LDS")
        glob, glob_all = timed_us(env, lambda: env.rollout_learn(K, out=out), args.repeats)
        kernel_global = env.learn_kernel_name(K)
        env.set_kernel_options()
        env.set_learner("sarsa", alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=1)
        sarsa, sarsa_all = timed_us(env, lambda: env.rollout_learn(K, out=out), args.repeats)
        env.set_learner(None)

        Q = torch.zeros((N, S, A), dtype=torch.float32, device=dev)
        idx = torch.arange(N, device=dev)

        def step_loop():
            obs = (env._obs if env._obs_src is None else env._obs_src).long()
            for _ in range(K):
                greedy = Q[idx, obs].argmax(dim=1)
                explore = torch.rand(N, device=dev) < EPS
                a = torch.where(explore, torch.randint(0, A, (N,), device=dev), greedy)
                nobs, r, term, _, _ = env.step(a.to(torch.int32))
                nobs = nobs.long()
                y = torch.where(term, r, r + GAMMA * Q[idx, nobs].max(dim=1).values)
                q = Q[idx, obs, a]
                Q[idx, obs, a] = q + ALPHA * (y - q)
                obs = nobs
        loop, loop_all = timed_us(env, step_loop, args.repeats)
        assert not env.status().any()
        env.close()

        pol_env = RLToyVectorEnv(num_envs=N, device=dev, **(quiet_cfg or cfg))
        pol_env.set_policy(np.full((S, A), 1.0 / A), seed=1)
        pout = pol_env.alloc_rollout_policy(K)
        pol, pol_all = timed_us(pol_env, lambda: pol_env.rollout_policy(K, out=pout), args.repeats)
        pol_env.close()

        row = dict(config=name, num_envs=N, steps=K, learn_us=round(learn, 1), learn_global_us=round(glob, 1), sarsa_us=round(sarsa, 1),
                   policy_us=round(pol, 1), step_loop_us=round(loop, 1), speedup_vs_step_loop=round(loop / learn, 2),
                   learn_over_policy=round(learn / pol, 2), global_over_lds=round(glob / learn, 2),
                   env_steps_per_s=round(N * K / (learn * 1e-6), 0), learn_kernel=kernel, learn_global_kernel=kernel_global,
                   learn_all_us=learn_all, learn_global_all_us=glob_all, sarsa_all_us=sarsa_all, policy_all_us=pol_all,
                   step_loop_all_us=loop_all)
        ok = ok and loop / learn >= args.min_speedup
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(dev), alpha=ALPHA, gamma=GAMMA, epsilon=EPS, min_speedup=args.min_speedup,
                           accepted=ok, rows=rows), f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
