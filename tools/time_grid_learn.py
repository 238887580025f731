"""Grid learners: the one-launch learner (rollout_grid_learn) against (a) the loop it replaces -- one step() per step plus torch
kernels doing the same epsilon-greedy Q-learning on an [N, S, A] tensor, as tools/time_learn_rollout.py does for discrete
handles -- and (b) the same handle's open-loop rollout() fed recorded action vectors.

    python tools/time_grid_learn.py [--envs 65536] [--steps 512] [--repeats 5] [--out profiles/grid_learn.json]

Grids: 5 x 5 with the tables staged in LDS (QLDS=1), 5 x 5 with the kernel option NO_GRID_QLDS (QLDS=0), 8 x 8 and 16 x 16
(QLDS=0: the tables do not fit); each quiet and with both noise keys; numpy streams, dense reward, same-step autoreset,
max_episode_steps 64.  Every figure is the median of --repeats timings after a warm-up of the timed form, taken with the
library's HIP events on the caller's stream; all runs are in the record.
  learn_us        one rollout_grid_learn(K) launch, Q-learning
  sarsa_us        the same, SARSA
  eval_us         one rollout_grid_eval(K) launch
  summary_us      rollout_grid_learn(K, summary=)
  rollout_us      (b) rollout(actions) of the same handle, the action vectors of a learning launch
  step_loop_us    (a) K x { epsilon-greedy action from Q in torch;  step();  Q-learning update in torch }
Acceptance (DESIGN.md 3.25's rule): on every row the SLOWEST learning launch beats the FASTEST run of loop (a); the tool exits
with status 1 otherwise.  The cost against (b) and QLDS=1 against QLDS=0 are recorded, not gated.
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

BASE = dict(state_space_type="grid", reward_function="move_to_a_point", make_denser=True, seed=0)
NOISE = dict(transition_noise=0.1, reward_noise=0.25)
# name: grid side, kernel options
SHAPES = {"5x5_qlds": (5, ()), "5x5_global": (5, ("NO_GRID_QLDS",)), "8x8": (8, ()), "16x16": (16, ())}
ALPHA, GAMMA, EPS = 0.3, 0.9, 0.1


def timed_us(env, fn, repeats):
    fn()                                    # warm-up: code objects, allocator, the LDS attribute
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
    rows, ok = [], True
    vectors = torch.tensor([[1, 0], [-1, 0], [0, 1], [0, -1]], dtype=torch.int32, device=dev)
    for shape, (side, opts) in SHAPES.items():
        for noisy in (False, True):
            cfg = dict(BASE, grid_shape=(side, side), target_point=[side // 2, side // 2], **(NOISE if noisy else {}))
            env = RLToyVectorEnv(num_envs=N, device=dev, max_episode_steps=64, **cfg)
            env.set_kernel_options(*opts)
            out = env.alloc_rollout_grid(K)
            env.set_grid_learner("q_learning", alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=1)
            learn, learn_all = timed_us(env, lambda: env.rollout_grid_learn(K, out=out), args.repeats)
            kernel = env.grid_learn_kernel_name(K)
            ev, ev_all = timed_us(env, lambda: env.rollout_grid_eval(K, out=out), args.repeats)
            summ = env.episode_summary()
            sm, sm_all = timed_us(env, lambda: env.rollout_grid_learn(K, summary=summ), args.repeats)
            env.set_grid_learner("sarsa", alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=1)
            sarsa, sarsa_all = timed_us(env, lambda: env.rollout_grid_learn(K, out=out), args.repeats)
            acts = out[4].clone()
            env.set_grid_learner(None)
            roll, roll_all = timed_us(env, lambda: env.rollout(acts, out=out[:4]), args.repeats)
            roll_kernel = env.rollout_kernel_name(K)

            W, A = side + 1, 4
            Q = torch.zeros((N, W * W, A), dtype=torch.float32, device=dev)
            idx = torch.arange(N, device=dev)

            def step_loop():
                o = (env._obs if env._obs_src is None else env._obs_src).long()
                s = o[:, 0] * W + o[:, 1]
                for _ in range(K):
                    greedy = Q[idx, s].argmax(dim=1)
                    explore = torch.rand(N, device=dev) < EPS
                    a = torch.where(explore, torch.randint(0, A, (N,), device=dev), greedy)
                    nobs, r, term, _, info = env.step(vectors[a])
                    # (the cell after the move is the observation except where the same-step reset replaced it: the loop a
                    #  user writes bootstraps from what step() returns, and so does this one)
                    nobs = nobs.long()
                    s2 = nobs[:, 0] * W + nobs[:, 1]
                    y = torch.where(term, r, r + GAMMA * Q[idx, s2].max(dim=1).values)
                    q = Q[idx, s, a]
                    Q[idx, s, a] = q + ALPHA * (y - q)
                    s = s2
            loop, loop_all = timed_us(env, step_loop, args.repeats)
            assert not env.status().any()
            env.close()

            slowest_fused = max(learn_all + sarsa_all)
            accepted = slowest_fused < min(loop_all)
            row = dict(shape=shape, noise=noisy, num_envs=N, steps=K, learn_us=round(learn, 1), sarsa_us=round(sarsa, 1), eval_us=round(ev, 1),
                       summary_us=round(sm, 1), rollout_us=round(roll, 1), step_loop_us=round(loop, 1),
                       speedup_vs_step_loop=round(loop / learn, 2), learn_over_rollout=round(learn / roll, 2),
                       env_steps_per_s=round(N * K / (learn * 1e-6), 0), slowest_learn_us=slowest_fused, fastest_step_loop_us=min(loop_all),
                       accepted=accepted, learn_kernel=kernel, rollout_kernel=roll_kernel, learn_all_us=learn_all, sarsa_all_us=sarsa_all,
                       eval_all_us=ev_all, summary_all_us=sm_all, rollout_all_us=roll_all, step_loop_all_us=loop_all)
            ok = ok and accepted
            print(json.dumps(row), flush=True)
            rows.append(row)
    by = {(r["shape"], r["noise"]): r for r in rows}
    placement = {("noise" if nz else "quiet"): dict(qlds_us=by["5x5_qlds", nz]["learn_us"], global_us=by["5x5_global", nz]["learn_us"],
                                                     qlds_no_slower=by["5x5_qlds", nz]["learn_us"] <= by["5x5_global", nz]["learn_us"])
                 for nz in (False, True)}
    print(json.dumps(dict(placement_5x5=placement, accepted=ok)), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(dev), alpha=ALPHA, gamma=GAMMA, epsilon=EPS, accepted=ok, placement_5x5=placement,
                           rows=rows), f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
