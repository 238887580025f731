"""Per-env noise levels of grid handles: a five-level noise sweep as ONE learner launch against the five launches it replaces,
and what the NLEV form of the kernel costs.

    python tools/time_grid_noise_levels.py [--envs 65536] [--steps 512] [--repeats 5] [--out profiles/grid_noise_levels.json]

Grids: 5 x 5 (the tables staged in LDS, QLDS=1), 8 x 8 and 16 x 16 (QLDS=0), created with both noise keys; numpy streams, dense
reward, same-step autoreset, max_episode_steps 64, Q-learning, epsilon 0.1.  The levels are the reference's own sweeps, paired:
transition_noise 0, 0.01, 0.02, 0.10, 0.25 with reward_noise 0, 1, 5, 10, 25.  Every figure is the median of --repeats timings
after a warm-up of the timed form, taken with the library's HIP events on the caller's stream.  Before every timed run (outside
the timing) the env is reset and the learner set anew, so every run is the first K steps of learning from zero tables.  All
runs are in the record.
  (a) mixed_us      one handle of N envs, level = i % 5, one rollout_grid_learn(K, out=) on the NLEV kernel
  (b) five_us       what a user does without levels: five uniform handles of N // 5 envs, one per level (transition_noise = 0: a
                    handle without that key), launched in a row on one stream and timed as one
  (c) uniform_us    one uniform handle of N envs at the middle level on the existing NOISE=1 kernel
  (d) uniform_nlev_us   the same handle with the middle level set everywhere through set_grid_noise_levels: the NLEV kernel
Acceptance (DESIGN.md 3.17's rule): on every row the SLOWEST run of (a) beats the FASTEST run of (b); the tool exits with status
1 otherwise.  (d)/(c), the form's own cost like for like, and (a)/(c) are recorded, not gated: a mixed wave does other work
than a uniform one -- lanes at p = 0 skip a draw their neighbours make, and the re-draw loop diverges more.
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

BASE = dict(state_space_type="grid", reward_function="move_to_a_point", make_denser=True, seed=0)
P_LEVELS = (0.0, 0.01, 0.02, 0.10, 0.25)
R_LEVELS = (0.0, 1.0, 5.0, 10.0, 25.0)
MIDDLE = 2
SIDES = {"5x5": 5, "8x8": 8, "16x16": 16}
ALPHA, GAMMA, EPS = 0.3, 0.9, 0.1


def timed_us(env, fn, repeats, before):
    """env: the handle whose events time fn (every launch of fn goes to the same stream)"""
    before()
    fn()                                    # warm-up: code objects, allocator, the LDS attribute
    torch.cuda.synchronize(env.device)
    out = []
    for _ in range(repeats):
        before()
        torch.cuda.synchronize(env.device)
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
    N, K, L = args.envs, args.steps, len(P_LEVELS)
    level = np.arange(N) % L
    rows, ok = [], True
    for shape, side in SIDES.items():
        cfg = dict(BASE, grid_shape=(side, side), target_point=[side // 2, side // 2])

        def make(n, p, sigma):
            noise = dict(reward_noise=sigma, **(dict(transition_noise=p) if p else {}))
            return RLToyVectorEnv(num_envs=n, device=dev, max_episode_steps=64, **cfg, **noise)

        def fresh(*envs):
            # every timed run is the FIRST K steps of learning: new episodes, zero tables
            for e in envs:
                e.reset()
                e.set_grid_learner("q_learning", alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=1)

        # (a) one mixed launch; (c), (d) the middle level everywhere, on the same handle
        env = make(N, P_LEVELS[MIDDLE], R_LEVELS[MIDDLE])
        out = env.alloc_rollout_grid(K)
        launch = lambda: env.rollout_grid_learn(K, out=out)
        uniform, uniform_all = timed_us(env, launch, args.repeats, lambda: fresh(env))
        uniform_kernel = env.grid_learn_kernel_name(K)
        env.set_grid_noise_levels(transition_noise=P_LEVELS[MIDDLE], reward_noise=R_LEVELS[MIDDLE])
        uniform_nlev, uniform_nlev_all = timed_us(env, launch, args.repeats, lambda: fresh(env))
        env.set_grid_noise_levels(transition_noise=np.asarray(P_LEVELS)[level], reward_noise=np.asarray(R_LEVELS)[level])
        mixed, mixed_all = timed_us(env, launch, args.repeats, lambda: fresh(env))
        mixed_kernel = env.grid_learn_kernel_name(K)
        assert not env.status().any()
        env.close()
        del out
        # (b) five uniform handles of N // 5 envs, launched in a row
        five = [make(N // L, p, s) for p, s in zip(P_LEVELS, R_LEVELS)]
        outs = [e.alloc_rollout_grid(K) for e in five]

        def five_launches():
            for e, o in zip(five, outs):
                e.rollout_grid_learn(K, out=o)
        fresh(*five)
        five_kernels = [e.grid_learn_kernel_name(K) for e in five]
        five_us, five_all = timed_us(five[0], five_launches, args.repeats, lambda: fresh(*five))
        for e in five:
            assert not e.status().any()
            e.close()
        del outs
        accepted = max(mixed_all) < min(five_all)
        r = dict(shape=shape, num_envs=N, steps=K, mixed_us=round(mixed, 1), five_us=round(five_us, 1), uniform_us=round(uniform, 1),
                 uniform_nlev_us=round(uniform_nlev, 1), five_over_mixed=round(five_us / mixed, 3), nlev_over_uniform=round(uniform_nlev / uniform, 3),
                 mixed_over_uniform=round(mixed / uniform, 3), slowest_mixed_us=max(mixed_all), fastest_five_us=min(five_all), accepted=accepted,
                 envs_per_uniform_handle=N // L, mixed_kernel=mixed_kernel, uniform_kernel=uniform_kernel, five_kernels=five_kernels,
                 mixed_all_us=mixed_all, five_all_us=five_all, uniform_all_us=uniform_all, uniform_nlev_all_us=uniform_nlev_all)
        ok = ok and accepted
        print(json.dumps(r), flush=True)
        rows.append(r)
    print(json.dumps(dict(accepted=ok)), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(dev), alpha=ALPHA, gamma=GAMMA, epsilon=EPS, transition_noise=P_LEVELS,
                           reward_noise=R_LEVELS, accepted=ok, rows=rows), f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
