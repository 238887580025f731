"""Per-env noise levels: what one launch over all levels of a noise sweep costs against one launch per level.

    python tools/time_noise_levels.py [--envs 65536] [--steps 512] [--repeats 5] [--out profiles/noise_levels.json]
                                      [--parent-runs A.json B.json --branch-runs C.json D.json]

Shape: the reference's tabular-agent shape of its six noise sweeps (S = A = 8, sequence_length 1, delay 0, seed 0), alpha 0.3,
gamma 0.9, epsilon 0.1.  Each figure is the median of --repeats timings after a warm-up, taken with the library's HIP events
on the caller's stream, for numpy and Philox streams, Q-learning and double Q-learning:
  p_sweep_one_handle_us      ONE handle holding the five transition_noise levels {0, 0.01, 0.02, 0.10, 0.25}, envs // 5 envs each
                             (set_noise_levels): one rollout_learn(K) launch
  p_sweep_five_handles_us    five uniform handles of envs // 5 envs, one level each, launched one after the other
  r_sweep_one_handle_us / r_sweep_five_handles_us    the same for the five reward_noise levels {0, 1, 5, 10, 25}
  nlev_equal_us / pe_uniform_us    what NLEV costs: the handle with ALL levels equal (p = 0.1, sigma = 1) against the uniform
                             handle created at those values, launched in its PE form (arrays of equal learner parameters)
  p_sweep_cdfs_global_us     numpy streams: the one-handle transition sweep with the per-level cdfs left in global memory
                             (NO_NLEV_LDS) -- against p_sweep_one_handle_us, whose cdfs are staged in LDS
The tool exits with status 1 unless every one-handle sweep is at least --min-ratio (2) times faster than its five handles; the
other ratios are recorded, not gated.

--parent-runs / --branch-runs: outputs of tools/time_learn_rollout.py --out and tools/time_learn_sweep.py --out from the parent
commit's tree and from this one, taken alternately in one session.  Their figures of the launches that existed before are
folded in as `no_regression` rows: the branch median must lie within parent median x (1 + parent spread), spread =
(max - min) / median over the parent's repeats (the rule of profiles/closed_loop_refactor.json).
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

TABULAR = dict(state_space_type="discrete", action_space_type="discrete", seed=0, state_space_size=8, action_space_size=8, delay=0,
               sequence_length=1)
ALPHA, GAMMA, EPS = 0.3, 0.9, 0.1
SWEEPS = {"p": ("transition_noise", (0.0, 0.01, 0.02, 0.10, 0.25)), "r": ("reward_noise", (0.0, 1.0, 5.0, 10.0, 25.0))}
# (what the one handle is created with: the key of its sweep, transition_noise > 0)
CREATED = {"p": dict(transition_noise=0.25), "r": dict(reward_noise=1.0)}


def timed_us(env, fn, repeats):
    fn()                                    # warm-up: code objects, allocator
    torch.cuda.synchronize(env.device)
    out = []
    for _ in range(repeats):
        env.timer_begin()
        fn()
        out.append(env.timer_end() * 1e3)
    return statistics.median(out), [round(x, 1) for x in out]


def fold_runs(parent_files, branch_files):
    """no_regression rows from alternated runs of tools/time_learn_rollout.py / tools/time_learn_sweep.py on the two trees"""
    def gather(files):
        acc = {}
        for f in files:
            for row in json.load(open(f))["rows"]:
                if "all_us" in row:                                  # time_learn_sweep.py: the launches, not the step() loop
                    for fig, v in row["all_us"].items():
                        if fig != "double_step_loop":
                            acc.setdefault((row["config"], fig + "_us"), []).extend(v)
                else:                                                # time_learn_rollout.py
                    for fig in ("learn", "learn_global", "sarsa"):
                        acc.setdefault((row["config"], fig + "_us"), []).extend(row[fig + "_all_us"])
        return acc
    par, br = gather(parent_files), gather(branch_files)
    rows, ok = [], True
    for key in sorted(par):
        p, b = par[key], br[key]
        pm, bm = statistics.median(p), statistics.median(b)
        ps, bs = (max(p) - min(p)) / pm, (max(b) - min(b)) / bm
        within = bm <= pm * (1 + ps)
        ok = ok and within
        rows.append(dict(config=key[0], figure=key[1], parent_all_us=p, branch_all_us=b, parent_median_us=round(pm, 1),
                         branch_median_us=round(bm, 1), parent_spread=round(ps, 4), branch_spread=round(bs, 4),
                         bound_us=round(pm * (1 + ps), 1), within_bound=within))
    return rows, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-ratio", type=float, default=2.0)
    ap.add_argument("--parent-runs", nargs="*", default=[])
    ap.add_argument("--branch-runs", nargs="*", default=[])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    N, K = args.envs, args.steps
    n5 = N // 5
    rows, ok = [], True
    for rng in ("numpy", "philox"):
        extra = dict(rng="philox", philox_seed=77) if rng == "philox" else {}
        for algo in ("q_learning", "double_q"):
            fig, alls, kernels = {}, {}, {}

            def learner(env, pe=False):
                al, ga, ep = (np.full(env.num_envs, v, np.float32) for v in (ALPHA, GAMMA, EPS)) if pe else (ALPHA, GAMMA, EPS)
                env.set_learner(algo, alpha=al, gamma=ga, epsilon=ep, seed=1)

            def take(key, env, *options):
                out = env.alloc_rollout_learn(K)
                env.set_kernel_options(*options)
                fig[key], alls[key] = timed_us(env, lambda: env.rollout_learn(K, out=out), args.repeats)
                kernels[key] = env.learn_kernel_name(K)
                env.set_kernel_options()
                assert not env.status().any()

            for sweep, (key, levels) in SWEEPS.items():
                one = RLToyVectorEnv(num_envs=5 * n5, device=dev, **extra, **dict(TABULAR, **CREATED[sweep]))
                learner(one)
                one.set_noise_levels(**{key: np.repeat(np.asarray(levels), n5)})
                take(sweep + "_sweep_one_handle", one)
                if sweep == "p" and rng == "numpy":
                    take("p_sweep_cdfs_global", one, "NO_NLEV_LDS")
                one.close()
                five = [RLToyVectorEnv(num_envs=n5, device=dev, env_id_offset=j * n5, **extra, **dict(TABULAR, **{key: v}))
                        for j, v in enumerate(levels)]
                outs = [e.alloc_rollout_learn(K) for e in five]
                for e in five:
                    learner(e)

                def five_launches():
                    for e, o in zip(five, outs):
                        e.rollout_learn(K, out=o)
                fig[sweep + "_sweep_five_handles"], alls[sweep + "_sweep_five_handles"] = timed_us(five[0], five_launches, args.repeats)
                kernels[sweep + "_sweep_five_handles"] = [e.learn_kernel_name(K) for e in five]
                for e in five:
                    e.close()

            both = dict(TABULAR, transition_noise=0.1, reward_noise=1.0)
            uni = RLToyVectorEnv(num_envs=N, device=dev, **extra, **both)
            learner(uni, pe=True)
            take("pe_uniform", uni)
            uni.close()
            eq = RLToyVectorEnv(num_envs=N, device=dev, **extra, **both)
            learner(eq, pe=True)
            eq.set_noise_levels(transition_noise=np.full(N, 0.1), reward_noise=np.full(N, 1.0))
            take("nlev_equal", eq)
            eq.close()

            row = dict(rng=rng, algo=algo, num_envs=N, steps=K, envs_per_level=n5, **{k + "_us": round(v, 1) for k, v in fig.items()},
                       p_sweep_five_over_one=round(fig["p_sweep_five_handles"] / fig["p_sweep_one_handle"], 2),
                       r_sweep_five_over_one=round(fig["r_sweep_five_handles"] / fig["r_sweep_one_handle"], 2),
                       nlev_over_pe_uniform=round(fig["nlev_equal"] / fig["pe_uniform"], 3), kernels=kernels, all_us=alls)
            if "p_sweep_cdfs_global" in fig:
                row["cdfs_global_over_lds"] = round(fig["p_sweep_cdfs_global"] / fig["p_sweep_one_handle"], 3)
            ok = ok and min(row["p_sweep_five_over_one"], row["r_sweep_five_over_one"]) >= args.min_ratio
            print(json.dumps(row), flush=True)
            rows.append(row)
    result = dict(device=torch.cuda.get_device_name(dev), alpha=ALPHA, gamma=GAMMA, epsilon=EPS, min_ratio=args.min_ratio, rows=rows)
    if args.parent_runs:
        result["no_regression"], within = fold_runs(args.parent_runs, args.branch_runs)
        result["no_regression_note"] = ("tools/time_learn_rollout.py and tools/time_learn_sweep.py on the parent commit's tree and on this one, "
                                        "alternated in one session; rule: branch median <= parent median x (1 + parent spread)")
        ok = ok and within
    result["accepted"] = ok
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
