"""Per-env noise levels on one MDP per env: what ONE launch over a noise x seed sweep costs against one launch per level.

    python tools/time_noise_seeds.py [--envs 65535] [--steps 512] [--repeats 5] [--out profiles/noise_levels_per_env_mdp.json]
                                     [--parent-runs A.json ... --branch-runs B.json ...]

Shape: the reference's tabular-agent shape of its six noise sweeps (S = A = 8, sequence_length 1, delay 0), one MDP per env on
seeds 0 ... envs - 1 built on the device, alpha 0.3, gamma 0.9, epsilon 0.1.  Each figure is the median of --repeats timings
after a warm-up of every timed form, taken with the library's HIP events on the caller's stream, for numpy and Philox
streams, Q-learning and double Q-learning:
  p_sweep_one_handle_us      (a) ONE handle over all seeds holding the five transition_noise levels {0, 0.01, 0.02, 0.10, 0.25},
                             envs // 5 envs each (set_learner and set_noise_levels with per_env_mdp=True): one rollout_learn(K)
  p_sweep_five_handles_us    (b) five uniform per-env-MDP handles of envs // 5 envs (their fifth of the seeds), one level each,
                             launched one after the other
  r_sweep_one_handle_us / r_sweep_five_handles_us    the same for the five reward_noise levels {0, 1, 5, 10, 25}
  nlev_equal_us / pe_uniform_us    (c) what NLEV costs: ALL levels equal (p = 0.1, sigma = 1) against the uniform per-env-MDP
                             handle created at those values (its launch is the PE form already)
  placement_<options>_us     (d) the one-handle transition sweep in each placement the kernel options reach
The tool exits with status 1 unless every one-handle sweep is at least --min-ratio (2) times faster than its five handles; (c)
and (d) are recorded, not gated.

--parent-runs / --branch-runs: outputs (--out) of tools/time_learn_rollout.py, tools/time_learn_seeds.py and
tools/time_noise_levels.py from the parent commit's tree and from this one, taken alternately in one session.  Every list of
repeats found under the same path in both is folded in as a `no_regression` row: the branch median must lie within parent
median x (1 + parent spread), spread = (max - min) / median over the parent's repeats (the rule of
profiles/closed_loop_refactor.json).
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

TABULAR = dict(state_space_type="discrete", action_space_type="discrete", state_space_size=8, action_space_size=8, delay=0,
               sequence_length=1)
ALPHA, GAMMA, EPS = 0.3, 0.9, 0.1
SWEEPS = {"p": ("transition_noise", (0.0, 0.01, 0.02, 0.10, 0.25)), "r": ("reward_noise", (0.0, 1.0, 5.0, 10.0, 25.0))}
# (what the one handle is created with: the key of its sweep, transition_noise > 0)
CREATED = {"p": dict(transition_noise=0.25), "r": dict(reward_noise=1.0)}
PLACEMENTS = [("NO_PM_NLEV_LDS",), ("NO_PM_LDS",), ("NO_PM_LDS", "NO_PM_NLEV_LDS"), ("NO_LEARN_LDS",), ("NO_LEARN_LDS", "NO_PM_NLEV_LDS"),
              ("NO_LEARN_LDS", "NO_PM_LDS"), ("NO_LEARN_LDS", "NO_PM_LDS", "NO_PM_NLEV_LDS")]


def timed_us(env, fn, repeats):
    fn()                                    # warm-up: code objects, allocator, the kernel's LDS attribute
    torch.cuda.synchronize(env.device)
    out = []
    for _ in range(repeats):
        env.timer_begin()
        fn()
        out.append(env.timer_end() * 1e3)
    return statistics.median(out), [round(x, 1) for x in out]


def _repeat_lists(node, path=()):
    """(path, list of timings) for every list of numbers stored under a key that ends in all_us, or inside an all_us dict"""
    if isinstance(node, dict):
        for k, v in node.items():
            yield from _repeat_lists(v, path + (str(k),))
    elif isinstance(node, list):
        if node and all(isinstance(x, (int, float)) and not isinstance(x, bool) for x in node):
            if any(p.endswith("all_us") for p in path):
                yield path, node
        else:
            for j, v in enumerate(node):
                yield from _repeat_lists(v, path + (str(j),))


def fold_runs(parent_files, branch_files):
    """no_regression rows from alternated runs of the three older timing tools on the two trees (files pair up by name)"""
    def gather(files):
        acc = {}
        for f in files:
            tool = os.path.basename(f).split(".")[0].rstrip("0123456789_")
            for prefix in ("parent_", "branch_"):
                tool = tool[len(prefix):] if tool.startswith(prefix) else tool
            for path, v in _repeat_lists(json.load(open(f))):
                acc.setdefault((tool,) + path, []).extend(v)
        return acc
    par, br = gather(parent_files), gather(branch_files)
    rows, ok = [], True
    for key in sorted(par):
        if key not in br:
            continue
        p, b = par[key], br[key]
        pm, bm = statistics.median(p), statistics.median(b)
        ps, bs = (max(p) - min(p)) / pm, (max(b) - min(b)) / bm
        within = bm <= pm * (1 + ps)
        ok = ok and within
        rows.append(dict(figure="/".join(key), parent_all_us=p, branch_all_us=b, parent_median_us=round(pm, 1), branch_median_us=round(bm, 1),
                         parent_spread=round(ps, 4), branch_spread=round(bs, 4), bound_us=round(pm * (1 + ps), 1), within_bound=within))
    return rows, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65535)
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-ratio", type=float, default=2.0)
    ap.add_argument("--parent-runs", nargs="*", default=[])
    ap.add_argument("--branch-runs", nargs="*", default=[])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    K = args.steps
    n5 = args.envs // 5
    N = 5 * n5
    seeds = list(range(N))
    rows, ok = [], True
    for rng in ("numpy", "philox"):
        extra = dict(rng="philox", philox_seed=77) if rng == "philox" else {}
        for algo in ("q_learning", "double_q"):
            fig, alls, kernels = {}, {}, {}

            def learner(env):
                env.set_learner(algo, alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=1, per_env_mdp=True)

            def take(key, env, out, *options):
                env.set_kernel_options(*options)
                fig[key], alls[key] = timed_us(env, lambda: env.rollout_learn(K, out=out), args.repeats)
                kernels[key] = env.learn_kernel_name(K)
                env.set_kernel_options()
                assert not env.status().any()

            for sweep, (key, levels) in SWEEPS.items():
                one = RLToyVectorEnv(seeds=seeds, device=dev, **extra, **dict(TABULAR, **CREATED[sweep]))
                assert one.tables_built_on == "device"
                learner(one)
                one.set_noise_levels(**{key: np.repeat(np.asarray(levels), n5)}, per_env_mdp=True)
                out = one.alloc_rollout_learn(K)
                take(sweep + "_sweep_one_handle", one, out)
                if sweep == "p":
                    for options in PLACEMENTS:
                        take("placement" + "".join("_" + o.lower() for o in options), one, out, *options)
                one.close()
                del out
                five = [RLToyVectorEnv(seeds=seeds[j * n5:(j + 1) * n5], device=dev, env_id_offset=j * n5, **extra, **dict(TABULAR, **{key: v}))
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
                del outs

            both = dict(TABULAR, transition_noise=0.1, reward_noise=1.0)
            uni = RLToyVectorEnv(seeds=seeds, device=dev, **extra, **both)
            learner(uni)
            out = uni.alloc_rollout_learn(K)
            take("pe_uniform", uni, out)
            uni.set_noise_levels(transition_noise=np.full(N, 0.1), reward_noise=np.full(N, 1.0), per_env_mdp=True)
            take("nlev_equal", uni, out)
            uni.close()
            del out

            row = dict(rng=rng, algo=algo, num_envs=N, steps=K, envs_per_level=n5, **{k + "_us": round(v, 1) for k, v in fig.items()},
                       p_sweep_five_over_one=round(fig["p_sweep_five_handles"] / fig["p_sweep_one_handle"], 2),
                       r_sweep_five_over_one=round(fig["r_sweep_five_handles"] / fig["r_sweep_one_handle"], 2),
                       nlev_over_pe_uniform=round(fig["nlev_equal"] / fig["pe_uniform"], 3),
                       env_steps_per_s=round(N * K / (fig["p_sweep_one_handle"] * 1e-6), 0), kernels=kernels, all_us=alls)
            ok = ok and min(row["p_sweep_five_over_one"], row["r_sweep_five_over_one"]) >= args.min_ratio
            print(json.dumps(row), flush=True)
            rows.append(row)
    result = dict(device=torch.cuda.get_device_name(dev), alpha=ALPHA, gamma=GAMMA, epsilon=EPS, min_ratio=args.min_ratio,
                  bar="p_sweep_five_over_one >= min_ratio and r_sweep_five_over_one >= min_ratio in every row", rows=rows)
    if args.parent_runs:
        result["no_regression"], within = fold_runs(args.parent_runs, args.branch_runs)
        result["no_regression_note"] = ("tools/time_learn_rollout.py, tools/time_learn_seeds.py and tools/time_noise_levels.py on the parent commit's "
                                        "tree and on this one, alternated in one session; rule: branch median <= parent median x (1 + parent spread)")
        ok = ok and within
    result["accepted"] = ok
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
