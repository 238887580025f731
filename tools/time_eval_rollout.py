"""Greedy evaluation and in-kernel episode summaries: what the new launches cost against what they replace.

    python tools/time_eval_rollout.py [--envs 65536] [--steps 512] [--repeats 5] [--out profiles/eval_rollout.json]
                                      [--parent-learn A.json ... --branch-learn B.json ...]
                                      [--parent-policy C.json ... --branch-policy D.json ...]

Shapes: BASELINE cfg2 (S = A = 8, delay 4, sequence_length 3) and the reference's tabular-agent shape (S = A = 8,
sequence_length 1, delay 0, transition_noise and reward_noise named at 0), numpy streams, random tables.  Each figure is the
median of --repeats timings after a warm-up of every timed form, taken with the library's HIP events on the caller's stream:
  eval_us / eval_global_us       one rollout_eval(K) launch, tables staged in LDS / left in global memory (NO_LEARN_LDS)
  eval_double_us                 the same for a double-Q handle (LDS form)
  learn_us                       one rollout_learn(K) launch of the same handle (Q-learning)
  eval_step_loop_us              what rollout_eval replaces: get_q() once, then K x { gather the env's row, argmax, step() }
  learn_then_stats_us            what summary= replaces: rollout_learn(K), then stats_csv.EpisodeStats.update on its outputs
  learn_summary_us               one rollout_learn(K, summary=) launch
  eval_summary_us                one rollout_eval(K, summary=) launch
The tool exits with status 1 unless (a) both evaluation forms are at least --min-speedup (2) times faster than the step loop
on every shape and (b) learn_summary_us <= learn_then_stats_us x (1 + spread of the pair), spread = (max - min) / median.

--parent-* / --branch-*: outputs (--out) of tools/time_learn_rollout.py and tools/time_policy_rollout.py from the parent commit's
tree and from this one, taken alternately in one session.  Their figures are folded in as `no_regression` rows: the branch
median must lie within parent median x (1 + parent spread).
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
from mdp_playground_amd.stats_csv import EpisodeStats  # noqa: E402

BASE = dict(state_space_type="discrete", action_space_type="discrete", seed=0)
CONFIGS = {
    "cfg2": dict(BASE, state_space_size=8, action_space_size=8, delay=4, sequence_length=3),
    "tabular_s8_noise_keys_at_0": dict(BASE, state_space_size=8, action_space_size=8, delay=0, sequence_length=1, transition_noise=0.0,
                                       reward_noise=0.0),
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


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs)


def fold_runs(parent_files, branch_files, figures):
    """no_regression rows from alternated runs of one timing tool on the two trees"""
    def gather(files):
        acc = {}
        for f in files:
            for row in json.load(open(f))["rows"]:
                for fig in figures:
                    acc.setdefault((row["config"], fig + "_us"), []).extend(row[fig + "_all_us"])
        return acc
    par, br = gather(parent_files), gather(branch_files)
    rows, ok = [], True
    for key in sorted(par):
        p, b = par[key], br[key]
        pm, bm = statistics.median(p), statistics.median(b)
        within = bm <= pm * (1 + spread(p))
        ok = ok and within
        rows.append(dict(config=key[0], figure=key[1], parent_all_us=p, branch_all_us=b, parent_median_us=round(pm, 1),
                         branch_median_us=round(bm, 1), parent_spread=round(spread(p), 4), branch_spread=round(spread(b), 4),
                         bound_us=round(pm * (1 + spread(p)), 1), within_bound=within))
    return rows, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-speedup", type=float, default=2.0)
    for tree in ("parent", "branch"):
        for tool in ("learn", "policy"):
            ap.add_argument("--%s-%s" % (tree, tool), nargs="*", default=[])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    N, K = args.envs, args.steps
    rows, ok = [], True
    for name, cfg in CONFIGS.items():
        env = RLToyVectorEnv(num_envs=N, device=dev, **cfg)
        S, A = env.mdps[0].S, env.mdps[0].A
        gen = torch.Generator(device=dev).manual_seed(1)
        q1 = torch.randn((N, S, A), generator=gen, device=dev)
        q2 = torch.randn((N, 2, S, A), generator=gen, device=dev)
        out = env.alloc_rollout_eval(K)
        fig, alls, kernels = {}, {}, {}

        def take(key, fn, kernel=None):
            fig[key], alls[key] = timed_us(env, fn, args.repeats)
            if kernel:
                kernels[key] = kernel()

        def learner(algo, q):
            env.set_learner(algo, alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=1, q=q)

        learner("q_learning", q1)
        take("eval", lambda: env.rollout_eval(K, out=out), lambda: env.eval_kernel_name(K))
        env.set_kernel_options("NO_LEARN_LDS")
        take("eval_global", lambda: env.rollout_eval(K, out=out), lambda: env.eval_kernel_name(K))
        env.set_kernel_options()
        take("learn", lambda: env.rollout_learn(K, out=out), lambda: env.learn_kernel_name(K))

        idx = torch.arange(N, device=dev)

        def eval_step_loop():
            Q = env.get_q()
            obs = (env._obs if env._obs_src is None else env._obs_src).long()
            for _ in range(K):
                a = Q[idx, obs].argmax(dim=1)
                obs = env.step(a.to(torch.int32))[0].long()
        take("eval_step_loop", eval_step_loop)

        stats = EpisodeStats(N, dev)

        def learn_then_stats():
            _, r, te, tr, _ = env.rollout_learn(K, out=out)
            stats.update(r, te, tr)
        take("learn_then_stats", learn_then_stats)
        summ = env.episode_summary()
        take("learn_summary", lambda: env.rollout_learn(K, summary=summ))
        take("eval_summary", lambda: env.rollout_eval(K, summary=summ))
        learner("double_q", q2)
        take("eval_double", lambda: env.rollout_eval(K, out=out), lambda: env.eval_kernel_name(K))
        assert not env.status().any()
        env.close()

        pair_spread = spread(alls["learn_then_stats"])
        bound = fig["learn_then_stats"] * (1 + pair_spread)
        row = dict(config=name, num_envs=N, steps=K, **{k + "_us": round(v, 1) for k, v in fig.items()},
                   eval_speedup_vs_step_loop=round(fig["eval_step_loop"] / fig["eval"], 2),
                   eval_global_speedup_vs_step_loop=round(fig["eval_step_loop"] / fig["eval_global"], 2),
                   eval_global_over_lds=round(fig["eval_global"] / fig["eval"], 3),
                   eval_over_learn=round(fig["eval"] / fig["learn"], 3),
                   eval_ns_per_env_step=round(fig["eval"] * 1e3 / (N * K), 4),
                   learn_then_stats_spread=round(pair_spread, 4), learn_summary_bound_us=round(bound, 1),
                   learn_summary_within_bound=fig["learn_summary"] <= bound,
                   learn_summary_over_pair=round(fig["learn_summary"] / fig["learn_then_stats"], 3),
                   learn_summary_over_learn=round(fig["learn_summary"] / fig["learn"], 3),
                   eval_summary_over_eval=round(fig["eval_summary"] / fig["eval"], 3),
                   kernels=kernels, all_us=alls)
        ok = ok and fig["eval_step_loop"] / max(fig["eval"], fig["eval_global"]) >= args.min_speedup and fig["learn_summary"] <= bound
        print(json.dumps(row), flush=True)
        rows.append(row)
    result = dict(device=torch.cuda.get_device_name(dev), alpha=ALPHA, gamma=GAMMA, epsilon=EPS, min_speedup=args.min_speedup, rows=rows)
    if args.parent_learn or args.parent_policy:
        learn_rows, ok1 = fold_runs(args.parent_learn, args.branch_learn, ("learn", "learn_global", "sarsa", "policy"))
        policy_rows, ok2 = fold_runs(args.parent_policy, args.branch_policy, ("closed_loop", "open_loop"))
        result["no_regression"] = dict(time_learn_rollout=learn_rows, time_policy_rollout=policy_rows)
        result["no_regression_note"] = ("tools/time_learn_rollout.py and tools/time_policy_rollout.py on the parent commit's tree and on this "
                                        "one, alternated in one session; rule: branch median <= parent median x (1 + parent spread)")
        ok = ok and ok1 and ok2
    result["accepted"] = ok
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
