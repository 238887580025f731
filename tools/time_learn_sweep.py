"""Double Q-learning and per-env learner hyper-parameters: what the new forms of the learner launch cost.

    python tools/time_learn_sweep.py [--envs 65536] [--steps 512] [--repeats 5] [--out profiles/learn_sweep.json]
                                     [--parent-runs A.json B.json --branch-runs C.json D.json]

Shapes: BASELINE cfg2 (S = A = 8, delay 4, sequence_length 3) and the reference's tabular-agent shape (S = A = 8,
sequence_length 1, delay 0, transition_noise and reward_noise named at 0), numpy streams.  Each figure is the median of
--repeats timings after a warm-up of every timed form, taken with the library's HIP events on the caller's stream:
  q_learning_us / sarsa_us          one rollout_learn(K) launch with uniform parameters
  q_learning_pe_us / sarsa_pe_us    the same with all three parameters per env (arrays of equal entries: the same work)
  double_us / double_global_us      double Q-learning, tables staged in LDS / left in global memory (NO_LEARN_LDS)
  double_pe_us                      double Q-learning with per-env parameters
  double_step_loop_us               K x { epsilon-greedy action from QA + QB in torch;  step();  double-Q update in torch }
  sweep_one_handle_us               ONE handle holding the nine (alpha, epsilon) points of the reference's *_tune_hps.py, each
                                    repeated over envs // 9 envs: one launch
  sweep_nine_handles_us             nine handles of envs // 9 envs with one point each, launched one after the other
The tool exits with status 1 unless the double-Q launch (both forms) is at least --min-speedup (2) times faster than the
step() loop on every shape; the other ratios are recorded, not gated.

--parent-runs / --branch-runs: outputs of tools/time_learn_rollout.py --out from the parent commit's tree and from this one,
taken alternately in one session.  Their uniform q_learning / sarsa figures are folded in as `no_regression` rows: the branch
median must lie within parent median x (1 + parent spread), spread = (max - min) / median over the parent's repeats.
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
    "tabular_s8_noise_keys_at_0": dict(BASE, state_space_size=8, action_space_size=8, delay=0, sequence_length=1, transition_noise=0.0,
                                       reward_noise=0.0),
}
ALPHA, GAMMA, EPS = 0.3, 0.9, 0.1
SWEEP = [(a, e) for a in (0.1, 0.3, 0.5) for e in (1e-1, 1e-2, 1e-3)]      # the (alpha, epsilon) grid of *_tabular_tune_hps.py


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
    """no_regression rows from alternated runs of tools/time_learn_rollout.py on the two trees"""
    def gather(files):
        acc = {}
        for f in files:
            for row in json.load(open(f))["rows"]:
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
    ap.add_argument("--min-speedup", type=float, default=2.0)
    ap.add_argument("--parent-runs", nargs="*", default=[])
    ap.add_argument("--branch-runs", nargs="*", default=[])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    N, K = args.envs, args.steps
    rows, ok = [], True
    for name, cfg in CONFIGS.items():
        env = RLToyVectorEnv(num_envs=N, device=dev, **cfg)
        S, A = env.mdps[0].S, env.mdps[0].A
        out = env.alloc_rollout_learn(K)
        run = lambda: env.rollout_learn(K, out=out)  # noqa: E731
        fig, alls, kernels = {}, {}, {}

        def take(key, algo, pe, *options):
            al, ga, ep = (np.full(N, v, np.float32) for v in (ALPHA, GAMMA, EPS)) if pe else (ALPHA, GAMMA, EPS)
            env.set_kernel_options(*options)
            env.set_learner(algo, alpha=al, gamma=ga, epsilon=ep, seed=1)
            fig[key], alls[key] = timed_us(env, run, args.repeats)
            kernels[key] = env.learn_kernel_name(K)
            env.set_kernel_options()

        take("q_learning", "q_learning", False)
        take("q_learning_pe", "q_learning", True)
        take("sarsa", "sarsa", False)
        take("sarsa_pe", "sarsa", True)
        take("double", "double_q", False)
        take("double_global", "double_q", False, "NO_LEARN_LDS")
        take("double_pe", "double_q", True)
        env.set_learner(None)

        Q = torch.zeros((N, 2, S, A), dtype=torch.float32, device=dev)
        idx = torch.arange(N, device=dev)

        def double_step_loop():
            obs = (env._obs if env._obs_src is None else env._obs_src).long()
            for _ in range(K):
                greedy = (Q[idx, 0, obs] + Q[idx, 1, obs]).argmax(dim=1)
                explore = torch.rand(N, device=dev) < EPS
                a = torch.where(explore, torch.randint(0, A, (N,), device=dev), greedy)
                nobs, r, term, _, _ = env.step(a.to(torch.int32))
                nobs = nobs.long()
                b = torch.randint(0, 2, (N,), device=dev)
                a_star = Q[idx, b, nobs].argmax(dim=1)
                y = torch.where(term, r, r + GAMMA * Q[idx, 1 - b, nobs, a_star])
                q = Q[idx, b, obs, a]
                Q[idx, b, obs, a] = q + ALPHA * (y - q)
                obs = nobs
        fig["double_step_loop"], alls["double_step_loop"] = timed_us(env, double_step_loop, args.repeats)
        assert not env.status().any()
        env.close()

        # the sweep: nine (alpha, epsilon) points in one handle / in nine
        n9 = N // 9
        al = np.repeat(np.asarray([a for a, _ in SWEEP], np.float32), n9)
        ep = np.repeat(np.asarray([e for _, e in SWEEP], np.float32), n9)
        one = RLToyVectorEnv(num_envs=9 * n9, device=dev, **cfg)
        one.set_learner("q_learning", alpha=al, gamma=GAMMA, epsilon=ep, seed=1)
        oout = one.alloc_rollout_learn(K)
        fig["sweep_one_handle"], alls["sweep_one_handle"] = timed_us(one, lambda: one.rollout_learn(K, out=oout), args.repeats)
        one.close()
        nine = [RLToyVectorEnv(num_envs=n9, device=dev, env_id_offset=j * n9, **cfg) for j in range(9)]
        outs = [e.alloc_rollout_learn(K) for e in nine]
        for e, (a, x) in zip(nine, SWEEP):
            e.set_learner("q_learning", alpha=a, gamma=GAMMA, epsilon=x, seed=1)

        def nine_launches():
            for e, o in zip(nine, outs):
                e.rollout_learn(K, out=o)
        fig["sweep_nine_handles"], alls["sweep_nine_handles"] = timed_us(nine[0], nine_launches, args.repeats)
        for e in nine:
            e.close()

        row = dict(config=name, num_envs=N, steps=K, **{k + "_us": round(v, 1) for k, v in fig.items()},
                   pe_over_uniform_q_learning=round(fig["q_learning_pe"] / fig["q_learning"], 3),
                   pe_over_uniform_sarsa=round(fig["sarsa_pe"] / fig["sarsa"], 3),
                   pe_over_uniform_double=round(fig["double_pe"] / fig["double"], 3),
                   double_over_q_learning=round(fig["double"] / fig["q_learning"], 2),
                   double_global_over_q_learning=round(fig["double_global"] / fig["q_learning"], 2),
                   double_global_over_lds=round(fig["double_global"] / fig["double"], 2),
                   double_speedup_vs_step_loop=round(fig["double_step_loop"] / fig["double"], 2),
                   double_global_speedup_vs_step_loop=round(fig["double_step_loop"] / fig["double_global"], 2),
                   sweep_envs_per_point=n9, sweep_nine_over_one=round(fig["sweep_nine_handles"] / fig["sweep_one_handle"], 2),
                   kernels=kernels, all_us=alls)
        ok = ok and fig["double_step_loop"] / max(fig["double"], fig["double_global"]) >= args.min_speedup
        print(json.dumps(row), flush=True)
        rows.append(row)
    result = dict(device=torch.cuda.get_device_name(dev), alpha=ALPHA, gamma=GAMMA, epsilon=EPS, min_speedup=args.min_speedup, rows=rows)
    if args.parent_runs:
        result["no_regression"], within = fold_runs(args.parent_runs, args.branch_runs)
        result["no_regression_note"] = ("tools/time_learn_rollout.py on the parent commit's tree and on this one, alternated in one session; "
                                        "rule: branch median <= parent median x (1 + parent spread)")
        ok = ok and within
    result["accepted"] = ok
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
