"""Per-episode epsilon / alpha schedules of the in-kernel learners: the scheduled launch (set_learner_schedule + rollout_learn)
against the unscheduled per-env-parameter launch it extends, and against the loop a user needs without it -- one step() per
step plus torch kernels doing the same epsilon-greedy Q-learning on an [N, S, A] tensor, WITH the per-env episode counter and
the epsilon lookup in torch (tools/time_learn_rollout.py's loop plus those two).

    python tools/time_learn_schedule.py [--envs 65536] [--steps 512] [--repeats 5] [--out profiles/learn_schedule.json]
                                        [--parent-runs A.json B.json --branch-runs C.json D.json]

Shapes: BASELINE cfg2 (S = A = 8, delay 4, sequence_length 3) and the reference's tabular-agent shape (S = A = 8,
sequence_length 1, delay 0, transition_noise and reward_noise named at 0), numpy streams, Q-learning.  Each figure is the
median of --repeats timings after a warm-up of every timed form, taken with the library's HIP events on the caller's stream:
  pe_us              one rollout_learn(K) launch with per-env alpha, no schedule (the PE form)
  sched_const_us     the SCHED form with one constant row of M = 1000 entries at the same epsilon
  sched_tune_us      the SCHED form with the 9-row schedule of the reference's *_tabular_tune_hps.py sweep: epsilon 0.1 / 0.01 /
                     0.001 x "linear" / "log" / "const" over M = 1000 episodes (row i % 9), alpha 0.1 / 0.3 / 0.5 per env
  sched_summary_us   the same keeping episode summaries (rollout_learn(K, summary=))
  step_loop_us       K x { epsilon[row, min(ep, M - 1)] in torch;  epsilon-greedy action from Q;  step();  Q-learning update;
                           ep += terminated | truncated }
sched_over_pe = sched_tune_us / pe_us is recorded, not gated.  The tool exits with status 1 unless the scheduled launch is at
least --min-speedup (2) times faster than the step() loop on every shape.

--parent-runs / --branch-runs: outputs of tools/time_learn_sweep.py --out from the parent commit's tree and from this one,
taken alternately in one session.  Every launch figure of theirs (the learner forms that existed before the schedule; the
step() loop and the nine-handle loop are host-bound and left out) is folded in as a `no_regression` row: the branch median
must lie within parent median x (1 + parent spread), spread = (max - min) / median over the parent's repeats -- the rule of
profiles/closed_loop_refactor.json.
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

from mdp_playground_amd import RLToyVectorEnv, policy  # noqa: E402

BASE = dict(state_space_type="discrete", action_space_type="discrete", seed=0)
_TAB = dict(BASE, state_space_size=8, action_space_size=8, delay=0, sequence_length=1)
CONFIGS = {
    "cfg2": dict(BASE, state_space_size=8, action_space_size=8, delay=4, sequence_length=3),
    "tabular_s8_noise_keys_at_0": dict(_TAB, transition_noise=0.0, reward_noise=0.0),
}
GAMMA, EPS = 0.9, 0.1
M = 1000
TUNE_EPS, TUNE_KINDS, TUNE_ALPHA = (1e-1, 1e-2, 1e-3), ("linear", "log", "const"), (0.1, 0.3, 0.5)


def tune_hps_schedule(n):
    """(epsilon float64 [9, M], row int32 [n], alpha float32 [n]) of the sweep; "log" ends at a hundredth of its start"""
    rows = [policy.epsilon_decay(kind, e, M, e / 100.0 if kind == "log" else 0.0) for e in TUNE_EPS for kind in TUNE_KINDS]
    i = np.arange(n)
    return np.stack(rows), (i % 9).astype(np.int32), np.asarray(TUNE_ALPHA, np.float32)[(i // 9) % 3]


FOLDED = ("q_learning", "sarsa", "q_learning_pe", "sarsa_pe", "double", "double_global", "double_pe", "sweep_one_handle")


def fold_runs(parent_files, branch_files):
    """no_regression rows from alternated runs of tools/time_learn_sweep.py on the two trees"""
    def gather(files):
        acc = {}
        for f in files:
            for row in json.load(open(f))["rows"]:
                for fig in FOLDED:
                    acc.setdefault((row["config"], fig + "_us"), []).extend(row["all_us"][fig])
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


def timed_us(env, fn, repeats):
    fn()                                    # warm-up: code objects, allocator, the fill of the parameter arrays
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
    ap.add_argument("--parent-runs", nargs="*", default=[])
    ap.add_argument("--branch-runs", nargs="*", default=[])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    N, K = args.envs, args.steps
    eps_tab, row, alpha = tune_hps_schedule(N)
    rows, ok = [], True
    for name, cfg in CONFIGS.items():
        env = RLToyVectorEnv(num_envs=N, device=dev, **cfg)
        S, A = env.mdps[0].S, env.mdps[0].A
        out = env.alloc_rollout_learn(K)
        learn = lambda: env.rollout_learn(K, out=out)                       # noqa: E731
        env.set_learner("q_learning", alpha=alpha, gamma=GAMMA, epsilon=EPS, seed=1)
        pe, pe_all = timed_us(env, learn, args.repeats)
        pe_kernel = env.learn_kernel_name(K)
        env.set_learner_schedule(epsilon=np.full(M, EPS))
        const, const_all = timed_us(env, learn, args.repeats)
        env.set_learner_schedule(epsilon=eps_tab, row=row)
        summary = env.episode_summary()
        summ, summ_all = timed_us(env, lambda: env.rollout_learn(K, summary=summary), args.repeats)
        env.set_learner_schedule(epsilon=eps_tab, row=row)                  # (the counters start again)
        tune, tune_all = timed_us(env, learn, args.repeats)
        kernel = env.learn_kernel_name(K)
        episodes = env.learner_episodes()                                   # after (1 + repeats) K steps
        ep_stats = [int(episodes.min()), int(episodes.median()), int(episodes.max())]
        env.set_learner(None)

        Q = torch.zeros((N, S, A), dtype=torch.float32, device=dev)
        idx = torch.arange(N, device=dev)
        eps_dev = torch.as_tensor(eps_tab.astype(np.float32), device=dev)
        row_dev = torch.as_tensor(row, device=dev).long()
        alpha_dev = torch.as_tensor(alpha, device=dev)
        ep = torch.zeros(N, dtype=torch.long, device=dev)

        def step_loop():
            obs = (env._obs if env._obs_src is None else env._obs_src).long()
            for _ in range(K):
                eps = eps_dev[row_dev, ep.clamp(max=M - 1)]
                greedy = Q[idx, obs].argmax(dim=1)
                explore = torch.rand(N, device=dev) < eps
                a = torch.where(explore, torch.randint(0, A, (N,), device=dev), greedy)
                nobs, r, term, trunc, _ = env.step(a.to(torch.int32))
                nobs = nobs.long()
                y = torch.where(term, r, r + GAMMA * Q[idx, nobs].max(dim=1).values)
                q = Q[idx, obs, a]
                Q[idx, obs, a] = q + alpha_dev * (y - q)
                ep.add_(term | trunc)
                obs = nobs
        loop, loop_all = timed_us(env, step_loop, args.repeats)
        assert not env.status().any()
        env.close()

        r = dict(config=name, num_envs=N, steps=K, schedule_rows=9, schedule_entries=M, pe_us=round(pe, 1), sched_const_us=round(const, 1),
                 sched_tune_us=round(tune, 1), sched_summary_us=round(summ, 1), step_loop_us=round(loop, 1),
                 sched_over_pe=round(tune / pe, 3), sched_const_over_pe=round(const / pe, 3), summary_over_full=round(summ / tune, 3),
                 speedup_vs_step_loop=round(loop / tune, 2), env_steps_per_s=round(N * K / (tune * 1e-6), 0),
                 episodes_min_median_max=ep_stats, pe_kernel=pe_kernel, sched_kernel=kernel,
                 pe_all_us=pe_all, sched_const_all_us=const_all, sched_tune_all_us=tune_all, sched_summary_all_us=summ_all, step_loop_all_us=loop_all)
        ok = ok and loop / tune >= args.min_speedup
        print(json.dumps(r), flush=True)
        rows.append(r)
    result = dict(device=torch.cuda.get_device_name(dev), gamma=GAMMA, epsilon=EPS, min_speedup=args.min_speedup, rows=rows)
    if args.parent_runs:
        result["no_regression"], within = fold_runs(args.parent_runs, args.branch_runs)
        result["no_regression_note"] = ("tools/time_learn_sweep.py on the parent commit's tree and on this one, alternated in one session (parent, "
                                        "branch, parent, branch); rule: branch median <= parent median x (1 + parent spread)")
        ok = ok and within
    result["accepted"] = ok
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
