"""Linear policy search inside the launch (rollout_linear(K, search=)) against what it replaces.

    python tools/time_linear_search.py [--envs 65536] [--steps 512] [--repeats 5] [--limit 32] [--out profiles/linear_search.json]

Shapes: bench.py's c_d2_n0, cfg3 and cfg5 with max_episode_steps = --limit, numpy streams, one episode per trial.  Each figure
is the median of --repeats timings after a warm-up of the timed form, taken with the library's HIP events on the caller's
stream (mdpp_timer_begin / mdpp_timer_end); every run is kept in the record.  Legs per shape:
  search_us            (a) one rollout_linear(K, search=) launch, full output
  search_summary_us    (a) one rollout_linear(K, summary=, search=) launch
  step_search_us       (b) what the launch replaces in general -- episodes end at a different step in every env --: K x
                       { rollout_linear(1, summary=); the per-env episode bookkeeping, accept and perturb in torch;
                       set_linear_policy }, with no host synchronisation
  episode_search_us    (c) the fixed-length special case: launches of one episode (--limit steps) each with the accept and
                       perturb in torch between them; right only where no env terminates early.  Reported, not a bar
  linear_summary_us    (d) rollout_linear(K, summary=) without a search at the same shape: search_summary_us over it is the
                       search's overhead
  search_summary_lockstep_us, linear_summary_lockstep_us
                       (a) and (d) again from the zero policy, under which no env moves and every env of a wave ends its
                       episodes at the same step: a wave runs the trial end (E entries, one normal each) whenever ANY of its
                       64 lanes ends a trial, so per-env episode ends cost a wave up to 64 times the trial ends of one env
Acceptance: on every shape the slowest run of (a), either form, is faster than the fastest run of (b)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mdp_playground_amd import RLToyVectorEnv  # noqa: E402
from tools.time_linear_rollout import CONFIGS, draw_theta, timed_us  # noqa: E402

SIGMA, UP, DOWN = 0.05, 1.25, 0.9


class TorchSearch:
    """the same (1+1)-ES kept on the host side of the launch, in torch, with torch's normals: no host synchronisation"""

    def __init__(self, env, theta):
        n, dev = env.num_envs, env.device
        self.env, self.cand, self.best = env, theta.clone(), theta.clone()
        self.sigma = torch.full((n,), SIGMA, dtype=torch.float32, device=dev)
        self.score = torch.full((n,), -float("inf"), dtype=torch.float64, device=dev)
        self.trial = torch.zeros(n, dtype=torch.int32, device=dev)
        self.summary = env.episode_summary()

    def after_launch(self):
        """one episode per trial: an env whose summary shows a finished episode ends its trial on that episode's return"""
        s = self.summary
        ended = s.episodes > 0
        improved = ended & (s.return_sum >= self.score)
        later = ended & (self.trial > 0)
        self.sigma = torch.where(later & improved, self.sigma * UP, torch.where(later, self.sigma * DOWN, self.sigma))
        self.score = torch.where(improved, s.return_sum, self.score)
        self.best = torch.where(improved[:, None, None], self.cand, self.best)
        self.trial += ended.to(torch.int32)
        z = torch.randn_like(self.cand)
        self.cand = torch.where(ended[:, None, None], self.best + self.sigma[:, None, None] * z, self.cand)
        s.episodes.zero_(); s.return_sum.zero_(); s.length_sum.zero_()
        self.env.set_linear_policy(self.cand)

    def run(self, launches, steps):
        for _ in range(launches):
            self.env.rollout_linear(steps, summary=self.summary)
            self.after_launch()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--limit", type=int, default=32)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    N, K, L = args.envs, args.steps, args.limit
    rows, ok = [], True
    for name in args.configs.split(","):
        env = RLToyVectorEnv(num_envs=N, device=dev, max_episode_steps=L, **CONFIGS[name])
        D = env.mdps[0].D
        theta = torch.from_numpy(draw_theta(N, D)).to(dev)
        env.reset()
        out = env.alloc_rollout_linear(K)
        row = dict(config=name, num_envs=N, steps=K, D=D, max_episode_steps=L, episodes_per_trial=1, sigma=SIGMA, sigma_up=UP, sigma_down=DOWN)

        env.set_linear_policy(theta)
        search = env.linear_search(SIGMA, seed=1, sigma_up=UP, sigma_down=DOWN)
        row["search_kernel"] = env.linear_kernel_name(K, search=True)
        full, row["search_all_us"] = timed_us(env, lambda: env.rollout_linear(K, out=out, search=search), args.repeats)
        row["search_summary_kernel"] = env.linear_kernel_name(K, summary=True, search=True)
        summary = env.episode_summary()
        summ, row["search_summary_all_us"] = timed_us(env, lambda: env.rollout_linear(K, summary=summary, search=search), args.repeats)
        row["episode_length_mean"] = round(float(summary.length_sum.double().sum() / summary.episodes.double().sum()), 2)
        row["trials_per_env_mean"] = round(float(search.trial.double().mean()), 1)
        row["accepted_per_env_mean"] = round(float(search.accepted.double().mean()), 1)

        # the same launch from the zero policy: the envs stay where a reset put them, (almost) none reaches the target, and every
        # env of a wave ends its trials at the same step -- the search's cost without the divergence of per-env episode ends
        env.reset()
        env.set_linear_policy(torch.zeros_like(theta))
        still = env.linear_search(0.0, seed=1, sigma_up=UP, sigma_down=DOWN)      # (sigma 0: the same work, and the policy stays zero)
        summary.clear()
        lock, row["search_summary_lockstep_all_us"] = timed_us(env, lambda: env.rollout_linear(K, summary=summary, search=still), args.repeats)
        row["lockstep_episode_length_mean"] = round(float(summary.length_sum.double().sum() / summary.episodes.double().sum()), 2)
        plain0, row["linear_summary_lockstep_all_us"] = timed_us(env, lambda: env.rollout_linear(K, summary=summary), args.repeats)

        env.reset()
        env.set_linear_policy(theta)
        summary.clear()
        row["linear_summary_kernel"] = env.linear_kernel_name(K, summary=True)
        plain, row["linear_summary_all_us"] = timed_us(env, lambda: env.rollout_linear(K, summary=summary), args.repeats)

        host = TorchSearch(env, theta)
        env.set_linear_policy(theta)
        step, row["step_search_all_us"] = timed_us(env, lambda: host.run(K, 1), args.repeats)
        epis, row["episode_search_all_us"] = timed_us(env, lambda: host.run(K // L, L), args.repeats)

        slowest_a = max(row["search_all_us"] + row["search_summary_all_us"])
        row.update(search_us=round(full, 1), search_summary_us=round(summ, 1), linear_summary_us=round(plain, 1),
                   step_search_us=round(step, 1), episode_search_us=round(epis, 1),
                   speedup_vs_step_search=round(step / full, 2), summary_speedup_vs_step_search=round(step / summ, 2),
                   episode_search_over_search_summary=round(epis / summ, 2), search_overhead=round(summ / plain, 3),
                   search_summary_lockstep_us=round(lock, 1), linear_summary_lockstep_us=round(plain0, 1), search_overhead_lockstep=round(lock / plain0, 3),
                   env_steps_per_s=round(N * K / (summ * 1e-6), 0),
                   accepted=slowest_a < min(row["step_search_all_us"]))
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
