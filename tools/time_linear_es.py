"""Linear policy ES inside the launch (rollout_linear(K, es=)) against what it replaces.

    python tools/time_linear_es.py [--envs 65536] [--steps 512] [--repeats 5] [--limit 32] [--out profiles/linear_es.json]

Shapes: bench.py's c_d2_n0, cfg3 and cfg5 with max_episode_steps = --limit, numpy streams, one episode per member.  Each figure
is the median of --repeats timings after a warm-up of the timed form, taken with the library's HIP events on the caller's
stream (mdpp_timer_begin / mdpp_timer_end); every run is kept in the record.  Legs per shape:
  es_us, es_summary_us     (a) one rollout_linear(K, es=) launch, full output, and one rollout_linear(K, summary=, es=) launch
  step_es_us               (b) the loop the launch replaces: K x { rollout_linear(1, summary=); the per-env episode bookkeeping,
                           the group vote, the ranks, the mean's update and the next candidates in torch; set_linear_policy },
                           with no host synchronisation -- so the generation end is computed at every step and applied where
                           the vote passed
  linear_summary_us        (c) rollout_linear(K, summary=) without any search at the same shape and policies
  search_summary_us        (d) the (1+1)-ES launch rollout_linear(K, summary=, search=) on the same handle
  *_lockstep_us            (a), (c) and (d) again from a zero mean with a tiny sigma and lr = 0 (the same work: the mean moves by
                           gain * S = 0), under which no env moves and every env ends its episodes at the same step
  waiting_share, spare_share
                           the share of env steps a member spends waiting for an episode boundary (eps == -1) or on spare
                           episodes (eps == T), restated in torch from the full-output launch's own flags, for both policies
Acceptance: on every shape the slowest run of (a), either form, is faster than the fastest run of (b)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mdp_playground_amd import RLToyVectorEnv  # noqa: E402
from tools.time_linear_rollout import CONFIGS, draw_theta, timed_us  # noqa: E402
from tools.time_linear_search import DOWN, UP  # noqa: E402

SIGMA, LR, STILL = 0.05, 0.1, 1e-6


class TorchES:
    """the same ES kept on the host side of the launch, in torch, with torch's normals: no host synchronisation"""

    def __init__(self, env, mean, sigma, lr):
        self.env, self.G, dev = env, env.num_envs // 64, env.device
        G, E = self.G, mean[0].numel()
        self.mean = mean.reshape(G, 1, E).clone()
        self.sigma, self.gain = sigma, lr / (sigma * 4032.0)
        self.sign = torch.tensor([1.0, -1.0], device=dev).repeat(32).reshape(1, 64, 1)
        self.z = torch.randn((G, 32, E), device=dev).repeat_interleave(2, dim=1)
        self.acc = torch.zeros((G, 64), dtype=torch.float64, device=dev)
        self.eps = torch.zeros((G, 64), dtype=torch.int32, device=dev)
        self.shape = tuple(mean.shape[1:])
        self.summary = env.episode_summary()
        self.push()

    def push(self):
        cand = self.mean + self.sigma * self.sign * self.z
        self.env.set_linear_policy(cand.reshape((self.env.num_envs,) + self.shape))

    def after_step(self):
        """T = 1 after a one-step launch: the summary shows whether the env's episode ended and with what return"""
        s, G = self.summary, self.G
        ended = (s.episodes > 0).reshape(G, 64)
        counting = self.eps == 0
        self.acc = torch.where(ended & counting, s.return_sum.reshape(G, 64), self.acc)
        self.eps = torch.where(ended & counting, 1, torch.where(ended & (self.eps < 0), 0, self.eps)).to(torch.int32)
        s.ret.masked_fill_(~counting.reshape(-1) | ended.reshape(-1), 0.0)       # (a waiting or spare episode is not summed)
        s.episodes.zero_(); s.return_sum.zero_(); s.length_sum.zero_()
        done = (self.eps == 1).all(dim=1)                                         # the vote, [G]
        key = torch.nan_to_num(self.acc, nan=-float("inf"))
        lt = (key[:, None, :] < key[:, :, None]).sum(-1)
        eq = (key[:, None, :] == key[:, :, None]).sum(-1) - 1
        r = (2 * lt + eq - 63).to(torch.float32)
        step = self.gain * (r[:, :, None] * self.sign * self.z).sum(dim=1, keepdim=True)
        d = done[:, None, None]
        self.mean = torch.where(d, self.mean + step, self.mean)
        self.z = torch.where(d, torch.randn((G, 32, self.z.shape[2]), device=self.z.device).repeat_interleave(2, dim=1), self.z)
        self.acc = torch.where(done[:, None], 0.0, self.acc)
        self.eps = torch.where(done[:, None], torch.where(ended, 0, -1), self.eps).to(torch.int32)
        self.push()

    def run(self, steps):
        for _ in range(steps):
            self.env.rollout_linear(1, summary=self.summary)
            self.after_step()


def shares(term, trunc):
    """(waiting, spare) shares of the env steps of a T = 1 launch, from its flags [K, N] (same-step autoreset: no reset calls)"""
    end = (term | trunc).bool()
    K, N = end.shape
    eps = torch.zeros((N // 64, 64), dtype=torch.int32, device=end.device)
    waiting = torch.zeros((), dtype=torch.int64, device=end.device)
    spare = torch.zeros_like(waiting)
    for k in range(K):
        e = end[k].reshape(-1, 64)
        waiting += (eps < 0).sum()
        spare += (eps == 1).sum()
        eps = torch.where(e & (eps == 0), 1, torch.where(e & (eps < 0), 0, eps))
        done = (eps == 1).all(dim=1, keepdim=True)
        eps = torch.where(done, torch.where(e, 0, -1), eps).to(torch.int32)
    return round(float(waiting) / (K * N), 4), round(float(spare) / (K * N), 4)


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
    G = N // 64
    rows, ok = [], True
    for name in args.configs.split(","):
        env = RLToyVectorEnv(num_envs=N, device=dev, max_episode_steps=L, **CONFIGS[name])
        D = env.mdps[0].D
        theta = torch.from_numpy(draw_theta(N, D)).to(dev)
        mean = torch.from_numpy(draw_theta(G, D, seed=1)).to(dev)
        zero = torch.zeros_like(mean)
        out = env.alloc_rollout_linear(K)
        summary = env.episode_summary()
        row = dict(config=name, num_envs=N, groups=G, steps=K, D=D, max_episode_steps=L, episodes_per_member=1, sigma=SIGMA, lr=LR)

        def fresh(start, sigma, lr=LR):
            env.reset()
            env.set_linear_policy(theta)
            summary.clear()
            return env.linear_es(start, sigma, lr, seed=1)

        for tag, start, sigma, lr in (("", mean, SIGMA, LR), ("_lockstep", zero, STILL, 0.0)):
            es = fresh(start, sigma, lr)
            row["es_kernel"] = env.linear_kernel_name(K, es=True)
            full, row["es%s_all_us" % tag] = timed_us(env, lambda: env.rollout_linear(K, out=out, es=es), args.repeats)
            es = fresh(start, sigma, lr)                                       # (one launch from a fresh start, not timed: the shares)
            env.rollout_linear(K, out=out, es=es)
            row["waiting_share" + tag], row["spare_share" + tag] = shares(out[2], out[3])
            row["generations_per_group_mean" + tag] = round(float(es.gen.double().mean()), 1)
            es = fresh(start, sigma, lr)
            row["es_summary_kernel"] = env.linear_kernel_name(K, summary=True, es=True)
            summ, row["es_summary%s_all_us" % tag] = timed_us(env, lambda: env.rollout_linear(K, summary=summary, es=es), args.repeats)
            row["episode_length_mean" + tag] = round(float(summary.length_sum.double().sum() / summary.episodes.double().sum()), 2)
            # (c) the same candidates without any search, (d) the (1+1)-ES from them
            fresh(start, sigma, lr)
            plain, row["linear_summary%s_all_us" % tag] = timed_us(env, lambda: env.rollout_linear(K, summary=summary), args.repeats)
            fresh(start, sigma, lr)
            search = env.linear_search(sigma, seed=1, sigma_up=UP, sigma_down=DOWN)
            one, row["search_summary%s_all_us" % tag] = timed_us(env, lambda: env.rollout_linear(K, summary=summary, search=search), args.repeats)
            row.update({"es%s_us" % tag: round(full, 1), "es_summary%s_us" % tag: round(summ, 1), "linear_summary%s_us" % tag: round(plain, 1),
                        "search_summary%s_us" % tag: round(one, 1), "es_over_linear" + tag: round(summ / plain, 3),
                        "es_over_search" + tag: round(summ / one, 3)})

        env.reset()
        env.set_linear_policy(theta)
        host = TorchES(env, mean, SIGMA, LR)
        step, row["step_es_all_us"] = timed_us(env, lambda: host.run(K), args.repeats)
        slowest_a = max(row["es_all_us"] + row["es_summary_all_us"])
        row.update(step_es_us=round(step, 1), speedup_vs_step_es=round(step / row["es_us"], 2),
                   summary_speedup_vs_step_es=round(step / row["es_summary_us"], 2),
                   env_steps_per_s=round(N * K / (row["es_summary_us"] * 1e-6), 0), accepted=slowest_a < min(row["step_es_all_us"]))
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
