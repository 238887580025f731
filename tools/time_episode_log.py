"""The episode log (rollout_learn with summary= and log=): what it costs, and that the summary launches without one -- the
learner's and the evaluation's -- cost what they did.

    python tools/time_episode_log.py measure [--tree DIR] [--envs 65536] [--steps 512] [--repeats 5] [--log-episodes 1024] --out RUN.json
    python tools/time_episode_log.py fold --parent P1.json P2.json --branch B1.json B2.json [--out profiles/episode_log.json]

measure: one run on one tree (--tree: the root of another checkout, e.g. the parent commit's; default this one).  The set-up is
tools/time_eval_rollout.py's: BASELINE cfg2 and the reference's tabular-agent shape, numpy streams, random tables, Q-learning,
the library's HIP events on the caller's stream.  A launch's time depends on the state it starts from (an evaluation launch: on
the tables it runs on), so EVERY timing is taken on a fresh handle after one untimed launch of the same form: env, streams,
tables and tick are then the same for every timing of a figure, in every tree, and a figure's spread is noise.  Figures, each
the median of --repeats such timings:
  learn_summary_us / eval_summary_us    one rollout_learn(K, summary=) / rollout_eval(K, summary=) launch, no log
  learn_full_us / eval_full_us          one full-output rollout_learn(K) / rollout_eval(K) launch
  learn_log_us                          (a tree with the log) the learner's summary launch with log=, M = --log-episodes
  segment_us                            (a tree with the log) the torch pass a host would run on the learner's full outputs to cut
                                        them into episodes: cumulative sums of reward and of the end flags along K, per-env
                                        episode index, scatter of returns and lengths into [M, N]; once per repeat, after a warm-up
fold: runs taken alternately in one session (parent, branch, parent, branch) and the three comparisons:
  1  no regression   the summary launches WITHOUT a log, learner and evaluation: branch median <= parent median x (1 + parent spread)
  2  cost of the log log launch / the summary launch without one (the same state), branch runs; no bar
  3  what it replaces   the learner's log launch median <= the PARENT's full-output launch median x (1 + its spread)
spread = (max - min) / median over a figure's timings.  Exit status 1 unless 1 and 3 hold for every shape and form.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BASE = dict(state_space_type="discrete", action_space_type="discrete", seed=0)
CONFIGS = {
    "cfg2": dict(BASE, state_space_size=8, action_space_size=8, delay=4, sequence_length=3),
    "tabular_s8_noise_keys_at_0": dict(BASE, state_space_size=8, action_space_size=8, delay=0, sequence_length=1, transition_noise=0.0,
                                       reward_noise=0.0),
}
ALPHA, GAMMA, EPS = 0.3, 0.9, 0.1
FORMS = ("learn", "eval")


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs)


def measure(args):
    sys.path.insert(0, os.path.abspath(args.tree) if args.tree else ROOT)
    import torch
    from mdp_playground_amd import RLToyVectorEnv

    dev = torch.device("cuda", 0)
    N, K, M = args.envs, args.steps, args.log_episodes
    rows = []
    has_log = hasattr(RLToyVectorEnv, "episode_log")
    for name, cfg in CONFIGS.items():
        def fresh():
            env = RLToyVectorEnv(num_envs=N, device=dev, **cfg)
            S, A = env.mdps[0].S, env.mdps[0].A
            gen = torch.Generator(device=dev).manual_seed(1)
            env.set_learner("q_learning", alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=1, q=torch.randn((N, S, A), generator=gen, device=dev))
            return env

        def timed(form, variant):
            """one timing: a fresh handle, one untimed launch of the form, the timed one -- every timing of a figure starts from
            the same state in every tree (env, streams, tables and tick after exactly one launch of K steps)"""
            env = fresh()
            call = env.rollout_learn if form == "learn" else env.rollout_eval
            summ = env.episode_summary()
            if variant == "summary":
                fn = lambda: call(K, summary=summ)
            elif variant == "full":
                out = env.alloc_rollout_learn(K)
                fn = lambda: call(K, out=out)
            else:
                lg = env.episode_log(M)
                fn = lambda: call(K, summary=summ, log=lg)
            fn()
            torch.cuda.synchronize(dev)
            env.timer_begin()
            fn()
            us = round(env.timer_end() * 1e3, 1)
            extra = {}
            if variant == "log":
                extra["log_count_min_max"] = [int(lg.count.min()), int(lg.count.max())]
            if variant == "full":
                extra["kernel"] = env.learn_kernel_name(K) if form == "learn" else env.eval_kernel_name(K)
                if has_log and form == "learn":
                    def segment():
                        _, r, te, tr, _ = out
                        end = (te | tr) != 0
                        e = end.long()
                        idx = torch.cumsum(e, 0) - e                            # the episode each step belongs to
                        cr = torch.cumsum(r.double(), 0)
                        k, i = torch.nonzero(end, as_tuple=True)
                        m = idx[k, i]
                        keep = m < M
                        k, i, m = k[keep], i[keep], m[keep]
                        cum_ret = torch.zeros((M + 1, N), dtype=torch.float64, device=dev)      # row m + 1: up to the end of episode m
                        cum_len = torch.zeros((M + 1, N), dtype=torch.int64, device=dev)
                        cum_ret[m + 1, i] = cr[k, i]
                        cum_len[m + 1, i] = k + 1
                        valid = cum_len[1:] > 0
                        ret = torch.where(valid, cum_ret[1:] - cum_ret[:-1], torch.zeros((), dtype=torch.float64, device=dev))
                        ln = torch.where(valid, cum_len[1:] - cum_len[:-1], torch.zeros((), dtype=torch.int64, device=dev))
                        return ret, ln
                    segment()
                    torch.cuda.synchronize(dev)
                    env.timer_begin()
                    segment()
                    extra["segment_us"] = round(env.timer_end() * 1e3, 1)
            assert not env.status().any()
            env.close()
            return us, extra

        alls, info = {}, dict(kernels={})
        for _ in range(args.repeats):
            for form in FORMS:
                for variant in ("summary", "full") + (("log",) if has_log and form == "learn" else ()):
                    us, extra = timed(form, variant)
                    alls.setdefault(form + "_" + variant, []).append(us)
                    if "kernel" in extra:
                        info["kernels"][form] = extra["kernel"]
                    if "segment_us" in extra:
                        alls.setdefault("segment", []).append(extra["segment_us"])
                    if "log_count_min_max" in extra:
                        info.setdefault("log_count_min_max", {})[form] = extra["log_count_min_max"]
        row = dict(config=name, num_envs=N, steps=K, log_episodes=M if has_log else None, **info, all_us=alls,
                   **{k + "_us": round(statistics.median(v), 1) for k, v in alls.items()})
        print(json.dumps(row), flush=True)
        rows.append(row)
    result = dict(device=torch.cuda.get_device_name(dev), tree=args.tree or ".", rows=rows)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    return 0


def fold(args):
    def gather(files):
        acc = {}
        for f in files:
            for row in json.load(open(f))["rows"]:
                for fig, xs in row["all_us"].items():
                    acc.setdefault((row["config"], fig), []).extend(xs)
        return acc
    par, br = gather(args.parent), gather(args.branch)
    first = json.load(open(args.branch[0]))
    ok = True
    no_regression, cost, replaces = [], [], []
    for cfg in CONFIGS:
        for form in FORMS:
            p, b = par[(cfg, form + "_summary")], br[(cfg, form + "_summary")]
            pm, bm = statistics.median(p), statistics.median(b)
            within = bm <= pm * (1 + spread(p))
            ok = ok and within
            no_regression.append(dict(config=cfg, figure=form + "_summary_us", parent_all_us=p, branch_all_us=b, parent_median_us=round(pm, 1),
                                      branch_median_us=round(bm, 1), parent_spread=round(spread(p), 4), bound_us=round(pm * (1 + spread(p)), 1),
                                      within_bound=within))
            if form != "learn":                     # (rollout_eval keeps no log)
                continue
            lg = br[(cfg, form + "_log")]
            lm = statistics.median(lg)
            cost.append(dict(config=cfg, figure=form + "_log_us", log_all_us=lg, log_median_us=round(lm, 1), no_log_median_us=round(bm, 1),
                             log_over_no_log=round(lm / bm, 4), a_few_per_cent=lm / bm <= 1.05))
            full = par[(cfg, form + "_full")]
            fm = statistics.median(full)
            within = lm <= fm * (1 + spread(full))
            ok = ok and within
            replaces.append(dict(config=cfg, figure=form + "_log_us", parent_full_all_us=full, parent_full_median_us=round(fm, 1),
                                 parent_full_spread=round(spread(full), 4), bound_us=round(fm * (1 + spread(full)), 1), log_median_us=round(lm, 1),
                                 log_over_full=round(lm / fm, 4), within_bound=within,
                                 segment_us=br[(cfg, "segment")], full_plus_segment_us=round(fm + statistics.median(br[(cfg, "segment")]), 1)))
    result = dict(device=first["device"], num_envs=first["rows"][0]["num_envs"], steps=first["rows"][0]["steps"],
                  log_episodes=first["rows"][0]["log_episodes"], kernels={r["config"]: r["kernels"] for r in first["rows"]},
                  log_count_min_max={r["config"]: r["log_count_min_max"] for r in first["rows"]},
                  order="parent, branch, parent, branch in one session",
                  no_regression=no_regression, cost_of_the_log=cost, against_the_full_output_launch=replaces, accepted=ok)
    print(json.dumps(result, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    m = sub.add_parser("measure")
    m.add_argument("--tree", default=None)
    m.add_argument("--envs", type=int, default=65536)
    m.add_argument("--steps", type=int, default=512)
    m.add_argument("--repeats", type=int, default=5)
    m.add_argument("--log-episodes", type=int, default=1024)
    m.add_argument("--out", required=True)
    f = sub.add_parser("fold")
    f.add_argument("--parent", nargs="+", required=True)
    f.add_argument("--branch", nargs="+", required=True)
    f.add_argument("--out", default=None)
    args = ap.parse_args()
    return measure(args) if args.cmd == "measure" else fold(args)


if __name__ == "__main__":
    sys.exit(main())
