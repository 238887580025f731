"""Eligibility traces of the in-kernel learners: the trace launch (set_learner_traces + rollout_learn) against the host loop it
replaces -- one step() per step, with selection, cut, mark, sweep and episode zeroing as torch kernels on [N, S, A] tensors --
and against the same handle's traceless launch.

    python tools/time_learn_traces.py [--envs 65536] [--steps 512] [--repeats 5] [--out profiles/learn_traces.json]

Shapes: S = A = 8, sequence_length 1, without delay and with delay = 4; numpy streams; Q-learning, Watkins's Q(lambda) with
replacing traces.  Each figure is the median of --repeats timings after a warm-up of every timed form, taken with the
library's HIP events on the caller's stream; every run is kept:
  learn_us           one rollout_learn(K) launch of the traceless learner (k_discrete_learn_rollout)
  trace_us           the same handle with traces (k_discrete_trace_rollout, replacing)
  trace_acc_us       ... accumulating
  trace_pe_us        ... replacing, with one lambda per env (the PE form)
  trace_summary_us   ... replacing, keeping episode summaries (rollout_learn(K, summary=))
  step_loop_us       K x { epsilon-greedy action from Q;  step();  target;  Z[explored] = 0;  Z[s, a] = 1;  Q += u Z;  Z *= c;
                           Z[terminated | truncated] = 0 }
trace_over_learn = trace_us / learn_us is recorded, not gated: what the sweep costs.  Acceptance (DESIGN.md 3.25's): on every
shape the SLOWEST run of every fused trace form beats the FASTEST run of the step() loop; exit status 1 otherwise.
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

BASE = dict(state_space_type="discrete", action_space_type="discrete", seed=0, state_space_size=8, action_space_size=8, sequence_length=1)
CONFIGS = {"s8_delay0": dict(BASE, delay=0), "s8_delay4": dict(BASE, delay=4)}
ALPHA, GAMMA, EPS, LAMBDA = 0.3, 0.9, 0.1, 0.8


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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    N, K = args.envs, args.steps
    rows, ok = [], True
    for name, cfg in CONFIGS.items():
        env = RLToyVectorEnv(num_envs=N, device=dev, **cfg)
        S, A = env.mdps[0].S, env.mdps[0].A
        out = env.alloc_rollout_learn(K)
        learn = lambda: env.rollout_learn(K, out=out)                       # noqa: E731
        fig, runs, kernels = {}, {}, {}
        env.set_learner("q_learning", alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=1)
        fig["learn"], runs["learn"] = timed_us(env, learn, args.repeats)
        kernels["learn"] = env.learn_kernel_name(K)
        env.set_learner_traces(LAMBDA, "replacing")
        fig["trace"], runs["trace"] = timed_us(env, learn, args.repeats)
        kernels["trace"] = env.learn_kernel_name(K)
        env.set_learner_traces(LAMBDA, "accumulating")
        fig["trace_acc"], runs["trace_acc"] = timed_us(env, learn, args.repeats)
        env.set_learner_traces(np.linspace(0.0, 1.0, N).astype(np.float32), "replacing")
        fig["trace_pe"], runs["trace_pe"] = timed_us(env, learn, args.repeats)
        kernels["trace_pe"] = env.learn_kernel_name(K)
        env.set_learner_traces(LAMBDA, "replacing")
        summary = env.episode_summary()
        fig["trace_summary"], runs["trace_summary"] = timed_us(env, lambda: env.rollout_learn(K, summary=summary), args.repeats)
        env.set_learner(None)

        Q = torch.zeros((N, S, A), dtype=torch.float32, device=dev)
        Z = torch.zeros((N, S, A), dtype=torch.float32, device=dev)
        idx = torch.arange(N, device=dev)
        none = torch.zeros(N, dtype=torch.bool, device=dev)
        c = GAMMA * LAMBDA

        def step_loop():
            obs = env.reset(mask=none)[0].long()                    # (the observation every env shows; a summary launch wrote none)
            for _ in range(K):
                greedy = Q[idx, obs].argmax(dim=1)
                explore = torch.rand(N, device=dev) < EPS
                a = torch.where(explore, torch.randint(0, A, (N,), device=dev), greedy)
                nobs, r, term, trunc, _ = env.step(a.to(torch.int32))
                nobs = nobs.long()
                y = torch.where(term, r, r + GAMMA * Q[idx, nobs].max(dim=1).values)
                u = ALPHA * (y - Q[idx, obs, a])
                Z[explore] = 0.0                                    # cut
                Z[idx, obs, a] = 1.0                                # mark (replacing)
                Q.addcmul_(u[:, None, None], Z)                     # sweep
                Z.mul_(c)
                Z[term | trunc] = 0.0                               # episode end
                obs = nobs
        fig["step_loop"], runs["step_loop"] = timed_us(env, step_loop, args.repeats)
        assert not env.status().any()
        env.close()

        fused = ("trace", "trace_acc", "trace_pe", "trace_summary")
        slowest_fused = max(max(runs[f]) for f in fused)
        accepted = slowest_fused < min(runs["step_loop"])
        ok = ok and accepted
        r = dict(config=name, num_envs=N, steps=K, **{k + "_us": round(v, 1) for k, v in fig.items()},
                 trace_over_learn=round(fig["trace"] / fig["learn"], 3), trace_acc_over_trace=round(fig["trace_acc"] / fig["trace"], 3),
                 trace_pe_over_trace=round(fig["trace_pe"] / fig["trace"], 3), summary_over_full=round(fig["trace_summary"] / fig["trace"], 3),
                 speedup_vs_step_loop=round(fig["step_loop"] / fig["trace"], 2), env_steps_per_s=round(N * K / (fig["trace"] * 1e-6), 0),
                 slowest_fused_us=slowest_fused, fastest_step_loop_us=min(runs["step_loop"]), accepted=accepted, kernels=kernels,
                 **{k + "_all_us": v for k, v in runs.items()})
        print(json.dumps(r), flush=True)
        rows.append(r)
    result = dict(device=torch.cuda.get_device_name(dev), alpha=ALPHA, gamma=GAMMA, epsilon=EPS, lam=LAMBDA, repeats=args.repeats,
                  rule="the slowest run of every fused trace form beats the fastest run of the step() loop, on every shape",
                  rows=rows, accepted=ok)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
