"""Per-episode epsilon / alpha schedules on the noise-level and per-env-MDP learners (set_learner_schedule(..., sweep=True);
DESIGN.md 3.23): what the schedule costs on each of the three forms, and what the one launch replaces.

    python tools/time_learn_schedule_sweep.py [--envs 65536] [--steps 512] [--repeats 5] [--out profiles/learn_schedule_sweep.json]

The workload is the reference's tabular noise sweep as its experiment files run it (q_learn_tabular_p_noise.py,
q_learn_tabular_r_noise.py): one agent with a decay schedule on dummy_seed 0 ... 9 over five levels of one noise key, S = A = 8,
numpy streams, Q-learning.  Env i is on seed (i // 5) % 10 at level i % 5; the schedule is the 9-row table of
tools/time_learn_schedule.py (the *_tabular_tune_hps.py sweep: epsilon 0.1 / 0.01 / 0.001 x "linear" / "log" / "const", M = 1000,
row i % 9, alpha 0.1 / 0.3 / 0.5 per env).  Both sweeps are timed: `p_noise` (transition_noise 0 / 0.01 / 0.02 / 0.1 / 0.25) and
`r_noise` (reward_noise 0 / 1 / 5 / 10 / 25).  Each figure is the median of --repeats timings after a warm-up of every timed
form, taken with the library's HIP events on the caller's stream, all in one session:
  <form>_us, <form>_sched_us   one rollout_learn(K) launch of the form's handle without / with the schedule, for the forms
        nlev      a shared MDP (seed 0) with the five levels                      ...,NLEV=1[,SCHED=1]>
        pm        one MDP per env on the ten seeds, the key created uniformly     ...,PM=2[,SCHED=1]>
        pm_nlev   the ten seeds x the five levels: the whole sweep                ...,NLEV=1,PM=2[,SCHED=1]>
  sched_over_plain             ratio 1, the cost of the schedule: <form>_sched_us / <form>_us.  No bar; the shared form measured
                               0.98 - 1.09 (profiles/learn_schedule.json)
  fifty_handles_us             what the sweep needs without the feature: 50 shared-MDP SCHED handles, one per (seed, level), of
                               envs / 50 envs each, their launches issued back to back on one stream and timed as one
  speedup_vs_fifty_handles     ratio 2: fifty_handles_us / pm_nlev_sched_us.  The bar is the project's standing one for
                               closed-loop launches: the tool exits with status 1 unless it is at least --min-speedup (2)
The fifty handles run kernels this change leaves bit-identical (profiles/learn_schedule_sweep_resources.txt), so they are
the parent's figure measured in the same session.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mdp_playground_amd import RLToyVectorEnv  # noqa: E402
from time_learn_schedule import tune_hps_schedule, timed_us, GAMMA, EPS  # noqa: E402

TAB = dict(state_space_type="discrete", action_space_type="discrete", state_space_size=8, action_space_size=8, delay=0, sequence_length=1)
SEEDS = 10
SWEEPS = {
    "p_noise": ("transition_noise", (0.0, 0.01, 0.02, 0.10, 0.25)),
    "r_noise": ("reward_noise", (0.0, 1.0, 5.0, 10.0, 25.0)),
}
# what a handle that is given levels is created with: both keys present, transition_noise > 0 (the levels replace the values)
CREATED = dict(transition_noise=0.5, reward_noise=3.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-speedup", type=float, default=2.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    N, K = args.envs, args.steps
    i = np.arange(N)
    seeds = ((i // 5) % SEEDS).tolist()
    eps_tab, row, alpha = tune_hps_schedule(N)
    rows, ok = [], True
    for sweep, (key, values) in SWEEPS.items():
        level = np.asarray(values)[i % 5]
        other = "reward_noise" if key == "transition_noise" else "transition_noise"
        levels = {key: level, other: np.zeros(N)}
        # the pm form has no levels: the key is created uniformly at the sweep's middle value
        uniform = {key: values[3]}
        r = dict(sweep=sweep, key=key, levels=list(values), seeds=SEEDS, num_envs=N, steps=K, schedule_rows=9, schedule_entries=eps_tab.shape[1])
        for form in ("nlev", "pm", "pm_nlev"):
            per_env, lev = form != "nlev", form != "pm"
            cfg = dict(TAB, **(CREATED if lev else uniform))
            env = RLToyVectorEnv(seeds=seeds, device=dev, **cfg) if per_env else RLToyVectorEnv(num_envs=N, device=dev, seed=0, **cfg)
            env.set_learner("q_learning", alpha=alpha, gamma=GAMMA, epsilon=EPS, seed=1, **(dict(per_env_mdp=True) if per_env else {}))
            if lev:
                env.set_noise_levels(**levels, **(dict(per_env_mdp=True) if per_env else {}))
            out = env.alloc_rollout_learn(K)
            learn = lambda: env.rollout_learn(K, out=out)                   # noqa: E731
            plain, plain_all = timed_us(env, learn, args.repeats)
            plain_kernel = env.learn_kernel_name(K)
            env.set_learner_schedule(epsilon=eps_tab, row=row, sweep=True)
            sched, sched_all = timed_us(env, learn, args.repeats)
            episodes = env.learner_episodes()
            r.update({form + "_us": round(plain, 1), form + "_sched_us": round(sched, 1), form + "_sched_over_plain": round(sched / plain, 3),
                      form + "_kernel": plain_kernel, form + "_sched_kernel": env.learn_kernel_name(K),
                      form + "_all_us": plain_all, form + "_sched_all_us": sched_all,
                      form + "_episodes_min_median_max": [int(episodes.min()), int(episodes.median()), int(episodes.max())]})
            assert not env.status().any()
            env.close()
            del env, out
        # without the feature: one shared-MDP SCHED handle per (seed, level)
        n = N // (SEEDS * len(values))
        handles = []
        for s in range(SEEDS):
            for v in values:
                e = RLToyVectorEnv(num_envs=n, device=dev, seed=s, **dict(TAB, **{key: v}))
                e.set_learner("q_learning", alpha=alpha[:n], gamma=GAMMA, epsilon=EPS, seed=1)
                e.set_learner_schedule(epsilon=eps_tab, row=row[:n])
                handles.append((e, e.alloc_rollout_learn(K)))

        def fifty():
            for e, o in handles:
                e.rollout_learn(K, out=o)
        many, many_all = timed_us(handles[0][0], fifty, args.repeats)
        r.update(fifty_handles=len(handles), fifty_handles_envs_each=n, fifty_handles_us=round(many, 1), fifty_handles_all_us=many_all,
                 fifty_handles_kernel=handles[0][0].learn_kernel_name(K), speedup_vs_fifty_handles=round(many / r["pm_nlev_sched_us"], 2),
                 env_steps_per_s=round(N * K / (r["pm_nlev_sched_us"] * 1e-6), 0))
        for e, _ in handles:
            assert not e.status().any()
            e.close()
        ok = ok and many / r["pm_nlev_sched_us"] >= args.min_speedup
        print(json.dumps(r), flush=True)
        rows.append(r)
    result = dict(device=torch.cuda.get_device_name(dev), gamma=GAMMA, epsilon=EPS, min_speedup=args.min_speedup, rows=rows, accepted=ok)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
