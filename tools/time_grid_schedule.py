"""Grid learner schedules and the episode log: what the SCHED and LOG forms of the one-launch learner cost, and what the
scheduled launch replaces.

    python tools/time_grid_schedule.py [--envs 65536] [--steps 512] [--repeats 5] [--out profiles/grid_schedule.json]

Grids: 5 x 5 (the tables staged in LDS, QLDS=1), 8 x 8 and 16 x 16 (QLDS=0), each quiet and with both noise keys; numpy
streams, dense reward, same-step autoreset, max_episode_steps 64, Q-learning.  Two schedules, both epsilon only, two rows of 40
entries, row[i] = i % 2: the CONSTANT one holds the handle's own epsilon in every entry, so the scheduled launch selects exactly
as the unscheduled launch does -- the same epsilon, the same number of episode ends (recorded), the same work -- and the
difference is the SCHED form's own cost; the DECAYING one (policy.epsilon_decay "linear" and "log", 1 -> 0.05) is what a user sets, and walks other trajectories
(epsilon near 1 at first: more exploring draws, longer episodes).  The log has capacity 32.  Every figure is the
median of --repeats timings after a warm-up of the timed form, taken with the library's HIP events on the caller's stream.
Before every timed run (outside the timing) the env is reset and the learner set anew, so every run is the first K steps of
learning from zero tables, zero counters and an empty log: the runs compared do the same kind of work whatever ran before
them.  All runs are in the record.
  (1) const_sched_us against plain_us   rollout_grid_learn(K, out=) with the constant schedule and without one, the same handle, the
                                        same epsilon (const_sched_summary_us against summary_us, const_sched_log_us against
                                        log_us likewise); sched_us, sched_summary_us, sched_log_us: the decaying schedule
  (2) sched_summary_us against loop_us  the scheduled summary launch against the loop it replaces: K x { counter and table lookup
                                        in torch; set_grid_learner_rates(epsilon=);  rollout_grid_learn(1, summary=) }
  (3) log_us against summary_us and plain_us   rollout_grid_learn(K, summary=, log=) against the summary launch and against the
                                        full-output launch, all three without a schedule; sched_log_us: with it
Acceptance (DESIGN.md 3.25's rule) for (2): on every row the SLOWEST scheduled launch (full output, summary or log form) beats
the FASTEST run of the loop; the tool exits with status 1 otherwise.  (1) and (3) are recorded, not gated.
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

BASE = dict(state_space_type="grid", reward_function="move_to_a_point", make_denser=True, seed=0)
NOISE = dict(transition_noise=0.1, reward_noise=0.25)
SIDES = {"5x5": 5, "8x8": 8, "16x16": 16}
ALPHA, GAMMA, EPS = 0.3, 0.9, 0.1
SCHED_M, LOG_M = 40, 32


def timed_us(env, fn, repeats, before=lambda: None):
    before()
    fn()                                    # warm-up: code objects, allocator, the LDS attribute
    torch.cuda.synchronize(env.device)
    out = []
    for _ in range(repeats):
        before()
        torch.cuda.synchronize(env.device)
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
    table = np.stack([policy.epsilon_decay("linear", 1.0, SCHED_M, 0.05), policy.epsilon_decay("log", 1.0, SCHED_M, 0.05)]).astype(np.float32)
    row = (np.arange(N) % 2).astype(np.int32)
    table_dev, row_dev = torch.as_tensor(table, device=dev), torch.as_tensor(row, device=dev).long()
    rows, ok = [], True
    for shape, side in SIDES.items():
        for noisy in (False, True):
            cfg = dict(BASE, grid_shape=(side, side), target_point=[side // 2, side // 2], **(NOISE if noisy else {}))
            env = RLToyVectorEnv(num_envs=N, device=dev, max_episode_steps=64, **cfg)
            out = env.alloc_rollout_grid(K)
            summ, log = env.episode_summary(), env.episode_log(LOG_M)

            def fresh(sched=None):
                # every timed run is the FIRST K steps of learning: new episodes, zero tables, zero counters, an empty log
                env.reset()
                env.set_grid_learner("q_learning", alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=1)
                if sched is not None:
                    env.set_grid_learner_schedule(epsilon=sched, row=row)
                summ.clear(); log.clear()

            def three(sched):
                """the full-output, summary and log launches under sched, and the episodes the last of them ended"""
                fo = timed_us(env, lambda: env.rollout_grid_learn(K, out=out), args.repeats, lambda: fresh(sched))
                name = env.grid_learn_kernel_name(K)
                sm_ = timed_us(env, lambda: env.rollout_grid_learn(K, summary=summ), args.repeats, lambda: fresh(sched))
                lg_ = timed_us(env, lambda: env.rollout_grid_learn(K, summary=summ, log=log), args.repeats, lambda: fresh(sched))
                return fo, sm_, lg_, name, int(log.count.sum()), int(log.filled().sum())

            (plain, plain_all), (sm, sm_all), (lg, lg_all), plain_kernel, ended_plain, entries_written = three(None)
            # the constant schedule: the unscheduled launch's epsilon, hence its workload, through the SCHED kernels
            (csched, csched_all), (cssm, cssm_all), (cslg, cslg_all), _, ended_const, _ = three(np.full_like(table, EPS))
            (sched, sched_all), (ssm, ssm_all), (slg, slg_all), sched_kernel, episodes, _ = three(table)
            fresh()

            def loop():         # (2) the loop a user writes without the schedule: one one-step launch per step
                for _ in range(K):
                    e = torch.clamp(summ.episodes.long(), max=SCHED_M - 1)
                    env.set_grid_learner_rates(epsilon=table_dev[row_dev, e].cpu().numpy())
                    env.rollout_grid_learn(1, summary=summ)
            loop_us, loop_all = timed_us(env, loop, args.repeats, fresh)
            assert not env.status().any()
            env.close()

            slowest_fused = max(sched_all + ssm_all + slg_all)
            accepted = slowest_fused < min(loop_all)
            r = dict(shape=shape, noise=noisy, num_envs=N, steps=K, plain_us=round(plain, 1), sched_us=round(sched, 1), summary_us=round(sm, 1),
                     log_us=round(lg, 1), sched_summary_us=round(ssm, 1), sched_log_us=round(slg, 1), loop_us=round(loop_us, 1),
                     const_sched_us=round(csched, 1), const_sched_summary_us=round(cssm, 1), const_sched_log_us=round(cslg, 1),
                     const_sched_over_plain=round(csched / plain, 3), const_sched_summary_over_summary=round(cssm / sm, 3),
                     const_sched_log_over_log=round(cslg / lg, 3),
                     sched_over_plain=round(sched / plain, 3), sched_summary_over_summary=round(ssm / sm, 3),
                     log_over_summary=round(lg / sm, 3), log_over_plain=round(lg / plain, 3), sched_log_over_sched_summary=round(slg / ssm, 3),
                     speedup_vs_loop=round(loop_us / ssm, 1), slowest_sched_us=slowest_fused, fastest_loop_us=min(loop_all), accepted=accepted,
                     log_exceeds_full_output=lg > plain, episodes_per_launch=episodes, episodes_per_launch_unscheduled=ended_plain, episodes_per_launch_const_sched=ended_const,
                     log_entries_written=entries_written,
                     plain_kernel=plain_kernel, sched_kernel=sched_kernel, plain_all_us=plain_all, sched_all_us=sched_all, summary_all_us=sm_all,
                     const_sched_all_us=csched_all, const_sched_summary_all_us=cssm_all, const_sched_log_all_us=cslg_all,
                     log_all_us=lg_all, sched_summary_all_us=ssm_all, sched_log_all_us=slg_all, loop_all_us=loop_all)
            ok = ok and accepted
            print(json.dumps(r), flush=True)
            rows.append(r)
    print(json.dumps(dict(accepted=ok)), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(dev), alpha=ALPHA, gamma=GAMMA, epsilon=EPS, schedule_entries=SCHED_M,
                           log_capacity=LOG_M, accepted=ok, rows=rows), f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
