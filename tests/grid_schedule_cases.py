"""The cases of the grid learners' schedule and episode-log tests: the six configs of tests/grid_learner_cases.py (imported, not
edited), each with a schedule of its own; N = 320, K = 37, two launches, as there.  tests/test_grid_schedule_host.py runs each
on the CPU (tests/grid_schedule_ref.py) and asserts the conditions that keep a GPU pass honest; tests/test_gpu_grid_schedule.py
runs each on the GPU against that restatement.

  g34_dense              epsilon only, R = 1, M = 3, row=None
  g55_sparse_limit_i32   epsilon and alpha, R = 3, M = 5, row[i] = i % 3 (QLDS = 1 under SCHED)
  g55_noop_next_every3   alpha only, R = 2, M = 4 (reset calls, QLDS = 0)
  g17_noise              epsilon and alpha, R = 1, M = 1: equals, bit for bit, an unscheduled handle with those two values
  g88_disabled_pnoise    epsilon only, R = 2, M = 6 (autoreset disabled: the counter runs at every step once the limit is reached)
  g34_noise_next_i32     epsilon and alpha, R = 3, M = 7

Rows are distinct and decreasing -- policy.epsilon_decay "linear" and "log" and a hand-written one -- so that a wrong row or a
wrong entry changes selections.  Every log has capacity 3."""
import numpy as np

import grid_learner_cases as gc

N, K, LAUNCHES = gc.N, gc.K, gc.LAUNCHES
LOG_M = 3
CASES = gc.CASES


def _rows(*rows):
    return np.array(rows, np.float64).astype(np.float32)


def _tables():
    from mdp_playground_amd import policy
    d = policy.epsilon_decay
    return {
        "g34_dense": dict(epsilon=_rows(d("linear", 0.9, 3, 0.1))[0], alpha=None, R=1),
        "g55_sparse_limit_i32": dict(epsilon=_rows(d("linear", 1.0, 5, 0.05), d("log", 0.8, 5, 0.05), [0.6, 0.45, 0.3, 0.2, 0.1]),
                                     alpha=_rows(d("linear", 1.0, 5, 0.25), d("log", 0.75, 5, 0.125), [0.5, 0.4, 0.3, 0.2, 0.1]), R=3),
        "g55_noop_next_every3": dict(epsilon=None, alpha=_rows(d("linear", 1.0, 4, 0.2), [0.9, 0.6, 0.4, 0.25]), R=2),
        "g17_noise": dict(epsilon=_rows([0.45]), alpha=_rows([0.375]), R=1),
        "g88_disabled_pnoise": dict(epsilon=_rows(d("linear", 1.0, 6, 0.1), d("log", 0.9, 6, 0.05)), alpha=None, R=2),
        "g34_noise_next_i32": dict(epsilon=_rows(d("linear", 1.0, 7, 0.05), d("log", 0.7, 7, 0.02), [0.8, 0.65, 0.5, 0.35, 0.25, 0.15, 0.1]),
                                   alpha=_rows(d("log", 1.0, 7, 0.1), d("linear", 0.8, 7, 0.2), [0.6, 0.5, 0.45, 0.4, 0.3, 0.25, 0.125]), R=3),
    }


def schedule(case, n=N):
    """dict(epsilon=, alpha=, row=): what the case hands set_grid_learner_schedule on a handle of n envs"""
    t = _tables()[case]
    return dict(epsilon=t["epsilon"], alpha=t["alpha"], row=None if t["R"] == 1 else (np.arange(n) % t["R"]).astype(np.int32))


def shape(case):
    """(R, M, epsilon scheduled, alpha scheduled)"""
    t = _tables()[case]
    tab = np.atleast_2d(t["epsilon"] if t["epsilon"] is not None else t["alpha"])
    return tab.shape[0], tab.shape[1], t["epsilon"] is not None, t["alpha"] is not None


def ref_schedule(case, n=N):
    import learner_schedule_ref as sref
    return sref.Schedule(n, **schedule(case, n))


_cpu_runs = {}


def cpu_run(case, algo, streams=None, sched="case"):
    """(info, Q, ep, traj) of the case's two scheduled learning launches on the CPU (tests/grid_schedule_ref.closed_loop), computed
    once per (case, algo) on the Philox streams of the cases' key; with ``streams`` (a handle's seeded numpy words) computed
    afresh.  sched=None: the same launches without a schedule."""
    import grid_schedule_ref as gsr
    c = CASES[case]
    al, ga, ep = c["rates"]

    def run():
        return gsr.closed_loop(c["cfg"], c["kw"], algo, al, ga, ep, N, gc.initial_tables(case), ref_schedule(case) if sched == "case" else None,
                               seed=gc.LEARNER_SEED, K=K, launches=LAUNCHES, noop=c["noop"], philox_seed=gc.PHILOX_SEED,
                               off=gc.ENV_ID_OFFSET, streams=streams)
    if streams is not None:
        return run()
    if (case, algo, sched) not in _cpu_runs:
        _cpu_runs[case, algo, sched] = run()
    return _cpu_runs[case, algo, sched]


def expected_name(case, rng, summary=False, qlds=None, sched=True):
    name = gc.expected_name(case, rng, summary=summary, qlds=qlds)
    return name[:-1] + ",SCHED=1>" if sched else name
