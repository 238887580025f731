"""The yardstick of greedy evaluation and of the in-kernel episode summaries (RLToyVectorEnv.rollout_eval, and summary= on
rollout_learn / rollout_eval): a numpy restatement of the semantics in include/mdpp.h and DESIGN.md 3.13, vectorised over
envs.  It imports nothing from the product.  Greedy evaluation draws no Philox word, so unlike tests/learner_sweep_ref.py
this file needs none from the oracle; the learning launches it summarises are restated there.

Greedy evaluation, env i in state s:
  one table:  a = the lowest j maximising Q[i][s][j] (float32, scanned from j = 0 with a strict >)
  double_q:   a = the lowest j maximising float32(QA[i][s][j] + QB[i][s][j])
  next-step autoreset: on an env's reset call the action is selected from the recorded state and ignored.
Tables: Q float32 [N, S, A]; double_q [N, 2, S, A], A first.

Episode summaries, per env, in step order, for every step that is not a reset call:
  ret += float64(reward);  len += 1;  terminated or truncated: episodes += 1, return_sum += ret, length_sum += len, ret = len = 0
with ret, return_sum float64 and len, episodes, length_sum int32.
"""
import numpy as np

from learner_sweep_ref import scan_best

DISABLED, SAME_STEP, NEXT_STEP = "disabled", "same_step", "next_step"
FIELDS = (("ret", np.float64), ("len", np.int32), ("episodes", np.int32), ("return_sum", np.float64), ("length_sum", np.int32))


def new_info():
    return dict(greedy_strict=0, greedy_ties=0, sum_differs=0, terminations=0, reset_calls=0)


def merge_info(total, info):
    for k, v in info.items():
        total[k] = total.get(k, 0) + v
    return total


def greedy(Q, s, info=None, live=None):
    """The greedy action of every env: Q float32 [n, S, A] or [n, 2, S, A], s int [n] -> int64 [n].  info (new_info) counts
    the selections of the envs in `live` (all): a strict maximum / a tie resolved to the lowest index / double Q: the summed
    tables' choice differs from QA's alone."""
    assert Q.dtype == np.float32 and Q.ndim in (3, 4)
    n = Q.shape[0]
    idx = np.arange(n)
    s = np.asarray(s).astype(np.int64)
    if Q.ndim == 4:
        with np.errstate(invalid="ignore", over="ignore"):
            row = Q[idx, 0, s] + Q[idx, 1, s]                # one float32 addition per entry
        assert row.dtype == np.float32
    else:
        row = Q[idx, s]
    a, best = scan_best(row)                                 # (the kernel's scan: not np.argmax, which ranks a NaN first)
    if info is not None:
        m = np.ones(n, bool) if live is None else live
        ties = (row == best[:, None]).sum(axis=1) > 1
        info["greedy_ties"] += int((m & ties).sum())
        info["greedy_strict"] += int((m & ~ties).sum())
        if Q.ndim == 4:
            info["sum_differs"] += int((m & (a != scan_best(Q[idx, 0, s])[0])).sum())
    return a.astype(np.int64)


def eval_run(Q, obs_before, obs, terminated, truncated, autoreset, pending=None):
    """One evaluation launch of K steps fed with the launch's own outputs.  Q (never modified); obs_before [N]; obs,
    terminated, truncated [K, N]; pending bool [N]: the env's next call is its reset.  Returns (actions int64 [K, N],
    reset_call bool [K, N], pending, info)."""
    K, n = obs.shape
    s = np.asarray(obs_before).astype(np.int64)
    pending = np.zeros(n, bool) if pending is None else np.asarray(pending, bool).copy()
    actions, reset_call = np.zeros((K, n), np.int64), np.zeros((K, n), bool)
    info = new_info()
    for k in range(K):
        live = ~pending
        reset_call[k] = pending
        actions[k] = greedy(Q, s, info, live)
        te, tr = np.asarray(terminated[k], bool), np.asarray(truncated[k], bool)
        info["terminations"] += int((live & te).sum())
        info["reset_calls"] += int(pending.sum())
        pending = live & (autoreset == NEXT_STEP) & (te | tr)
        s = np.asarray(obs[k]).astype(np.int64)
    return actions, reset_call, pending, info


def reset_calls(terminated, truncated, autoreset, pending=None):
    """bool [K, N]: which steps of a launch were an env's reset call, and the pending flags after it"""
    K, n = terminated.shape
    pending = np.zeros(n, bool) if pending is None else np.asarray(pending, bool).copy()
    out = np.zeros((K, n), bool)
    for k in range(K):
        out[k] = pending
        pending = ~pending & (autoreset == NEXT_STEP) & (np.asarray(terminated[k], bool) | np.asarray(truncated[k], bool))
    return out, pending


def new_state5(n):
    return {name: np.zeros(n, dt) for name, dt in FIELDS}


def new_counters():
    return dict(two_in_one_launch=0, spans_boundary=0, ended_terminated=0, ended_truncated=0, reset_calls=0)


def summary(reward, term, trunc, reset_call, state5, counters=None):
    """The rule, step by step.  reward float32 [K, N]; term, trunc, reset_call bool [K, N]; state5 (new_state5; not
    modified).  Returns the five arrays after the launch.  counters (new_counters): envs that finished two or more episodes
    in this launch; envs whose first episode finished here had begun before it (ret / len carried in); episode ends by
    flag; reset calls."""
    reward = np.asarray(reward)
    assert reward.dtype == np.float32
    st = {k: v.copy() for k, v in state5.items()}
    assert all(st[name].dtype == dt for name, dt in FIELDS)
    K, n = reward.shape
    carried_in = st["len"] > 0
    finished_here = np.zeros(n, np.int64)
    spans = np.zeros(n, bool)
    for k in range(K):
        live = ~np.asarray(reset_call[k], bool)
        st["ret"] = np.where(live, st["ret"] + reward[k].astype(np.float64), st["ret"])
        st["len"] = np.where(live, st["len"] + np.int32(1), st["len"]).astype(np.int32)
        te, tr = np.asarray(term[k], bool), np.asarray(trunc[k], bool)
        end = live & (te | tr)
        spans |= end & carried_in & (finished_here == 0)
        finished_here += end
        st["episodes"] = (st["episodes"] + end).astype(np.int32)
        st["return_sum"] = np.where(end, st["return_sum"] + st["ret"], st["return_sum"])
        st["length_sum"] = np.where(end, st["length_sum"] + st["len"], st["length_sum"]).astype(np.int32)
        st["ret"] = np.where(end, 0.0, st["ret"])
        st["len"] = np.where(end, np.int32(0), st["len"]).astype(np.int32)
        if counters is not None:
            counters["ended_terminated"] += int((live & te).sum())
            counters["ended_truncated"] += int((live & tr & ~te).sum())
            counters["reset_calls"] += int((~live).sum())
    if counters is not None:
        counters["two_in_one_launch"] += int((finished_here >= 2).sum())
        counters["spans_boundary"] += int(spans.sum())
    assert all(st[name].dtype == dt for name, dt in FIELDS)
    return st


def pop(state5):
    """(episodes, return_sum, length_sum) as copies and the state with those three zeroed"""
    out = tuple(state5[k].copy() for k in ("episodes", "return_sum", "length_sum"))
    st = {k: (np.zeros_like(v) if k in ("episodes", "return_sum", "length_sum") else v.copy()) for k, v in state5.items()}
    return out, st
