"""The yardstick of the episode log (log= on rollout_learn / rollout_eval with summary=; include/mdpp.h "Episode summaries",
DESIGN.md 3.24): the rule restated in numpy, step by step, vectorised over envs.  It imports nothing from the product.

A log of capacity M >= 1:  count int32 [N], ret float64 [M, N], len int32 [M, N] (episode-major).  Per env, in step order, for
every step that is not the reset call of a next-step-autoreset env (tests/eval_summary_ref.py: reset_calls):
    run_ret += float64(reward);  run_len += 1
    terminated or truncated:
        if count < M:  ret[count, i] = run_ret;  len[count, i] = run_len
        count += 1
        episodes += 1;  return_sum += run_ret;  length_sum += run_len;  run_ret = run_len = 0
The five summary arrays are restated here too (not taken from eval_summary_ref.summary, which the host test holds them to).
"""
import numpy as np

FIELDS5 = (("ret", np.float64), ("len", np.int32), ("episodes", np.int32), ("return_sum", np.float64), ("length_sum", np.int32))
WAVE = 64


def new_state5(n):
    return {name: np.zeros(n, dt) for name, dt in FIELDS5}


def new_log(n, M, fill_ret=0.0, fill_len=0):
    """a log state; fill_*: what the unwritten entries hold (a sentinel shows that a launch leaves them alone)"""
    assert M >= 1
    return dict(count=np.zeros(n, np.int32), ret=np.full((M, n), fill_ret, np.float64), len=np.full((M, n), fill_len, np.int32))


def new_counters():
    return dict(over_M=0, under_M=0, zero=0, spanning_logged=0, wave_rows_differ=0, ended_terminated=0, ended_truncated=0, reset_calls=0)


def run(reward, term, trunc, reset_call, state5, log, counters=None):
    """One launch.  reward float32 [K, N]; term, trunc, reset_call bool [K, N]; state5 (new_state5) and log (new_log) are not
    modified.  Returns (log, state5) after the launch.  counters (new_counters), added to:
      spanning_logged    logged episodes that began in an earlier launch (the running length was > 0 when this one began)
      wave_rows_differ   steps at which lanes of one 64-env wave wrote different rows m
      ended_terminated / ended_truncated / reset_calls   episode ends by flag (truncated: not also terminated), skipped reset calls
    and SET from the log's final count (call end_counters after the last launch for the totals of a pass):
      over_M / under_M / zero    envs that end with count > M / count < M / count == 0"""
    reward = np.asarray(reward)
    assert reward.dtype == np.float32
    st = {k: v.copy() for k, v in state5.items()}
    lg = {k: v.copy() for k, v in log.items()}
    assert all(st[name].dtype == dt for name, dt in FIELDS5)
    assert lg["count"].dtype == np.int32 and lg["ret"].dtype == np.float64 and lg["len"].dtype == np.int32
    K, n = reward.shape
    M = lg["ret"].shape[0]
    assert lg["ret"].shape == lg["len"].shape == (M, n) and lg["count"].shape == (n,)
    carried_in = st["len"] > 0
    first = np.ones(n, bool)                       # the env has not finished an episode in this launch yet
    for k in range(K):
        for i in range(n):
            if reset_call[k][i]:
                if counters is not None:
                    counters["reset_calls"] += 1
                continue
            st["ret"][i] = st["ret"][i] + np.float64(reward[k][i])
            st["len"][i] += np.int32(1)
        rows = np.full(n, -1, np.int64)            # the row each env wrote at this step
        for i in range(n):
            if reset_call[k][i] or not (term[k][i] or trunc[k][i]):
                continue
            c = int(lg["count"][i])
            if c < M:
                lg["ret"][c, i] = st["ret"][i]
                lg["len"][c, i] = st["len"][i]
                rows[i] = c
                if counters is not None and first[i] and carried_in[i]:
                    counters["spanning_logged"] += 1
            lg["count"][i] += np.int32(1)
            st["episodes"][i] += np.int32(1)
            st["return_sum"][i] = st["return_sum"][i] + st["ret"][i]
            st["length_sum"][i] += st["len"][i]
            st["ret"][i] = 0.0
            st["len"][i] = 0
            first[i] = False
            if counters is not None:
                counters["ended_terminated" if term[k][i] else "ended_truncated"] += 1
        if counters is not None:
            for lo in range(0, n, WAVE):
                w = rows[lo:lo + WAVE]
                if len(set(w[w >= 0].tolist())) > 1:
                    counters["wave_rows_differ"] += 1
    if counters is not None:
        end_counters(lg, counters)
    return lg, st


def end_counters(log, counters):
    M = log["ret"].shape[0]
    counters["over_M"] = int((log["count"] > M).sum())
    counters["under_M"] = int((log["count"] < M).sum())
    counters["zero"] = int((log["count"] == 0).sum())
    return counters


def left_to_right_sum(log, i):
    """the float64 sum of env i's logged returns, added in order from 0.0"""
    s = np.float64(0.0)
    for m in range(min(int(log["count"][i]), log["ret"].shape[0])):
        s = s + log["ret"][m, i]
    return s


def pop5(state5):
    """EpisodeSummary.pop(): the three sums zeroed; the log is not touched"""
    return {k: (np.zeros_like(v) if k in ("episodes", "return_sum", "length_sum") else v.copy()) for k, v in state5.items()}
