"""The yardstick of double Q-learning and of per-env learner hyper-parameters (RLToyVectorEnv.set_learner / set_learner_rates /
rollout_learn): a numpy restatement of the semantics in include/mdpp.h and DESIGN.md 3.12, vectorised over envs, float32
throughout, its Philox words from the oracle.  It imports nothing from the product.

Env i of a handle (global id g = off + i) at step counter t in state s, with ITS alpha[i], gamma[i] (float32) and
E[i] = ceil(float64(float32(epsilon[i])) 2^31) -- the arrays go by the local index i, only the words by g:
  sel(s, t):  wE = philox_tick_word(seed, g, t, 15); (wE >> 1) < E[i]: explore, a = (uint64(wA) A) >> 32 with wA the word of
              stream 16; otherwise the lowest j maximising Q[s][j] -- double_q: maximising float32(QA[s][j] + QB[s][j])
  q_learning / sarsa: target, update and sarsa's carry as tests/learner_ref.py states them
  double_q:   wU = philox_tick_word(seed, g, t, 17); wU >> 31 == 0: X = QA, Y = QB, otherwise X = QB, Y = QA;
              terminated: y = r; otherwise a* = the lowest argmax_j X[s'][j], y = r + gamma Y[s'][a*];
              q = X[s][a], d = y - q, u = alpha d, X[s][a] = q + u;  no carry
  next-step autoreset: on an env's reset call an action is selected from the recorded state and ignored; no update.
Tables: Q float32 [N, S, A]; double_q [N, 2, S, A], A first.

select() and update() are one step for all envs (a CPU closed loop drives an env between them); run() is a launch of K steps
fed with the launch's own outputs, like learner_ref.run.  s' is obs[k] except where a same-step autoreset replaced it; there
it matters only when truncated and not terminated, and is P[s][a] (noise-free cases).
"""
import numpy as np

EXPLORE_STREAM, ACTION_STREAM, UPDATE_STREAM = 15, 16, 17
ALGOS = ("q_learning", "sarsa", "double_q")
DISABLED, SAME_STEP, NEXT_STEP = "disabled", "same_step", "next_step"

_cache = {}


def tick_words(seed, off, tick0, rows, n, stream):
    """uint32 [rows, n]: the word env off + i draws at tick tick0 + k from `stream` of the learner's seed"""
    from oracle import oracle as ora
    key = (seed, off, tick0, rows, n, stream)
    if key not in _cache:
        _cache[key] = np.array([[ora.philox_tick_word(seed, off + i, tick0 + k, stream) for i in range(n)]
                                for k in range(rows)], dtype=np.uint32)
    return _cache[key]


def epsilon_threshold(eps):
    """element-wise, int64"""
    return np.ceil(np.asarray(eps, np.float32).astype(np.float64) * 2147483648.0).astype(np.int64)


def per_env(n, alpha, gamma, epsilon):
    """(alpha float32 [n], gamma float32 [n], E int64 [n]) from scalars or arrays of n"""
    al = np.broadcast_to(np.asarray(alpha, np.float32), (n,)).copy()
    ga = np.broadcast_to(np.asarray(gamma, np.float32), (n,)).copy()
    E = np.broadcast_to(epsilon_threshold(epsilon), (n,)).copy()
    return al, ga, E


def new_info(n):
    return dict(explored=0, explored_env=np.zeros(n, np.int64), selections_env=np.zeros(n, np.int64), greedy_ties=0, greedy_strict=0,
                carried=0, carried_differs=0, updates=0, updates_a=0, updates_b=0, cross_differs=0, sum_differs=0,
                trunc_resets=0, trunc_carry_differs=0, zero_sign_ties=0, denormal_results=0, nans_made=0)


def merge_info(total, info):
    for k, v in info.items():
        total[k] = v.copy() if k not in total and isinstance(v, np.ndarray) else total.get(k, 0) + v
    return total


def scan_best(row):
    """(arg int64 [n], best [n]) of row [n, A]: best = row[0]; for j = 1 ... A - 1: row[j] > best moves on.  Not np.argmax, which
    ranks a NaN first wherever it stands."""
    row = np.asarray(row)
    best, arg = row[:, 0].copy(), np.zeros(row.shape[0], np.int64)
    with np.errstate(invalid="ignore"):
        for j in range(1, row.shape[1]):
            m = row[:, j] > best
            best, arg = np.where(m, row[:, j], best), np.where(m, j, arg)
    return arg, best


def _greedy_row(algo, Q, s):
    idx = np.arange(Q.shape[0])
    if algo == "double_q":
        with np.errstate(invalid="ignore", over="ignore"):
            row = Q[idx, 0, s] + Q[idx, 1, s]
        assert row.dtype == np.float32
        return row
    return Q[idx, s]


def select(algo, Q, s, w_e, w_a, E, info=None, fresh_mask=None):
    """sel for every env: (actions, explored).  info (new_info): counts the selections of the envs in fresh_mask (all)"""
    n, A = Q.shape[0], Q.shape[-1]
    explored = (w_e >> np.uint32(1)).astype(np.int64) < E
    a_x = ((w_a.astype(np.uint64) * np.uint64(A)) >> np.uint64(32)).astype(np.int64)
    row = _greedy_row(algo, Q, s)
    a_g, best = scan_best(row)
    if info is not None:
        m = np.ones(n, bool) if fresh_mask is None else fresh_mask
        info["explored"] += int((explored & m).sum())
        info["explored_env"] += explored & m
        info["selections_env"] += m
        ties = (row == best[:, None]).sum(axis=1) > 1
        greedy = ~explored & m
        info["greedy_ties"] += int((greedy & ties).sum())
        info["greedy_strict"] += int((greedy & ~ties).sum())
        # a tie decided between -0.0 and +0.0: the maximum is zero and zeros of both signs attain it
        zeros = row == 0
        both = (zeros & np.signbit(row)).any(axis=1) & (zeros & ~np.signbit(row)).any(axis=1)
        info["zero_sign_ties"] += int((greedy & (best == 0) & both).sum())
        if algo == "double_q":
            info["sum_differs"] += int((greedy & (a_g != scan_best(Q[np.arange(n), 0, s])[0])).sum())
    return np.where(explored, a_x, a_g), explored


def update(algo, Q, s, a, r, s2, terminated, live, alpha, gamma, w_u=None, a2=None, info=None):
    """One step's update of Q IN PLACE for the envs in `live`.  r float32 [n]; s2 the true next states; sarsa: a2 = sel(s2, t + 1)
    on Q before this update; double_q: w_u the tick's words of stream 17."""
    n = Q.shape[0]
    idx = np.arange(n)
    r = np.asarray(r, np.float32)
    te = np.asarray(terminated, bool)
    if algo == "double_q":
        b = (w_u >> np.uint32(31)).astype(np.int64)          # 0: A learns, 1: B
        a_star = scan_best(Q[idx, b, s2])[0]
        qn = Q[idx, 1 - b, s2, a_star]
        if info is not None:
            info["cross_differs"] += int((live & ~te & (qn != scan_best(Q[idx, 1 - b, s2])[1])).sum())
            info["updates_a"] += int((live & (b == 0)).sum())
            info["updates_b"] += int((live & (b == 1)).sum())
    elif algo == "sarsa":
        qn = Q[idx, s2, a2]
    else:
        qn = scan_best(Q[idx, s2])[1]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):     # (the tables may hold infinities and denormals)
        g = gamma * qn
        y = np.where(te, r, r + g).astype(np.float32)
        q = Q[idx, b, s, a] if algo == "double_q" else Q[idx, s, a]
        d = y - q
        u = alpha * d
        new = (q + u)[live]
    assert g.dtype == d.dtype == u.dtype == new.dtype == np.float32
    if algo == "double_q":
        Q[idx[live], b[live], s[live], a[live]] = new
    else:
        Q[idx[live], s[live], a[live]] = new
    if info is not None:
        info["updates"] += int(live.sum())
        info["denormal_results"] += int(((new != 0) & (np.abs(new) < np.finfo(np.float32).tiny)).sum())
        info["nans_made"] += int((np.isnan(new) & ~np.isnan(q[live])).sum())


def run(algo, alpha, gamma, epsilon, Q, obs_before, obs, reward, terminated, truncated, P, autoreset, w_e, w_a, w_u=None, pending=None):
    """One launch of K steps.  alpha, gamma, epsilon: scalars or arrays [N].  Q (not modified); obs_before [N]; obs, reward,
    terminated, truncated [K, N]; P [S, A]; w_e, w_a uint32 [K + 1, N] (row k: tick0 + k; the last row serves sarsa's
    sel(s', t + 1) of the last step); w_u uint32 [>= K, N] (double_q); pending bool [N]: the env's next call is its reset.
    Returns (actions int64 [K, N], Q, pending, info)."""
    assert algo in ALGOS and Q.dtype == np.float32 and Q.ndim == (4 if algo == "double_q" else 3)
    sarsa = algo == "sarsa"
    Q = Q.copy()
    K, n = obs.shape
    al, ga, E = per_env(n, alpha, gamma, epsilon)
    s = np.asarray(obs_before).astype(np.int64)
    pending = np.zeros(n, bool) if pending is None else np.asarray(pending, bool).copy()
    have_carry, carry = np.zeros(n, bool), np.zeros(n, np.int64)
    actions = np.zeros((K, n), np.int64)
    info = new_info(n)
    dropped = np.zeros(n, bool)                           # sarsa: the previous step dropped its carry at a truncation with a reset
    for k in range(K):
        fresh, _ = select(algo, Q, s, w_e[k], w_a[k], E, info, ~have_carry)
        info["trunc_carry_differs"] += int((dropped & (carry != fresh)).sum())
        a = np.where(have_carry, carry, fresh)
        actions[k] = a
        info["carried"] += int(have_carry.sum())
        info["carried_differs"] += int((have_carry & (carry != fresh)).sum())
        live = ~pending                                   # (a reset call: nothing is learnt)
        te, tr = np.asarray(terminated[k], bool), np.asarray(truncated[k], bool)
        s2 = np.asarray(obs[k]).astype(np.int64)
        if autoreset == SAME_STEP:
            s2 = np.where(te | tr, P[s, a], s2)
        a2 = select(algo, Q, s2, w_e[k + 1], w_a[k + 1], E)[0] if sarsa else np.zeros(n, np.int64)
        update(algo, Q, s, a, reward[k], s2, te, live, al, ga, None if w_u is None else w_u[k], a2, info)
        have_carry = live & sarsa & ~te & ~(tr & (autoreset != DISABLED))
        cut = live & ~te & tr & (autoreset != DISABLED)
        info["trunc_resets"] += int(cut.sum())
        dropped = cut & sarsa
        carry = a2
        pending = live & (autoreset == NEXT_STEP) & (te | tr)
        s = np.asarray(obs[k]).astype(np.int64)
    return actions, Q, pending, info
