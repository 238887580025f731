"""The yardstick of the in-kernel tabular learners (RLToyVectorEnv.set_learner / rollout_learn): a numpy restatement of the
learner's semantics (include/mdpp.h), vectorised over envs, float32 throughout, its Philox words from the
oracle.  It imports nothing from the product.

For env i (global id g = off + i) at step counter t in state s:
  sel(s, t):  wE = philox_tick_word(seed, g, t, 15); (wE >> 1) < E = ceil(float64(float32(epsilon)) 2^31): explore,
              a = (uint64(wA) A) >> 32 with wA = philox_tick_word(seed, g, t, 16); otherwise a = argmax_j Q[s][j] (the lowest)
  target:     terminated: y = r;  q_learning: y = r + gamma max_j Q[s'][j];  sarsa: y = r + gamma Q[s'][a'], a' = sel(s', t + 1) on Q
              before the update;  update: q = Q[s][a], d = y - q, u = alpha d, Q[s][a] = q + u
  sarsa:      the next step of the same launch takes a' when it starts from s' (no termination, no reset in between)
  next-step autoreset: on an env's reset call an action is selected from the recorded state and ignored; no update.
The step itself is not restated: its outputs (obs, reward, terminated, truncated) are inputs here.  s' is obs[k] except where a
same-step autoreset replaced it; there it matters only when truncated and not terminated, and is P[s][a] (noise-free cases).
"""
import numpy as np

EXPLORE_STREAM, ACTION_STREAM = 15, 16
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
    return int(np.ceil(np.float64(np.float32(eps)) * 2147483648.0))


def select(Q, s, w_e, w_a, E):
    """sel for every env: (actions, explored)"""
    n, _, A = Q.shape
    explored = (w_e >> np.uint32(1)).astype(np.int64) < E
    a_x = ((w_a.astype(np.uint64) * np.uint64(A)) >> np.uint64(32)).astype(np.int64)
    a_g = np.argmax(Q[np.arange(n), s], axis=1)
    return np.where(explored, a_x, a_g), explored


def run(algo, alpha, gamma, epsilon, Q, obs_before, obs, reward, terminated, truncated, P, autoreset, w_e, w_a, pending=None):
    """One launch of K steps.  Q float32 [N, S, A] (not modified); obs_before [N]; obs, reward, terminated, truncated [K, N];
    P [S, A]; w_e, w_a uint32 [K + 1, N] (row k: tick0 + k; the last row serves sarsa's sel(s', t + 1) of the last step);
    pending bool [N]: the env's next call is its reset (next-step autoreset).
    Returns (actions int64 [K, N], Q, pending, info); info counts what keeps a comparison honest."""
    assert algo in ("q_learning", "sarsa") and Q.dtype == np.float32
    sarsa = algo == "sarsa"
    alpha, gamma = np.float32(alpha), np.float32(gamma)
    E = epsilon_threshold(epsilon)
    Q = Q.copy()
    K, n = obs.shape
    idx = np.arange(n)
    s = np.asarray(obs_before).astype(np.int64)
    pending = np.zeros(n, bool) if pending is None else np.asarray(pending, bool).copy()
    have_carry, carry = np.zeros(n, bool), np.zeros(n, np.int64)
    actions = np.zeros((K, n), np.int64)
    info = dict(explored=0, greedy_ties=0, greedy_strict=0, carried=0, carried_differs=0, updates=0)
    for k in range(K):
        fresh, explored = select(Q, s, w_e[k], w_a[k], E)
        a = np.where(have_carry, carry, fresh)
        actions[k] = a
        info["explored"] += int(explored.sum())
        row = Q[idx, s]
        ties = (row == row.max(axis=1, keepdims=True)).sum(axis=1) > 1
        greedy = ~explored & ~have_carry
        info["greedy_ties"] += int((greedy & ties).sum())
        info["greedy_strict"] += int((greedy & ~ties).sum())
        info["carried"] += int(have_carry.sum())
        info["carried_differs"] += int((have_carry & (carry != fresh)).sum())
        live = ~pending                                   # (a reset call: nothing is learnt)
        te, tr = np.asarray(terminated[k], bool), np.asarray(truncated[k], bool)
        r = np.asarray(reward[k], np.float32)
        s2 = np.asarray(obs[k]).astype(np.int64)
        if autoreset == SAME_STEP:
            s2 = np.where(te | tr, P[s, a], s2)
        if sarsa:
            a2, _ = select(Q, s2, w_e[k + 1], w_a[k + 1], E)
            qn = Q[idx, s2, a2]
        else:
            a2 = np.zeros(n, np.int64)
            qn = Q[idx, s2].max(axis=1)
        g = gamma * qn
        y = np.where(te, r, r + g).astype(np.float32)
        q = Q[idx, s, a]
        d = y - q
        u = alpha * d
        assert g.dtype == d.dtype == u.dtype == np.float32
        Q[idx[live], s[live], a[live]] = (q + u)[live]
        info["updates"] += int(live.sum())
        have_carry = live & sarsa & ~te & ~(tr & (autoreset != DISABLED))
        carry = a2
        pending = live & (autoreset == NEXT_STEP) & (te | tr)
        s = np.asarray(obs[k]).astype(np.int64)
    return actions, Q, pending, info
