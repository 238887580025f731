"""Tabular policies for closed-loop fused rollouts (RLToyVectorEnv.set_policy / rollout_policy).

The kernel samples a ~ pi(. | s) from a table of integer thresholds, T uint32 [S][A]: with m the upper 31 bits of the
step's Philox word,

    a = min(#{ j < A : T[s][j] <= m }, A - 1).

policy_thresholds makes T from probabilities the way numpy's Generator.choice makes its cdf (float64 cumsum, divided by its
last entry): T[s][j] = ceil(cdf[j] * 2^31).  m * 2^-31 and cdf[j] * 2^31 are exact in float64, so the count equals
searchsorted(cdf, m * 2^-31, 'right') -- the rule the library uses for start states on Philox streams.  T[s][A-1] = 2^31
is never <= m; a one-hot row gives thresholds 0 and 2^31 and is exactly deterministic; an action of probability zero has
T[j] == T[j-1] and is never drawn.

Host helpers of the in-kernel tabular learners (set_learner / rollout_learn) live here too: epsilon_threshold makes the
integer the kernel compares the explore word with, explore_action is its rule for the exploring action, and
check_learner_params is the validation set_learner applies.  alpha, gamma and epsilon are each a Python scalar (uniform over
the handle) or a 1-D array with one float32 per env (numpy, or a torch tensor on any device): learner_param_array tells the
two apart and validates the array.

Per-env noise levels (set_noise_levels) are validated and reduced here as the library does it: noise_level_array makes the
float64 [N] array of one key, noise_levels_reduce the distinct transition levels and each env's level byte,
noise_level_thresholds the Philox (T, M) pair of every level, noise_level_cdfs the [levels, S, S] table of the
categoricals' cdfs.

Per-episode schedules of the learners (set_learner_schedule): epsilon_decay makes one row of a table,
learner_schedule_arrays validates the tables and the envs' row indices and returns what the library takes.
"""
import numpy as np

__all__ = ["policy_thresholds", "epsilon_threshold", "explore_action", "check_learner_params", "learner_param_array", "LEARN_ALGOS",
           "noise_level_array", "grid_noise_level_array", "noise_levels_reduce", "noise_level_thresholds", "noise_level_cdfs", "MAX_NOISE_LEVELS",
           "epsilon_decay", "learner_schedule_arrays", "MAX_SCHEDULE_ENTRIES", "DECAY_KINDS"]

LEARN_ALGOS = ("q_learning", "sarsa", "double_q")
MAX_SCHEDULE_ENTRIES = 1 << 22   # R M of one schedule table (MDPP_MAX_SCHEDULE_ENTRIES)
DECAY_KINDS = ("linear", "log", "const")
MAX_NOISE_LEVELS = 16        # distinct transition_noise values one handle serves at a time (MDPP_MAX_NOISE_LEVELS)


def _to_numpy(policy):
    if hasattr(policy, "detach") and hasattr(policy, "cpu"):     # a torch tensor
        policy = policy.detach().cpu().numpy()
    return np.asarray(policy)


def policy_thresholds(policy, S, A):
    """policy: float [S, A] probabilities (finite, >= 0, every row summing to 1 within sqrt(float64 eps), numpy's own rule
    for choice(p=...)), or integer [S] -- the one action taken in each state.  A torch tensor is accepted for either.
    Returns the thresholds, np.uint32 [S, A]; raises ValueError on shape, range, NaN or row sum."""
    S, A = int(S), int(A)
    if S < 1 or A < 1:
        raise ValueError("policy_thresholds: S and A must be positive")
    p = _to_numpy(policy)
    if p.dtype == np.bool_ or not (np.issubdtype(p.dtype, np.integer) or np.issubdtype(p.dtype, np.floating)):
        raise ValueError(f"policy must be float [S, A] probabilities or integer [S] actions, got dtype {p.dtype}")
    if np.issubdtype(p.dtype, np.integer):
        if p.shape != (S,):
            raise ValueError(f"an integer policy must have shape ({S},), got {p.shape}")
        if p.size and (p.min() < 0 or p.max() >= A):
            raise ValueError(f"an integer policy's actions must lie in [0, {A})")
        T = np.zeros((S, A), np.uint32)
        T[np.arange(A)[None, :] >= p.astype(np.int64)[:, None]] = 2 ** 31
        return T
    if p.shape != (S, A):
        raise ValueError(f"a probability policy must have shape ({S}, {A}), got {p.shape}")
    p = p.astype(np.float64)
    if not np.all(np.isfinite(p)):
        raise ValueError("policy probabilities must be finite")
    if np.any(p < 0):
        raise ValueError("policy probabilities must be non-negative")
    if np.any(np.abs(p.sum(axis=1) - 1.0) > np.sqrt(np.finfo(np.float64).eps)):
        raise ValueError("every row of a probability policy must sum to 1")
    cdf = p.cumsum(axis=1)
    cdf /= cdf[:, -1:]
    return np.ceil(cdf * 2.0 ** 31).astype(np.uint32)


def epsilon_threshold(eps):
    """E = ceil(epsilon * 2^31) in float64, epsilon rounded to float32 first (the C ABI takes a float): a step explores iff
    (wE >> 1) < E, so epsilon = 0 never explores and epsilon = 1 always does.  An array gives np.uint32 thresholds, element-wise."""
    if _is_array(eps):
        e = _to_numpy(eps).astype(np.float32)
        if not np.all((e >= 0.0) & (e <= 1.0)):
            raise ValueError("every epsilon must lie in [0, 1]")
        return np.ceil(e.astype(np.float64) * 2147483648.0).astype(np.uint32)
    e = float(np.float32(eps))
    if not 0.0 <= e <= 1.0:
        raise ValueError(f"epsilon must lie in [0, 1], got {eps!r}")
    return int(np.ceil(np.float64(e) * 2147483648.0))


def explore_action(word, A):
    """The exploring action of a 32-bit word: (uint64(word) * A) >> 32."""
    return (np.asarray(word, dtype=np.uint64) * np.uint64(A)) >> np.uint64(32)


def _is_array(v):
    return isinstance(v, (np.ndarray, list, tuple)) or (hasattr(v, "detach") and hasattr(v, "cpu"))


def learner_param_array(name, v, num_envs=None):
    """None for a scalar (or None); for an array its float32 numpy copy, after the checks: 1-D, num_envs entries (when given),
    every element in range -- alpha in (0, 1], gamma and epsilon in [0, 1]; NaN fails.  ValueError otherwise."""
    if v is None or not _is_array(v):
        return None
    a = _to_numpy(v)
    if a.dtype == np.bool_ or not (np.issubdtype(a.dtype, np.integer) or np.issubdtype(a.dtype, np.floating)):
        raise ValueError(f"{name} must be a number or a 1-D array of numbers, got dtype {a.dtype}")
    if a.ndim != 1:
        raise ValueError(f"a per-env {name} must be 1-D, got shape {a.shape}")
    if num_envs is not None and a.shape[0] != int(num_envs):
        raise ValueError(f"a per-env {name} must have num_envs = {int(num_envs)} entries, got {a.shape[0]}")
    a = np.ascontiguousarray(a, dtype=np.float32)
    ok = (a > 0.0) & (a <= 1.0) if name == "alpha" else (a >= 0.0) & (a <= 1.0)       # (NaN fails both)
    if not np.all(ok):
        bad = int(np.argmin(ok))
        raise ValueError(f"{name} must lie in {'(0, 1]' if name == 'alpha' else '[0, 1]'}, got {a[bad]!r} at env {bad}")
    return a


def check_learner_params(algo, alpha, gamma, epsilon, num_envs=None):
    """ValueError unless algo is known, alpha in (0, 1], gamma and epsilon in [0, 1] (None: not checked).  Each of the three
    is a scalar or a per-env array (learner_param_array: 1-D, num_envs entries when num_envs is given, every element in range)."""
    if algo is not None and algo not in LEARN_ALGOS:
        raise ValueError(f"algo must be one of {LEARN_ALGOS}, got {algo!r}")
    arrays = [n for n, v in (("alpha", alpha), ("gamma", gamma), ("epsilon", epsilon)) if _is_array(v)]
    for n, v in (("alpha", alpha), ("gamma", gamma), ("epsilon", epsilon)):
        if n in arrays:
            learner_param_array(n, v, num_envs)
    alpha = None if "alpha" in arrays else alpha
    gamma = None if "gamma" in arrays else gamma
    epsilon = None if "epsilon" in arrays else epsilon
    if alpha is not None and not 0.0 < float(np.float32(alpha)) <= 1.0:
        raise ValueError(f"alpha must lie in (0, 1], got {alpha!r}")
    for name, v in (("gamma", gamma), ("epsilon", epsilon)):
        if v is not None and not 0.0 <= float(np.float32(v)) <= 1.0:
            raise ValueError(f"{name} must lie in [0, 1], got {v!r}")


def noise_level_array(name, v, num_envs, max_levels=MAX_NOISE_LEVELS):
    """The per-env levels of one noise key, ``name`` "transition_noise" or "reward_noise": None for None; otherwise a float64
    numpy [num_envs] -- a scalar is broadcast, an array (numpy, or a torch tensor on any device) must be 1-D with num_envs
    entries.  transition_noise lies in [0, 1] (-0.0 becomes 0.0) with at most MAX_NOISE_LEVELS distinct values, reward_noise is
    finite and >= 0; NaN fails.  ValueError, naming the key, otherwise.  ``max_levels=None``: no limit on the distinct values
    (grid_noise_level_array)."""
    if name not in ("transition_noise", "reward_noise"):
        raise ValueError(f"unknown noise key {name!r}")
    if v is None:
        return None
    n = int(num_envs)
    if _is_array(v):
        a = _to_numpy(v)
        if a.dtype == np.bool_ or not (np.issubdtype(a.dtype, np.integer) or np.issubdtype(a.dtype, np.floating)):
            raise ValueError(f"{name} must be a number or a 1-D array of numbers, got dtype {a.dtype}")
        if a.ndim != 1:
            raise ValueError(f"per-env {name} must be 1-D, got shape {a.shape}")
        if a.shape[0] != n:
            raise ValueError(f"per-env {name} must have num_envs = {n} entries, got {a.shape[0]}")
        a = np.array(a, dtype=np.float64)
    else:
        a = np.full(n, float(v), dtype=np.float64)
    ok = (a >= 0.0) & (a <= 1.0) if name == "transition_noise" else (a >= 0.0) & np.isfinite(a)      # (NaN fails both)
    if not np.all(ok):
        bad = int(np.argmin(ok))
        raise ValueError(f"{name} must {'lie in [0, 1]' if name == 'transition_noise' else 'be finite and >= 0'}, got {a[bad]!r} at env {bad}")
    if name == "transition_noise":
        a[a == 0.0] = 0.0
        k = len(np.unique(a))
        if max_levels is not None and k > max_levels:
            raise ValueError(f"transition_noise has {k} distinct values, at most {max_levels} levels are served")
    return a


def grid_noise_level_array(name, v, num_envs):
    """noise_level_array for a GRID handle (set_grid_noise_levels): the same checks and the same float64 [num_envs] result,
    without the limit on distinct transition_noise values -- the grid kernels keep no per-level table."""
    return noise_level_array(name, v, num_envs, max_levels=None)


def noise_levels_reduce(transition_noise):
    """(levels, index): the distinct values of a float64 [N] transition_noise array in ascending order, and each env's level
    as a uint8 index into them.  More than MAX_NOISE_LEVELS levels: ValueError."""
    a = np.asarray(transition_noise, dtype=np.float64)
    levels, index = np.unique(a, return_inverse=True)
    if len(levels) > MAX_NOISE_LEVELS:
        raise ValueError(f"transition_noise has {len(levels)} distinct values, at most {MAX_NOISE_LEVELS} levels are served")
    return levels, index.reshape(a.shape).astype(np.uint8)


def noise_level_thresholds(levels, S):
    """(T uint32 [levels], M uint64 [levels]) of Philox streams: T = ceil(p 2^32) capped at 2^32 - 1, M = ceil(2^64 (S - 1) / T),
    0 when S < 2 or T <= S - 1 (the library's philox_pnoise_threshold / philox_pnoise_magic).  p == 0: T = M = 0, no noise."""
    T, M = [], []
    for p in np.asarray(levels, dtype=np.float64):
        t = min(int(np.ceil(p * 4294967296.0)), 4294967295) if p > 0.0 else 0
        T.append(t)
        M.append(0 if (S < 2 or t <= S - 1) else -((-(int(S - 1) << 64)) // t))
    return np.asarray(T, dtype=np.uint32), np.asarray(M, dtype=np.uint64)


def noise_level_cdfs(levels, S):
    """float64 [levels, S, S]: row n of block l is the normalised cdf numpy's Generator.choice builds for the transition-noise
    categorical with mode n at p = levels[l] (DiscreteMDP.noise_cdf; rl_toy_env.py:1605-1612).  A level of value 0 is never
    read (the env makes no draw): zeros."""
    levels = np.asarray(levels, dtype=np.float64)
    out = np.zeros((len(levels), S, S), dtype=np.float64)
    for l, p in enumerate(levels):
        if not p > 0.0:
            continue
        for n in range(S):
            probs = np.ones(shape=(S,)) * p / (S - 1)
            probs[n] = 1 - p
            cdf = probs.cumsum()
            cdf /= cdf[-1]
            out[l, n] = cdf
    return out


def epsilon_decay(kind, start, num_episodes, final=0.0):
    """One row of a per-episode table (set_learner_schedule), float64 [num_episodes]: entry e is the value of episode e.  With
    x = e / max(num_episodes - 1, 1):
        "const":   start
        "linear":  start + (final - start) x
        "log":     start (final / start) ** x        (needs start > 0 and final > 0)
    so the first entry is ``start`` and, for num_episodes > 1, the last is ``final``.  These are THIS project's definitions: the
    reference's experiment files name the three kinds ("epsilon_decay": ["linear", "log", "const"]) and ship no tabular agent
    that would define them.  The row serves epsilon and alpha alike; the table's range checks are learner_schedule_arrays'."""
    if kind not in DECAY_KINDS:
        raise ValueError(f"epsilon_decay: kind must be one of {DECAY_KINDS}, got {kind!r}")
    m = int(num_episodes)
    if m != num_episodes or m < 1:
        raise ValueError(f"epsilon_decay: num_episodes must be a positive integer, got {num_episodes!r}")
    start, final = float(start), float(final)
    if not (np.isfinite(start) and np.isfinite(final)):
        raise ValueError("epsilon_decay: start and final must be finite")
    x = np.arange(m, dtype=np.float64) / np.float64(max(m - 1, 1))
    if kind == "const":
        return np.full(m, start, dtype=np.float64)
    if kind == "linear":
        return start + (final - start) * x
    if not (start > 0.0 and final > 0.0):
        raise ValueError(f"epsilon_decay: \"log\" needs start > 0 and final > 0, got start = {start!r}, final = {final!r}")
    return start * (final / start) ** x


def _schedule_table(name, v):
    a = _to_numpy(v)
    if a.dtype == np.bool_ or not (np.issubdtype(a.dtype, np.integer) or np.issubdtype(a.dtype, np.floating)):
        raise ValueError(f"a schedule's {name} table must hold numbers, got dtype {a.dtype}")
    if a.ndim not in (1, 2):
        raise ValueError(f"a schedule's {name} table must be [M] or [R, M], got shape {a.shape}")
    a = np.ascontiguousarray(a.reshape(1, -1) if a.ndim == 1 else a, dtype=np.float32)
    if a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"a schedule's {name} table needs at least one row and one entry, got shape {a.shape}")
    if a.size > MAX_SCHEDULE_ENTRIES:
        raise ValueError(f"a schedule's {name} table has {a.size} entries, at most 2^22 = {MAX_SCHEDULE_ENTRIES} are served")
    ok = (a > 0.0) & (a <= 1.0) if name == "alpha" else (a >= 0.0) & (a <= 1.0)       # (NaN fails both)
    if not np.all(ok):
        r, e = (int(x) for x in np.argwhere(~ok)[0])
        raise ValueError(f"a schedule's {name} must lie in {'(0, 1]' if name == 'alpha' else '[0, 1]'} as float32, got {a[r, e]!r} "
                         f"at row {r}, episode {e}")
    return a


def learner_schedule_arrays(epsilon=None, alpha=None, row=None, num_envs=None):
    """What set_learner_schedule hands the library, after every check: (epsilon, alpha, row, R, M) with the tables float32
    [R, M] (None: that parameter is not scheduled) and row int32 [num_envs] (None when R == 1).  A table is [M] (one row) or
    [R, M], numpy or a torch tensor on any device; epsilon lies in [0, 1], alpha -- as float32 -- in (0, 1]; NaN fails; at
    least one table is given, two have the same shape, 1 <= M and R M <= 2^22.  ``row`` is an integer array of num_envs entries
    in [0, R): the table row env i of THE HANDLE follows; required iff R > 1 (with R == 1 it may be given, all zeros).
    ValueError otherwise."""
    if epsilon is None and alpha is None:
        raise ValueError("a schedule needs an epsilon table, an alpha table or both")
    eps = None if epsilon is None else _schedule_table("epsilon", epsilon)
    al = None if alpha is None else _schedule_table("alpha", alpha)
    if eps is not None and al is not None and eps.shape != al.shape:
        raise ValueError(f"a schedule's tables must have one shape, got epsilon {eps.shape} and alpha {al.shape}")
    R, M = (eps if eps is not None else al).shape
    if row is None:
        if R > 1:
            raise ValueError(f"a schedule of R = {R} rows needs row, the row index of every env")
        return eps, al, None, R, M
    r = _to_numpy(row)
    if r.dtype == np.bool_ or not np.issubdtype(r.dtype, np.integer):
        raise ValueError(f"a schedule's row must be an integer array, got dtype {r.dtype}")
    if r.ndim != 1 or (num_envs is not None and r.shape[0] != int(num_envs)):
        raise ValueError(f"a schedule's row must be 1-D with num_envs{'' if num_envs is None else ' = %d' % int(num_envs)} entries, got shape {r.shape}")
    if r.size and (r.min() < 0 or r.max() >= R):
        raise ValueError(f"a schedule's row indices must lie in [0, {R}), got {int(r.min() if r.min() < 0 else r.max())}")
    return eps, al, (None if R == 1 else np.ascontiguousarray(r, dtype=np.int32)), R, M
