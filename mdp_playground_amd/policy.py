"""Tabular policies for closed-loop fused rollouts (RLToyVectorEnv.set_policy / rollout_policy).

The kernel samples a ~ pi(. | s) from a table of integer thresholds, T uint32 [S][A]: with m the upper 31 bits of the
step's Philox word,

    a = min(#{ j < A : T[s][j] <= m }, A - 1).

policy_thresholds makes T from probabilities the way numpy's Generator.choice makes its cdf (float64 cumsum, divided by its
last entry): T[s][j] = ceil(cdf[j] * 2^31).  m * 2^-31 and cdf[j] * 2^31 are exact in float64, so the count equals
searchsorted(cdf, m * 2^-31, 'right') -- the rule the library uses for start states on Philox streams.  T[s][A-1] = 2^31
is never <= m; a one-hot row gives thresholds 0 and 2^31 and is exactly deterministic; an action of probability zero has
T[j] == T[j-1] and is never drawn.
"""
import numpy as np

__all__ = ["policy_thresholds"]


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

