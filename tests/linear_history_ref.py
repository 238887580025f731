"""A numpy restatement of the linear policy WITH MEMORY of closed-loop continuous rollouts (include/mdpp.h "Linear policies with
memory") -- the act and the memory rule -- from a launch's own outputs.  Nothing here comes from the product.

theta float32 [D, 2 D + 1] or [N, D, 2 D + 1]: W = theta[.., :D], V = theta[.., D:2 D], b = theta[.., 2 D].  The action:
for r = 0 .. D-1, acc = b[r]; then for c = 0 .. D-1 in that order acc = acc + W[r][c] * o[c]; then for c = 0 .. D-1 in that
order acc = acc + V[r][c] * p[c]; every product and every sum rounded to float32 (numpy's float32 multiply and add are two
ufuncs: no fused multiply-add); then a[r] = acc < -amax ? -amax : (acc > amax ? amax : acc); a NaN acc stays NaN.

The memory rule: p = o where the env's count of steps taken in its current episode is 0 when the action is formed, the env's
memory otherwise; after the action is formed the memory becomes o -- on the reset call of a next-step-autoreset env too.  The
count is followed from the flags a launch returned: a reset call sets it to 0, every other step adds 1, and a same-step reset
(terminated or truncated) sets it to 0 again."""
import numpy as np

F32 = np.float32


def history_actions(theta, o, p, amax):
    """theta float32 [D, 2 D + 1] or [N, D, 2 D + 1]; o, p float32 [..., N, D].  The actions, float32 of o's shape."""
    theta, o, p = np.asarray(theta), np.asarray(o), np.asarray(p)
    assert theta.dtype == F32 and o.dtype == F32 and p.dtype == F32 and o.shape == p.shape
    D = o.shape[-1]
    assert theta.shape[-2:] == (D, 2 * D + 1)
    amax = F32(amax)
    out = np.empty(o.shape, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(D):
            acc = np.broadcast_to(theta[..., r, 2 * D], o.shape[:-1]).astype(F32)
            for c in range(D):
                prod = (theta[..., r, c] * o[..., c]).astype(F32)
                acc = (acc + prod).astype(F32)
            for c in range(D):
                prod = (theta[..., r, D + c] * p[..., c]).astype(F32)
                acc = (acc + prod).astype(F32)
            out[..., r] = np.where(acc < -amax, -amax, np.where(acc > amax, amax, acc))
    return out


def new_carry(obs0, steps0=None):
    """What crosses launches, as a policy just set on envs showing obs0 [N, D] has it: the memory (the current state), the
    step counts (0 after a reset) and, for next-step autoreset, which envs have their reset call ahead of them (none)."""
    obs0 = np.asarray(obs0, F32)
    n = obs0.shape[0]
    return dict(mem=obs0.copy(), steps=np.zeros(n, np.int64) if steps0 is None else np.asarray(steps0, np.int64).copy(),
                pending=np.zeros(n, bool))


def launch(theta, carry, obs0, obs, terminated, truncated, mode, amax):
    """One launch, from its outputs.  carry: new_carry()'s dict BEFORE the launch; obs0 [N, D]: what every env showed before it;
    obs [K, N, D], terminated / truncated [K, N]: what it returned; mode: "same_step", "next_step" or "disabled".
    Returns (actions [K, N, D], p [K, N, D] -- what the V pass read --, first bool [K, N] -- the step count was 0 --, the carry
    after the launch)."""
    obs = np.asarray(obs)
    K, N, D = obs.shape
    mem, steps, pending = carry["mem"].copy(), carry["steps"].copy(), carry["pending"].copy()
    seen = np.concatenate([np.asarray(obs0, F32)[None], obs[:-1]], axis=0)
    acts, ps, firsts = np.empty((K, N, D), F32), np.empty((K, N, D), F32), np.empty((K, N), bool)
    for k in range(K):
        o = seen[k]
        first = steps == 0
        p = np.where(first[:, None], o, mem)
        acts[k] = history_actions(theta, o, p, amax)
        ps[k], firsts[k] = p, first
        mem = o.copy()
        end = np.asarray(terminated[k], bool) | np.asarray(truncated[k], bool)
        if mode == "next_step":
            steps = np.where(pending, 0, steps + 1)
            pending = ~pending & end
        else:
            steps = steps + 1
            if mode == "same_step":
                steps = np.where(end, 0, steps)
    return acts, ps, firsts, dict(mem=mem, steps=steps, pending=pending)
