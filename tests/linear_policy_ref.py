"""A numpy restatement of the linear policy of closed-loop continuous rollouts (include/mdpp.h "Linear policies") and of the
episode-summary rule, from a launch's own outputs.  Nothing here comes from the product.

The action: for r = 0 .. D-1, acc = b[r], then for c = 0 .. D-1 in that order acc = acc + W[r][c] * o[c], every product and every
sum rounded to float32 (numpy's float32 multiply and add are two ufuncs: no fused multiply-add), then
a[r] = acc < -amax ? -amax : (acc > amax ? amax : acc); a NaN acc stays NaN."""
import numpy as np

F32 = np.float32


def linear_actions(theta, obs, amax):
    """theta float32 [D, D + 1] (one policy) or [N, D, D + 1] (one per env); obs float32 [..., N, D]: the state each env shows.
    Returns the actions, float32 of obs's shape, vectorised over envs and any leading axes."""
    theta = np.asarray(theta)
    obs = np.asarray(obs)
    assert theta.dtype == F32 and obs.dtype == F32
    D = obs.shape[-1]
    assert theta.shape[-2:] == (D, D + 1)
    amax = F32(amax)
    out = np.empty(obs.shape, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(D):
            acc = np.broadcast_to(theta[..., r, D], obs.shape[:-1]).astype(F32)
            for c in range(D):
                prod = (theta[..., r, c] * obs[..., c]).astype(F32)
                acc = (acc + prod).astype(F32)
            out[..., r] = np.where(acc < -amax, -amax, np.where(acc > amax, amax, acc))
    return out


def observed(obs0, obs):
    """What the policy reads at every step of a launch: obs0 [N, D], the observation before the launch, then obs[k - 1]."""
    return np.concatenate([np.asarray(obs0)[None], np.asarray(obs)[:-1]], axis=0)


def new_summary(n):
    return dict(ret=np.zeros(n, np.float64), len=np.zeros(n, np.int32), episodes=np.zeros(n, np.int32),
                return_sum=np.zeros(n, np.float64), length_sum=np.zeros(n, np.int32))


def summarise(summary, reward, terminated, truncated, next_step=False, pending=None):
    """The summary rule on one launch's outputs [K, N], in float64, step by step: for every step that is not a reset call
    ret += (double)reward, len += 1; terminated or truncated: episodes += 1, return_sum += ret, length_sum += len, ret = len = 0.
    next_step (next-step autoreset): the call after an episode's end is the env's reset call and is left out; ``pending``
    bool [N]: which envs enter the launch with that call ahead of them.  Returns (the updated copy, pending after the launch)."""
    s = {k: v.copy() for k, v in summary.items()}
    K, N = reward.shape
    pend = np.zeros(N, bool) if pending is None else np.asarray(pending, bool).copy()
    for k in range(K):
        live = ~pend if next_step else np.ones(N, bool)
        s["ret"] = np.where(live, s["ret"] + reward[k].astype(np.float32).astype(np.float64), s["ret"])
        s["len"] = s["len"] + live.astype(np.int32)
        end = live & (np.asarray(terminated[k], bool) | np.asarray(truncated[k], bool))
        s["episodes"] = s["episodes"] + end.astype(np.int32)
        s["return_sum"] = np.where(end, s["return_sum"] + s["ret"], s["return_sum"])
        s["length_sum"] = np.where(end, s["length_sum"] + s["len"], s["length_sum"]).astype(np.int32)
        s["ret"] = np.where(end, 0.0, s["ret"])
        s["len"] = np.where(end, 0, s["len"]).astype(np.int32)
        pend = end if next_step else pend
    return s, pend


def draw_theta(n, d, seed, g_max=2.0, spread=0.3, bias=0.2):
    """Per-env parameters [n, d, d + 1]: a contracting part -g I with g uniform in [0, g_max] per env, plus a random part
    (uniform +-spread on W, +-bias on b), so that some envs reach the origin and some run into the walls."""
    r = np.random.default_rng(seed)
    th = np.zeros((n, d, d + 1), np.float64)
    th[:, :, :d] = r.uniform(-spread, spread, (n, d, d))
    th[:, :, d] = r.uniform(-bias, bias, (n, d))
    g = r.uniform(0.0, g_max, n)
    th[:, np.arange(d), np.arange(d)] -= g[:, None]
    return th.astype(F32)
