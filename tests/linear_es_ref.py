"""A numpy restatement of the linear policy ES (include/mdpp.h "Linear policy ES") from a launch's own outputs -- observations,
rewards and flags.  The normals come from the oracle's restatement of the Philox stream (oracle.philox_normals); nothing here
comes from the product.

Group g is the envs 64g .. 64g+63; member m = i - 64g, sign +1 for even m, -1 for odd m; both members of a pair read the stream
of the even member's env id.  Per env, at every step that is not a reset call, after the step's float32 reward rw:
    0 <= eps < T: ret += (double)rw
    terminated or truncated:  0 <= eps < T: acc += ret; ret = 0; eps += 1      eps == -1: eps = 0
Per group, after every step: every member at eps == T ends the generation (generation_end below).  The butterflies are six
explicit pairwise passes, v = v + v[lane ^ (1 << k)], in the precision of v."""
import numpy as np

import linear_policy_ref as ref

F32 = np.float32
STREAM = 19
GROUP = 64
ARRAYS = ("mean", "sigma", "gain", "gen", "acc", "ret", "fitness", "eps", "log_mean")
_LANES = np.arange(GROUP)
SIGN_PLUS = (_LANES & 1) == 0


def _normals(seed, env, tick, n):
    from oracle import oracle as ora
    return ora.philox_normals(seed, env, tick, STREAM, 1, n)[0].astype(F32)


def gain_of(sigma, lr):
    """lr / (sigma * float32(4032)) in float32: the product rounded, then the quotient"""
    sigma, lr = np.asarray(sigma, F32), np.asarray(lr, F32)
    return (lr / (sigma * F32(4032)).astype(F32)).astype(F32)


def butterfly(v):
    """six pairwise passes over 64 lanes in v's own dtype; every lane's result (all equal: addition is commutative)"""
    v = np.asarray(v).copy()
    assert v.shape == (GROUP,) and v.dtype in (F32, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(6):
            v = (v + v[_LANES ^ (1 << k)]).astype(v.dtype)
    return v


def ranks(acc):
    """r_m = 2 #{k_j < k_m} + #{j != m: k_j == k_m} - 63 on the keys k = isnan(acc) ? -inf : acc; int [64] in [-63, 63]"""
    acc = np.asarray(acc, np.float64)
    key = np.where(np.isnan(acc), -np.inf, acc)
    lt = (key[None, :] < key[:, None]).sum(1)
    eq = (key[None, :] == key[:, None]).sum(1) - 1
    return (2 * lt + eq - 63).astype(np.int64)


def new_state(mean_theta, sigma, lr, log_rows=0):
    """The ES before mdpp_linear_es_init: mean_theta float32 [G, D, D + 1]; sigma, lr scalars or float32 [G].  mean is kept
    entry-major, [E, G], like the product's array; cand [N, D, D + 1] is the handle's parameter buffer (zeros until init)."""
    mean_theta = np.asarray(mean_theta)
    assert mean_theta.dtype == F32 and mean_theta.ndim == 3 and mean_theta.shape[2] == mean_theta.shape[1] + 1
    G, d = mean_theta.shape[:2]
    n = GROUP * G
    sg = np.full(G, sigma, F32) if np.isscalar(sigma) else np.asarray(sigma).copy()
    rate = np.full(G, lr, F32) if np.isscalar(lr) else np.asarray(lr).copy()
    assert sg.dtype == F32 and sg.shape == (G,) and rate.dtype == F32 and rate.shape == (G,)
    return dict(cand=np.zeros((n, d, d + 1), F32), mean=np.ascontiguousarray(mean_theta.reshape(G, d * (d + 1)).T), sigma=sg,
                gain=gain_of(sg, rate), gen=np.zeros(G, np.int32), acc=np.zeros(n, np.float64), ret=np.zeros(n, np.float64),
                fitness=np.zeros(n, np.float64), eps=np.zeros(n, np.int32), log_mean=np.zeros((log_rows, G), np.float64))


def candidates(mu, sigma, z, fma=False):
    """mu float32 [E], z float32 [32 pairs, E]: the 64 members' candidates [64, E], mu +- sigma z with the product rounded
    before the sum (fma: what a fused multiply-add would give)"""
    zz = np.repeat(np.asarray(z, F32), 2, axis=0)
    with np.errstate(invalid="ignore", over="ignore"):
        if fma:
            t = np.float64(F32(sigma)) * zz.astype(np.float64)
            return np.where(SIGN_PLUS[:, None], np.asarray(mu, F32).astype(np.float64) + t, np.asarray(mu, F32).astype(np.float64) - t).astype(F32)
        t = (F32(sigma) * zz).astype(F32)
        return np.where(SIGN_PLUS[:, None], (np.asarray(mu, F32) + t).astype(F32), (np.asarray(mu, F32) - t).astype(F32))


def _pair_normals(normals, seed, env0, g, tick, E):
    return np.stack([normals(seed, env0 + GROUP * g + 2 * p, tick, E) for p in range(GROUP // 2)])


def init(s, *, seed, env0, normals=_normals):
    """mdpp_linear_es_init, in place: the candidates of the current gen; acc = ret = 0, eps = 0"""
    E, G = s["mean"].shape
    d = s["cand"].shape[1]
    for g in range(G):
        z = _pair_normals(normals, seed, env0, g, int(s["gen"][g]), E)
        s["cand"][GROUP * g:GROUP * (g + 1)] = candidates(s["mean"][:, g], s["sigma"][g], z).reshape(GROUP, d, d + 1)
    s["acc"][:] = 0.0
    s["ret"][:] = 0.0
    s["eps"][:] = 0
    return s


def move_mean(mean, gain, r, z0, fma=False):
    """mean float32 [E], r int [64], z0 float32 [32 pairs, E]: mean[e] + gain * S[e], S the float32 butterfly of
    (float)r_m * (s_m > 0 ? z0 : -z0); the product rounded, then the sum (fma: fused)"""
    z = np.repeat(np.asarray(z0, F32), 2, axis=0)
    E = z.shape[1]
    out = np.empty(E, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = (np.asarray(r).astype(F32)[:, None] * np.where(SIGN_PLUS[:, None], z, -z)).astype(F32)
        for e in range(E):
            S = butterfly(v[:, e])[0]
            if fma:
                out[e] = F32(np.float64(F32(gain)) * np.float64(S) + np.float64(F32(mean[e])))
            else:
                out[e] = F32(F32(mean[e]) + F32(F32(gain) * S))
    return out


def observe(s, i, rw, end, T):
    """one env, one step that is not a reset call"""
    counting = 0 <= s["eps"][i] < T
    if counting:
        s["ret"][i] += float(F32(rw))
    if end:
        if counting:
            s["acc"][i] += s["ret"][i]
            s["ret"][i] = 0.0
            s["eps"][i] += 1
        elif s["eps"][i] == -1:
            s["eps"][i] = 0


def vote(s, g, fresh, *, seed, env0, T, normals=_normals, info=None):
    """group g after a step: fresh bool [64] -- the member's step was no reset call and ended an episode.  True: a generation ended."""
    lo, hi = GROUP * g, GROUP * (g + 1)
    if not (s["eps"][lo:hi] == T).all():
        return False
    E = s["mean"].shape[0]
    d = s["cand"].shape[1]
    acc = s["acc"][lo:hi].copy()
    s["fitness"][lo:hi] = acc
    r = ranks(acc)
    gen = int(s["gen"][g])
    if gen < s["log_mean"].shape[0]:
        s["log_mean"][gen, g] = butterfly(acc)[0] * (1.0 / 64.0)
    z0 = _pair_normals(normals, seed, env0, g, gen, E)
    z1 = _pair_normals(normals, seed, env0, g, gen + 1, E)
    old = s["mean"][:, g].copy()
    mu = move_mean(old, s["gain"][g], r, z0)
    s["mean"][:, g] = mu
    cand = candidates(mu, s["sigma"][g], z1)
    s["cand"][lo:hi] = cand.reshape(GROUP, d, d + 1)
    if info is not None:
        info["ties"] += int(len(np.unique(r)) < GROUP)
        info["non_ties"] += int(len(np.unique(r)) > 1)
        info["mean_moved"] += int((mu.view(np.uint32) != old.view(np.uint32)).sum())
        info["fma_differs"] += int((move_mean(old, s["gain"][g], r, z0, fma=True).view(np.uint32) != mu.view(np.uint32)).sum())
        info["fma_differs"] += int((candidates(mu, s["sigma"][g], z1, fma=True).view(np.uint32) != cand.view(np.uint32)).sum())
    s["gen"][g] = gen + 1
    s["acc"][lo:hi] = 0.0
    s["ret"][lo:hi] = 0.0
    s["eps"][lo:hi] = np.where(np.asarray(fresh, bool), 0, -1)
    return True


def new_info():
    return dict(ties=0, non_ties=0, mean_moved=0, fma_differs=0, waiting=0, spare=0, steps=0)


def run_launch(state, obs0, obs, reward, terminated, truncated, *, seed, env0, T, amax, next_step=False, pending=None,
               normals=_normals, info=None):
    """One launch of K steps restated from its outputs: obs0 [N, D] (what every env shows before it), obs [K, N, D], reward and
    flags [K, N].  Returns (actions [K, N, D], the state after the launch -- a copy --, pending after the launch, ended: bool
    [K, G], where a generation ended).  info (new_info()) gathers the figures of the honesty conditions."""
    s = {k: v.copy() for k, v in state.items()}
    obs, reward = np.asarray(obs), np.asarray(reward)
    K, N, D = obs.shape
    G = N // GROUP
    seen = ref.observed(obs0, obs)
    pend = np.zeros(N, bool) if pending is None else np.asarray(pending, bool).copy()
    actions = np.zeros((K, N, D), F32)
    ended = np.zeros((K, G), bool)
    for k in range(K):
        actions[k] = ref.linear_actions(s["cand"], seen[k], amax)
        live = ~pend if next_step else np.ones(N, bool)
        end = live & (np.asarray(terminated[k], bool) | np.asarray(truncated[k], bool))
        if info is not None:
            info["waiting"] += int((live & (s["eps"] == -1)).sum())
            info["spare"] += int((live & (s["eps"] == T)).sum())
            info["steps"] += int(live.sum())
        for i in np.flatnonzero(live):
            observe(s, i, reward[k, i], end[i], T)
        for g in range(G):
            ended[k, g] = vote(s, g, end[GROUP * g:GROUP * (g + 1)], seed=seed, env0=env0, T=T, normals=normals, info=info)
        pend = end if next_step else pend
    return actions, s, pend, ended
