"""A numpy restatement of the linear policy search (include/mdpp.h "Linear policy search") from a launch's own outputs --
observations, rewards and flags.  The normals come from the oracle's restatement of the Philox stream
(oracle.philox_normals); nothing here comes from the product.

Per env, at every step that is not a reset call, after the step's float32 reward rw:
    ret += (double)rw
    terminated or truncated: acc += ret; ret = 0; eps += 1
        eps == T: improved = acc >= score (false for NaN)
                  trial > 0: sigma = improved ? min(sigma * up, sigma_max) : sigma * down          (float32)
                  improved: score = acc; best = cand; accepted += 1
                  trial += 1; acc = 0; eps = 0
                  cand[e] = best[e] + sigma * z[e], z = the first E normals of stream (seed, env id, trial, 18); a float32
                  product, rounded, then a float32 sum, rounded (numpy's multiply and add are two ufuncs: no FMA)
The candidate acts from the next action on (the action of a next-step-autoreset reset call included)."""
import numpy as np

import linear_policy_ref as ref

F32 = np.float32
STREAM = 18
ARRAYS = ("best", "sigma", "score", "acc", "ret", "eps", "trial", "accepted")


def _normals(seed, env, tick, n):
    from oracle import oracle as ora
    return ora.philox_normals(seed, env, tick, STREAM, 1, n)[0].astype(F32)


def new_state(theta, sigma):
    """The search at its start: theta float32 [N, D, D + 1] is trial 0's candidate and the first incumbent; sigma a scalar or
    float32 [N].  best is kept entry-major, [E, N], like the product's array."""
    theta = np.asarray(theta)
    assert theta.dtype == F32 and theta.ndim == 3 and theta.shape[2] == theta.shape[1] + 1
    n, d = theta.shape[:2]
    sg = np.full(n, sigma, F32) if np.isscalar(sigma) else np.asarray(sigma).copy()
    assert sg.dtype == F32 and sg.shape == (n,)
    return dict(cand=theta.copy(), best=np.ascontiguousarray(theta.reshape(n, d * (d + 1)).T), sigma=sg,
                score=np.full(n, -np.inf, np.float64), acc=np.zeros(n, np.float64), ret=np.zeros(n, np.float64),
                eps=np.zeros(n, np.int32), trial=np.zeros(n, np.int32), accepted=np.zeros(n, np.int32))


def perturb(best, sigma, z):
    """best + sigma * z in float32, the product rounded before the sum"""
    with np.errstate(invalid="ignore", over="ignore"):
        step = (F32(sigma) * np.asarray(z, F32)).astype(F32)
        return (np.asarray(best, F32) + step).astype(F32)


def perturb_fma(best, sigma, z):
    """what a fused multiply-add would give: the exact product (float64 holds it) added to best, rounded once"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.float64(F32(sigma)) * np.asarray(z, F32).astype(np.float64) + np.asarray(best, F32).astype(np.float64)).astype(F32)


def end_episode(s, i, *, seed, env_id, T, up=1.0, down=1.0, sigma_max=np.inf, normals=_normals):
    """env i's episode has ended (ret already holds its return): the rule from `acc += ret` on, in place.  True: a trial ended."""
    s["acc"][i] += s["ret"][i]
    s["ret"][i] = 0.0
    s["eps"][i] += 1
    if s["eps"][i] != T:
        return False
    improved = bool(s["acc"][i] >= s["score"][i])
    if s["trial"][i] > 0:
        with np.errstate(over="ignore"):
            s["sigma"][i] = min(F32(s["sigma"][i] * F32(up)), F32(sigma_max)) if improved else F32(s["sigma"][i] * F32(down))
    n, d = s["cand"].shape[:2]
    if improved:
        s["score"][i] = s["acc"][i]
        s["best"][:, i] = s["cand"][i].reshape(-1)
        s["accepted"][i] += 1
    s["trial"][i] += 1
    s["acc"][i] = 0.0
    s["eps"][i] = 0
    z = normals(seed, env_id, int(s["trial"][i]), d * (d + 1))
    s["cand"][i] = perturb(s["best"][:, i], s["sigma"][i], z).reshape(d, d + 1)
    return True


def run_launch(state, obs0, obs, reward, terminated, truncated, *, seed, env0, T, amax, up=1.0, down=1.0, sigma_max=np.inf,
               next_step=False, pending=None, normals=_normals):
    """One launch of K steps restated from its outputs: obs0 [N, D] (what every env shows before it), obs [K, N, D], reward and
    flags [K, N].  Returns (actions [K, N, D], the state after the launch -- a copy --, pending after the launch, ended: bool
    [K, N], where a trial ended)."""
    s = {k: v.copy() for k, v in state.items()}
    obs, reward = np.asarray(obs), np.asarray(reward)
    K, N, D = obs.shape
    seen = ref.observed(obs0, obs)
    pend = np.zeros(N, bool) if pending is None else np.asarray(pending, bool).copy()
    actions = np.zeros((K, N, D), F32)
    ended = np.zeros((K, N), bool)
    for k in range(K):
        actions[k] = ref.linear_actions(s["cand"], seen[k], amax)
        live = ~pend if next_step else np.ones(N, bool)
        s["ret"] = np.where(live, s["ret"] + reward[k].astype(F32).astype(np.float64), s["ret"])
        end = live & (np.asarray(terminated[k], bool) | np.asarray(truncated[k], bool))
        for i in np.flatnonzero(end):
            ended[k, i] = end_episode(s, i, seed=seed, env_id=env0 + int(i), T=T, up=up, down=down, sigma_max=sigma_max, normals=normals)
        pend = end if next_step else pend
    return actions, s, pend, ended
