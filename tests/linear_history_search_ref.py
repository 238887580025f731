"""The linear policy search and the linear policy ES under a policy WITH MEMORY, restated in numpy from a launch's own outputs.

tests/linear_search_ref.py and tests/linear_es_ref.py state the trial end and the generation end for E = D (D + 1); their
building blocks (perturb, ranks, butterfly, move_mean, candidates, the Philox normals of streams 18 and 19, observe) are generic
in E and are used as they are.  What is restated here is what is not: the loops over a launch, with the act and the memory rule
of tests/linear_history_ref.py and the candidates in the shape [N, D, 2 D + 1], E = D (2 D + 1).  The normal of entry e is the
e-th draw of the same stream.  Nothing here comes from the product."""
import numpy as np

import linear_es_ref as ler
import linear_history_ref as href
import linear_search_ref as lsr

F32 = np.float32
GROUP = ler.GROUP


def _step_carry(carry, o, end, mode):
    """the memory rule's bookkeeping after one act on o (linear_history_ref.launch, one step)"""
    carry["mem"] = o.copy()
    if mode == "next_step":
        carry["steps"] = np.where(carry["pending"], 0, carry["steps"] + 1)
        carry["pending"] = ~carry["pending"] & end
    else:
        carry["steps"] = carry["steps"] + 1
        if mode == "same_step":
            carry["steps"] = np.where(end, 0, carry["steps"])


def _act(cand, carry, o, amax):
    first = carry["steps"] == 0
    return href.history_actions(cand, o, np.where(first[:, None], o, carry["mem"]), amax)


# --- the (1+1)-ES per env

def search_new_state(theta, sigma):
    theta = np.asarray(theta)
    assert theta.dtype == F32 and theta.ndim == 3 and theta.shape[2] == 2 * theta.shape[1] + 1
    n = theta.shape[0]
    sg = np.full(n, sigma, F32) if np.isscalar(sigma) else np.asarray(sigma).copy()
    return dict(cand=theta.copy(), best=np.ascontiguousarray(theta.reshape(n, -1).T), sigma=sg,
                score=np.full(n, -np.inf, np.float64), acc=np.zeros(n, np.float64), ret=np.zeros(n, np.float64),
                eps=np.zeros(n, np.int32), trial=np.zeros(n, np.int32), accepted=np.zeros(n, np.int32))


def search_end_episode(s, i, *, seed, env_id, T, up, down, sigma_max):
    """linear_search_ref.end_episode over E = D (2 D + 1) entries"""
    s["acc"][i] += s["ret"][i]
    s["ret"][i] = 0.0
    s["eps"][i] += 1
    if s["eps"][i] != T:
        return False
    improved = bool(s["acc"][i] >= s["score"][i])
    if s["trial"][i] > 0:
        with np.errstate(over="ignore"):
            s["sigma"][i] = min(F32(s["sigma"][i] * F32(up)), F32(sigma_max)) if improved else F32(s["sigma"][i] * F32(down))
    shape = s["cand"].shape[1:]
    if improved:
        s["score"][i] = s["acc"][i]
        s["best"][:, i] = s["cand"][i].reshape(-1)
        s["accepted"][i] += 1
    s["trial"][i] += 1
    s["acc"][i] = 0.0
    s["eps"][i] = 0
    z = lsr._normals(seed, env_id, int(s["trial"][i]), shape[0] * shape[1])
    s["cand"][i] = lsr.perturb(s["best"][:, i], s["sigma"][i], z).reshape(shape)
    return True


def search_launch(state, carry, obs0, obs, reward, terminated, truncated, *, seed, env0, T, amax, mode="same_step", up=1.0,
                  down=1.0, sigma_max=np.inf):
    """Returns (actions [K, N, D], the search after the launch, the carry after the launch, ended bool [K, N])."""
    s = {k: v.copy() for k, v in state.items()}
    c = {k: v.copy() for k, v in carry.items()}
    obs, reward = np.asarray(obs), np.asarray(reward)
    K, N, D = obs.shape
    seen = np.concatenate([np.asarray(obs0, F32)[None], obs[:-1]], axis=0)
    actions, ended = np.zeros((K, N, D), F32), np.zeros((K, N), bool)
    for k in range(K):
        actions[k] = _act(s["cand"], c, seen[k], amax)
        live = ~c["pending"] if mode == "next_step" else np.ones(N, bool)
        s["ret"] = np.where(live, s["ret"] + reward[k].astype(F32).astype(np.float64), s["ret"])
        end = live & (np.asarray(terminated[k], bool) | np.asarray(truncated[k], bool))
        for i in np.flatnonzero(end):
            ended[k, i] = search_end_episode(s, i, seed=seed, env_id=env0 + int(i), T=T, up=up, down=down, sigma_max=sigma_max)
        _step_carry(c, seen[k], end, mode)
    return actions, s, c, ended


# --- the antithetic ES per 64 envs

def es_new_state(mean_theta, sigma, lr, log_rows=0):
    mean_theta = np.asarray(mean_theta)
    assert mean_theta.dtype == F32 and mean_theta.ndim == 3 and mean_theta.shape[2] == 2 * mean_theta.shape[1] + 1
    G, d, cols = mean_theta.shape
    n = GROUP * G
    sg, rate = np.full(G, sigma, F32), np.full(G, lr, F32)
    return dict(cand=np.zeros((n, d, cols), F32), mean=np.ascontiguousarray(mean_theta.reshape(G, -1).T), sigma=sg,
                gain=ler.gain_of(sg, rate), gen=np.zeros(G, np.int32), acc=np.zeros(n, np.float64), ret=np.zeros(n, np.float64),
                fitness=np.zeros(n, np.float64), eps=np.zeros(n, np.int32), log_mean=np.zeros((log_rows, G), np.float64))


def es_init(s, *, seed, env0):
    """mdpp_linear_es_init over E = D (2 D + 1) entries, in place"""
    E, G = s["mean"].shape
    shape = s["cand"].shape[1:]
    for g in range(G):
        z = ler._pair_normals(ler._normals, seed, env0, g, int(s["gen"][g]), E)
        s["cand"][GROUP * g:GROUP * (g + 1)] = ler.candidates(s["mean"][:, g], s["sigma"][g], z).reshape((GROUP,) + shape)
    s["acc"][:] = 0.0
    s["ret"][:] = 0.0
    s["eps"][:] = 0
    return s


def es_vote(s, g, fresh, *, seed, env0, T):
    """linear_es_ref.vote over E = D (2 D + 1) entries"""
    lo, hi = GROUP * g, GROUP * (g + 1)
    if not (s["eps"][lo:hi] == T).all():
        return False
    E = s["mean"].shape[0]
    acc = s["acc"][lo:hi].copy()
    s["fitness"][lo:hi] = acc
    r = ler.ranks(acc)
    gen = int(s["gen"][g])
    if gen < s["log_mean"].shape[0]:
        s["log_mean"][gen, g] = ler.butterfly(acc)[0] * (1.0 / 64.0)
    z0 = ler._pair_normals(ler._normals, seed, env0, g, gen, E)
    z1 = ler._pair_normals(ler._normals, seed, env0, g, gen + 1, E)
    mu = ler.move_mean(s["mean"][:, g].copy(), s["gain"][g], r, z0)
    s["mean"][:, g] = mu
    s["cand"][lo:hi] = ler.candidates(mu, s["sigma"][g], z1).reshape((GROUP,) + s["cand"].shape[1:])
    s["gen"][g] = gen + 1
    s["acc"][lo:hi] = 0.0
    s["ret"][lo:hi] = 0.0
    s["eps"][lo:hi] = np.where(np.asarray(fresh, bool), 0, -1)
    return True


def es_launch(state, carry, obs0, obs, reward, terminated, truncated, *, seed, env0, T, amax, mode="same_step"):
    """Returns (actions [K, N, D], the ES after the launch, the carry after the launch, ended bool [K, G])."""
    s = {k: v.copy() for k, v in state.items()}
    c = {k: v.copy() for k, v in carry.items()}
    obs, reward = np.asarray(obs), np.asarray(reward)
    K, N, D = obs.shape
    G = N // GROUP
    seen = np.concatenate([np.asarray(obs0, F32)[None], obs[:-1]], axis=0)
    actions, ended = np.zeros((K, N, D), F32), np.zeros((K, G), bool)
    for k in range(K):
        actions[k] = _act(s["cand"], c, seen[k], amax)
        live = ~c["pending"] if mode == "next_step" else np.ones(N, bool)
        end = live & (np.asarray(terminated[k], bool) | np.asarray(truncated[k], bool))
        for i in np.flatnonzero(live):
            ler.observe(s, i, reward[k, i], end[i], T)
        for g in range(G):
            ended[k, g] = es_vote(s, g, end[GROUP * g:GROUP * (g + 1)], seed=seed, env0=env0, T=T)
        _step_carry(c, seen[k], end, mode)
    return actions, s, c, ended
