"""The yardstick of the grid learners (RLToyVectorEnv.set_grid_learner / rollout_grid_learn / rollout_grid_eval): the index map and
the action map of include/mdpp.h "Grid learners", and a closed loop of oracle.GridOracle envs driven step by step by the
learner's restatement tests/learner_sweep_ref.py (select, update, tick_words: imported, not edited).  Shaped like
tests/closed_loop_cpu.py.  It imports nothing from the product but mdp.build_mdp, which reads a config.

  state index   s = c0 (g1 + 1) + c1,  S = (g0 + 1)(g1 + 1)      (a start cell may be the index g, one past the grid)
  action j      j < 4: component j >> 1 is +1 (j even) or -1 (j odd), the other 0;  j == 4: the noop
  tables        Q float32 [n, S, A]; as_grid() shows them as the product does, [n, g0 + 1, g1 + 1, A]

The envs run on Philox streams (the oracle keyed like the handle: seed, global env id, step counter) or, given the handle's
seeded stream words, on numpy streams.  On Philox streams the reset call of a next-step-autoreset env draws from the
feature-space stream of ITS OWN tick: the oracle keys that stream only inside step(), so the loop replaces the env by a
fresh oracle keyed at that tick, steps it once (the move is irrelevant, reset() overwrites it) and resets it.
"""
import numpy as np

import learner_sweep_ref as ref

ACTION_VECTORS = np.array([[1, 0], [-1, 0], [0, 1], [0, -1], [0, 0]], np.int32)
ALGOS = ("q_learning", "sarsa")


def n_states(grid_shape):
    return (int(grid_shape[0]) + 1) * (int(grid_shape[1]) + 1)


def state_index(c0, c1, grid_shape):
    return np.asarray(c0, np.int64) * (int(grid_shape[1]) + 1) + np.asarray(c1, np.int64)


def action_vector(j):
    """int32 [..., 2] of action indices j"""
    j = np.asarray(j, np.int64)
    v = np.zeros(j.shape + (2,), np.int32)
    move = j < 4
    sign = np.where(j & 1, -1, 1).astype(np.int32)
    d = j >> 1
    v[..., 0] = np.where(move & (d == 0), sign, 0)
    v[..., 1] = np.where(move & (d == 1), sign, 0)
    return v


def as_grid(Q, grid_shape):
    return Q.reshape(Q.shape[0], int(grid_shape[0]) + 1, int(grid_shape[1]) + 1, Q.shape[-1])


def as_flat(Qg):
    return np.ascontiguousarray(Qg).reshape(Qg.shape[0], Qg.shape[1] * Qg.shape[2], Qg.shape[3])


def _new_oracle(m):
    from oracle import oracle as ora
    return ora.GridOracle(m.grid_shape, m.target_point, m.make_denser, m.transition_noise, m.reward_noise,
                          m.reward_every_n_steps, m.reward_scale, m.reward_shift, m.term_state_reward)


def make_oracles(m, n, philox_seed=77, off=0, streams=None):
    """n oracle envs of the grid MDP m, reset: on the Philox streams of global env ids off ... off + n - 1, or (streams: the
    handle's seeded words of the env, feature-space and action-space streams, [3][n][6]) on numpy streams.  Returns (envs,
    first cells int64 [n, 2])."""
    envs, first = [], np.zeros((n, 2), np.int64)
    for i in range(n):
        o = _new_oracle(m)
        if streams is None:
            o.set_philox(philox_seed, off + i)
        else:
            o.set_rng(streams[0][i], streams[1][i], streams[2][i])
        first[i] = o.reset()
        envs.append(o)
    return envs, first


def new_info(n):
    info = ref.new_info(n)
    info.update(stay_steps=0, terminations=0, truncations=0, reset_calls=0, start_on_g=np.zeros(2, np.int64), redrawn_moves=0,
                greedy_selections=0)
    return info


def closed_loop(cfg, kw, algo, alpha, gamma, epsilon, n, q0=None, *, seed, K, launches, noop=False, philox_seed=77, off=0,
                streams=None, greedy=False, tick0=0, state=None):
    """launches x K steps of n envs under the handle's autoreset / max_episode_steps (kw) and the learner (algo, alpha, gamma,
    epsilon: scalars or arrays [n], its Philox key `seed`) starting from q0 (zeros), the handle's step counter at tick0.  A
    launch's first step selects afresh.  greedy: evaluation -- the lowest argmax, nothing learnt, no word drawn.  state: the
    dict a previous call returned as traj["state_out"] (the loop goes on where that one stopped; tick0 must follow on).
    Returns (info, Q [n, S, A], traj): traj a dict of [launches K, n(, 2)] arrays -- actions (indices), vectors, obs (as a
    handle returns them), reward float32, terminated, truncated, reset_call, cell (acted from), next_cell (after the move,
    before any reset) -- and obs0 [n, 2]."""
    from mdp_playground_amd import mdp as mdp_mod
    m = mdp_mod.build_mdp(dict(cfg))
    g = m.grid_shape
    A = 5 if noop else 4
    autoreset, max_steps = kw.get("autoreset", ref.SAME_STEP), kw.get("max_episode_steps", 0)
    if state is None:
        envs, cell = make_oracles(m, n, philox_seed, off, streams)
        pending, steps = np.zeros(n, bool), np.zeros(n, np.int64)
    else:
        envs, cell, pending, steps = state["envs"], state["cell"].copy(), state["pending"].copy(), state["steps"].copy()
    al, ga, E = ref.per_env(n, alpha, gamma, epsilon)
    Q = np.zeros((n, n_states(g), A), np.float32) if q0 is None else q0.copy()
    assert Q.shape == (n, n_states(g), A) and Q.dtype == np.float32
    info = new_info(n)
    if state is None:
        info["start_on_g"] += (cell == np.asarray(g[:2])).sum(axis=0)
    total = launches * K
    w = None if greedy else {st: ref.tick_words(seed, off, tick0, total + 1, n, st) for st in (ref.EXPLORE_STREAM, ref.ACTION_STREAM)}
    have_carry, carry = np.zeros(n, bool), np.zeros(n, np.int64)
    dropped = np.zeros(n, bool)
    traj = {k: np.zeros((total, n) + tail, dt) for k, tail, dt in (
        ("actions", (), np.int64), ("vectors", (2,), np.int32), ("obs", (2,), np.int64), ("reward", (), np.float32),
        ("terminated", (), bool), ("truncated", (), bool), ("reset_call", (), bool), ("cell", (2,), np.int64), ("next_cell", (2,), np.int64))}
    traj["obs0"] = cell.copy()
    hi = np.asarray(g[:2], np.int64) - 1
    for t in range(total):
        live = ~pending
        s = state_index(cell[:, 0], cell[:, 1], g)
        if greedy:
            a = ref.scan_best(Q[np.arange(n), s])[0]
            info["greedy_selections"] += int(live.sum())
        else:
            if t % K == 0:
                have_carry[:] = False                        # (a launch's first step selects afresh)
                dropped[:] = False
            fresh, _ = ref.select(algo, Q, s, w[ref.EXPLORE_STREAM][t], w[ref.ACTION_STREAM][t], E, info, ~have_carry)
            info["trunc_carry_differs"] += int((dropped & (carry != fresh)).sum())
            info["carried"] += int(have_carry.sum())
            info["carried_differs"] += int((have_carry & (carry != fresh)).sum())
            a = np.where(have_carry, carry, fresh)
        vec = action_vector(a)
        cell2, r, te = cell.copy(), np.zeros(n, np.float32), np.zeros(n, bool)
        for i in np.flatnonzero(live):
            o, rr, d = envs[i].step(vec[i])
            cell2[i], r[i], te[i] = o, np.float32(rr), d
        steps[live] += 1
        tr = live & (max_steps > 0) & (steps >= max_steps)
        expected = np.clip(cell + vec, 0, hi)
        info["redrawn_moves"] += int((live & (expected != cell2).any(axis=1)).sum())
        info["stay_steps"] += int((live & (cell2 == cell).all(axis=1)).sum())
        info["terminations"] += int((live & te).sum())
        info["truncations"] += int((live & tr).sum())
        info["reset_calls"] += int(pending.sum())
        traj["cell"][t], traj["next_cell"][t] = cell, cell2
        if not greedy:
            s2 = state_index(cell2[:, 0], cell2[:, 1], g)
            a2 = ref.select(algo, Q, s2, w[ref.EXPLORE_STREAM][t + 1], w[ref.ACTION_STREAM][t + 1], E)[0] if algo == "sarsa" else None
            ref.update(algo, Q, s, a, r, s2, te, live, al, ga, None, a2, info)
            cut = live & ~te & tr & (autoreset != ref.DISABLED)
            info["trunc_resets"] += int(cut.sum())
            have_carry = live & (algo == "sarsa") & ~te & ~cut
            dropped = cut & (algo == "sarsa")
            carry = a2 if a2 is not None else carry
        ended = live & (te | tr)
        reset_now = pending | (ended & (autoreset == ref.SAME_STEP))
        out = cell2.copy()
        for i in np.flatnonzero(reset_now):
            if pending[i] and streams is None:               # (Philox: the reset call's own tick keys the feature-space stream)
                envs[i] = _new_oracle(m)
                envs[i].set_philox(philox_seed, off + i, tick=tick0 + t)
                envs[i].step(np.zeros(2, np.int32))
            out[i] = envs[i].reset(explicit=False)
            steps[i] = 0
            info["start_on_g"] += out[i] == np.asarray(g[:2])
        for k, v in (("actions", a), ("vectors", vec), ("obs", out), ("reward", r), ("terminated", te), ("truncated", tr), ("reset_call", pending)):
            traj[k][t] = v
        pending = ended & (autoreset == ref.NEXT_STEP)
        cell = out
    traj["state_out"] = dict(envs=envs, cell=cell, pending=pending, steps=steps)
    return info, Q, traj
