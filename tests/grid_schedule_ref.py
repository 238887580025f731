"""The yardstick of the grid learners' per-episode schedules and episode log (RLToyVectorEnv.set_grid_learner_schedule,
rollout_grid_learn(K, summary=, log=); include/mdpp.h "Grid learner schedules and the episode log"): the closed loop of
tests/grid_learner_ref.closed_loop over oracle.GridOracle envs, with the agent of tests/learner_schedule_ref.py (Agent /
Schedule: act, then learn) in place of fixed rates.  The log is tests/episode_log_ref.run on the loop's trajectory.  It
imports nothing from the product but mdp.build_mdp, which reads a config (through grid_learner_ref).

What the loop adds to the agent's counters (learner_schedule_ref.new_info): terminations, truncations, start_on_g,
redrawn_moves, as grid_learner_ref counts them."""
import numpy as np

import episode_log_ref as lref
import grid_learner_ref as gref
import learner_schedule_ref as sref
import learner_sweep_ref as ref


def closed_loop(cfg, kw, algo, alpha, gamma, epsilon, n, q0=None, sched=None, *, seed, K, launches, noop=False, philox_seed=77, off=0,
                streams=None, tick0=0, state=None, ep=None):
    """launches x K learning steps of n envs under the handle's autoreset / max_episode_steps (kw) and the learner (algo, its own
    alpha, gamma, epsilon: scalars or arrays [n]; sched: a learner_schedule_ref.Schedule or None) from q0 (zeros) and the
    counters ep (zeros).  state: traj["state_out"] of a previous call (tick0 must follow on).  Returns (info, Q [n, S, A], ep
    int64 [n], traj): traj as grid_learner_ref.closed_loop's -- actions, vectors, obs, reward, terminated, truncated,
    reset_call [launches K, n(, 2)], obs0 -- and E, alpha [launches K, n], the values each step began with."""
    from mdp_playground_amd import mdp as mdp_mod
    m = mdp_mod.build_mdp(dict(cfg))
    g = m.grid_shape
    A = 5 if noop else 4
    autoreset, max_steps = kw.get("autoreset", ref.SAME_STEP), kw.get("max_episode_steps", 0)
    if state is None:
        envs, cell = gref.make_oracles(m, n, philox_seed, off, streams)
        pending, steps = np.zeros(n, bool), np.zeros(n, np.int64)
    else:
        envs, cell, pending, steps = state["envs"], state["cell"].copy(), state["pending"].copy(), state["steps"].copy()
    Q = np.zeros((n, gref.n_states(g), A), np.float32) if q0 is None else q0.copy()
    assert Q.shape == (n, gref.n_states(g), A) and Q.dtype == np.float32
    agent = sref.Agent(algo, n, alpha, gamma, epsilon, sched, Q, autoreset, ep=ep, pending=pending)
    info = agent.info
    info.update(terminations=0, truncations=0, redrawn_moves=0, start_on_g=np.zeros(2, np.int64))
    if state is None:
        info["start_on_g"] += (cell == np.asarray(g[:2])).sum(axis=0)
    total = launches * K
    w = {st: ref.tick_words(seed, off, tick0, total + 1, n, st) for st in (ref.EXPLORE_STREAM, ref.ACTION_STREAM)}
    traj = {k: np.zeros((total, n) + tail, dt) for k, tail, dt in (
        ("actions", (), np.int64), ("vectors", (2,), np.int32), ("obs", (2,), np.int64), ("reward", (), np.float32),
        ("terminated", (), bool), ("truncated", (), bool), ("reset_call", (), bool), ("E", (), np.int64), ("alpha", (), np.float32))}
    traj["obs0"] = cell.copy()
    hi = np.asarray(g[:2], np.int64) - 1
    for t in range(total):
        assert np.array_equal(pending, agent.pending)
        live = ~pending
        s = gref.state_index(cell[:, 0], cell[:, 1], g)
        if t % K == 0:
            agent.launch_start()
        a = agent.act(s, w[ref.EXPLORE_STREAM][t], w[ref.ACTION_STREAM][t])
        traj["E"][t], traj["alpha"][t] = agent.E_step, agent.al_step
        vec = gref.action_vector(a)
        cell2, r, te = cell.copy(), np.zeros(n, np.float32), np.zeros(n, bool)
        for i in np.flatnonzero(live):
            o, rr, d = envs[i].step(vec[i])
            cell2[i], r[i], te[i] = o, np.float32(rr), d
        steps[live] += 1
        tr = live & (max_steps > 0) & (steps >= max_steps)
        info["redrawn_moves"] += int((live & (np.clip(cell + vec, 0, hi) != cell2).any(axis=1)).sum())
        info["terminations"] += int((live & te).sum())
        info["truncations"] += int((live & tr).sum())
        s2 = gref.state_index(cell2[:, 0], cell2[:, 1], g)
        agent.learn(s, a, r, s2, te, tr, w[ref.EXPLORE_STREAM][t + 1], w[ref.ACTION_STREAM][t + 1], None)
        ended = live & (te | tr)
        reset_now = pending | (ended & (autoreset == ref.SAME_STEP))
        out = cell2.copy()
        for i in np.flatnonzero(reset_now):
            if pending[i] and streams is None:               # (Philox: the reset call's own tick keys the feature-space stream)
                envs[i] = gref._new_oracle(m)
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
    return info, agent.Q, agent.ep.copy(), traj


def log_of(traj, K, launches, M, state5=None, log=None, counters=None, fill_ret=0.0, fill_len=0):
    """The five summary values and the log of capacity M after the trajectory's launches, launch by launch
    (episode_log_ref.run); returns (log, state5, counters)."""
    n = traj["reward"].shape[1]
    st = lref.new_state5(n) if state5 is None else state5
    lg = lref.new_log(n, M, fill_ret, fill_len) if log is None else log
    counters = lref.new_counters() if counters is None else counters
    for launch in range(launches):
        sl = slice(launch * K, (launch + 1) * K)
        lg, st = lref.run(traj["reward"][sl], traj["terminated"][sl], traj["truncated"][sl], traj["reset_call"][sl], st, lg, counters)
    return lg, st, counters
