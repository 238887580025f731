"""The scheduled learners' closed loop on the CPU, beside tests/closed_loop_cpu.py: n oracle envs on Philox streams driven step
by step by tests/learner_schedule_ref.py's Agent.  It predicts a scheduled learning launch without a GPU and shows that the
counters tests/learner_schedule_cases.py asserts can be met before any GPU run."""
import numpy as np

import closed_loop_cpu as cl
import learner_schedule_ref as sref
import learner_sweep_ref as ref


def closed_loop(cfg, kw, algo, alpha, gamma, epsilon, sched, n, *, seed, K, launches, philox_seed=77, off=0):
    """launches x K steps of n envs under the handle's autoreset / max_episode_steps (kw) and the scheduled learner.  Returns
    (agent, traj): the Agent at the end (Q, ep, info) and a dict of [launches K, n] arrays -- actions, obs, reward, terminated,
    truncated, reset_call, ep (the counter each step began with) -- and obs0 [n]."""
    from mdp_playground_amd import mdp as mdp_mod
    m = mdp_mod.build_mdp(dict(cfg))
    autoreset, max_steps = kw.get("autoreset", ref.SAME_STEP), kw.get("max_episode_steps", 0)
    envs = cl.make_oracles(m, n, philox_seed, off)
    s = np.array([o.reset() for o in envs], np.int64)
    Q = np.zeros((n, 2, m.S, m.A) if algo == "double_q" else (n, m.S, m.A), np.float32)
    agent = sref.Agent(algo, n, alpha, gamma, epsilon, sched, Q, autoreset)
    total = launches * K
    w = {st: ref.tick_words(seed, off, 0, total + 1, n, st) for st in (ref.EXPLORE_STREAM, ref.ACTION_STREAM, ref.UPDATE_STREAM)}
    steps = np.zeros(n, np.int64)
    traj = {k: np.zeros((total, n), dt) for k, dt in (("actions", np.int64), ("obs", np.int64), ("reward", np.float32), ("terminated", bool),
                                                       ("truncated", bool), ("reset_call", bool), ("ep", np.int64))}
    traj["obs0"] = s.copy()
    for t in range(total):
        if t % K == 0:
            agent.launch_start()
        pending = agent.pending.copy()
        live = ~pending
        traj["ep"][t] = agent.ep
        a = agent.act(s, w[ref.EXPLORE_STREAM][t], w[ref.ACTION_STREAM][t])
        s2, r, te = s.copy(), np.zeros(n, np.float32), np.zeros(n, bool)
        for i in np.flatnonzero(live):
            o, rr, d = envs[i].step(int(a[i]))
            s2[i], r[i], te[i] = o, np.float32(rr), d
        steps[live] += 1
        tr = live & (max_steps > 0) & (steps >= max_steps)
        agent.learn(s, a, r, s2, te, tr, w[ref.EXPLORE_STREAM][t + 1], w[ref.ACTION_STREAM][t + 1], w[ref.UPDATE_STREAM][t])
        ended = live & (te | tr)
        for i in np.flatnonzero(pending | (ended & (autoreset == ref.SAME_STEP))):
            s2[i] = envs[i].reset(explicit=False)
            steps[i] = 0
        for k, v in (("actions", a), ("obs", s2), ("reward", r), ("terminated", te), ("truncated", tr), ("reset_call", pending)):
            traj[k][t] = v
        s = s2
    return agent, traj
