"""The closed loop on the CPU: n oracle envs (oracle.DiscreteOracle on Philox streams) driven step by step by the learner's
restatement tests/learner_sweep_ref.py.  It predicts a whole learning launch without a GPU -- also where the launch's own
outputs do not tell the restatement enough (truncation, noise and same-step autoreset together: learn() sees a next state
that appears in no output) -- and it shows on the CPU that the coverage a GPU test asserts about itself can be met.
Shared by tests/test_learner_sweep_host.py, tests/test_closed_loop_shapes_host.py and tests/test_gpu_closed_loop_shapes.py."""
import numpy as np

import learner_sweep_ref as ref


def make_oracles(m, n, philox_seed=77, off=0):
    """n oracle envs of the MDP m (mdp.build_mdp's) on the Philox streams of global env ids off ... off + n - 1"""
    from oracle import oracle as ora
    custom = m.reward_matrix is not None
    table = np.zeros(m.S ** m.sequence_length) if custom else m.reward_table()
    envs = []
    for i in range(n):
        o = ora.DiscreteOracle(m.S, m.A, m.sequence_length, m.delay, m.reward_every_n_steps, m.P, table, m.terminal_states,
                               m.init_dist, m.transition_noise, m.reward_noise, m.reward_scale, m.reward_shift, m.term_state_reward)
        if custom:
            o.set_reward_matrix(m.reward_matrix)
        o.set_philox(philox_seed, off + i)
        envs.append(o)
    return envs


def closed_loop(cfg, kw, algo, alpha, gamma, epsilon, n, q0=None, *, seed, K, launches, philox_seed=77, off=0, greedy=None):
    """launches x K steps of n envs under the handle's autoreset / max_episode_steps (kw), the learner (algo, alpha, gamma,
    epsilon: scalars or arrays [n], its Philox key `seed`) starting from q0 (zeros).  A launch's first step selects afresh.
    greedy: a function (Q, s, live) -> actions replaces the learner (evaluation: nothing is learnt, no word is drawn).
    Returns (info, Q, traj): info as learner_sweep_ref.new_info, traj a dict of [launches K, n] arrays -- actions, obs (as a
    handle returns them: after a same-step reset the next episode's first), reward float32, terminated, truncated, reset_call,
    state (the state acted from), next_state (the true next state, whatever was returned) -- and obs0 [n]."""
    from mdp_playground_amd import mdp as mdp_mod
    m = mdp_mod.build_mdp(dict(cfg))
    autoreset, max_steps = kw.get("autoreset", ref.SAME_STEP), kw.get("max_episode_steps", 0)
    envs = make_oracles(m, n, philox_seed, off)
    s = np.array([o.reset() for o in envs], np.int64)
    al, ga, E = ref.per_env(n, alpha, gamma, epsilon)
    Q = (np.zeros((n, 2, m.S, m.A) if algo == "double_q" else (n, m.S, m.A), np.float32) if q0 is None else q0.copy())
    pending, steps = np.zeros(n, bool), np.zeros(n, np.int64)
    info = ref.new_info(n)
    total = launches * K
    w = None if greedy else {st: ref.tick_words(seed, off, 0, total + 1, n, st) for st in (ref.EXPLORE_STREAM, ref.ACTION_STREAM, ref.UPDATE_STREAM)}
    have_carry, carry = np.zeros(n, bool), np.zeros(n, np.int64)
    dropped = np.zeros(n, bool)                          # sarsa: the previous step dropped its carry at a truncation
    traj = {k: np.zeros((total, n), dt) for k, dt in (("actions", np.int64), ("obs", np.int64), ("reward", np.float32), ("terminated", bool),
                                                       ("truncated", bool), ("reset_call", bool), ("state", np.int64), ("next_state", np.int64))}
    traj["obs0"] = s.copy()
    for t in range(total):
        live = ~pending
        if greedy:
            a = greedy(Q, s, live)
        else:
            if t % K == 0:
                have_carry[:] = False                        # (a launch's first step selects afresh)
                dropped[:] = False
            fresh, _ = ref.select(algo, Q, s, w[ref.EXPLORE_STREAM][t], w[ref.ACTION_STREAM][t], E, info, ~have_carry)
            info["trunc_carry_differs"] += int((dropped & (carry != fresh)).sum())
            a = np.where(have_carry, carry, fresh)
        s2, r, te = s.copy(), np.zeros(n, np.float32), np.zeros(n, bool)
        for i in np.flatnonzero(live):
            o, rr, d = envs[i].step(int(a[i]))
            s2[i], r[i], te[i] = o, np.float32(rr), d
        steps[live] += 1
        tr = live & (max_steps > 0) & (steps >= max_steps)
        traj["state"][t], traj["next_state"][t] = s, s2
        if not greedy:
            a2 = ref.select(algo, Q, s2, w[ref.EXPLORE_STREAM][t + 1], w[ref.ACTION_STREAM][t + 1], E)[0] if algo == "sarsa" else None
            ref.update(algo, Q, s, a, r, s2, te, live, al, ga, w[ref.UPDATE_STREAM][t], a2, info)
            cut = live & ~te & tr & (autoreset != ref.DISABLED)
            info["trunc_resets"] += int(cut.sum())
            have_carry = live & (algo == "sarsa") & ~te & ~cut
            dropped = cut & (algo == "sarsa")
            carry = a2 if a2 is not None else carry
        ended = live & (te | tr)
        reset_now = pending | (ended & (autoreset == ref.SAME_STEP))
        for i in np.flatnonzero(reset_now):
            s2[i] = envs[i].reset(explicit=False)
            steps[i] = 0
        for k, v in (("actions", a), ("obs", s2), ("reward", r), ("terminated", te), ("truncated", tr), ("reset_call", pending)):
            traj[k][t] = v
        pending = ended & (autoreset == ref.NEXT_STEP)
        s = s2
    return info, Q, traj
