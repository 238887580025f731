"""The yardstick of the learners' per-episode epsilon / alpha schedules (RLToyVectorEnv.set_learner_schedule; include/mdpp.h
"Schedules"): tests/learner_sweep_ref.py's select() and update() with E and alpha recomputed at every step from
(row, ep).  It imports nothing from the product.

A schedule has an epsilon table, an alpha table or both, float [R, M]; env i (the handle's LOCAL index) follows row[i] and
owns a counter ep[i], zero when the schedule is set.  With e = min(ep[i], M - 1):
    E     = ceil(float64(float32(eps[row[i]][e])) 2^31)   if epsilon is scheduled, else the env's own E
    alpha = float32(alpha[row[i]][e])                      if alpha is scheduled, else the env's own alpha
Every selection of a step -- its action, and sarsa's a' = sel(s', t + 1) inside the target -- uses the E in force at the
step's start, the update that alpha.  AFTER the update of a step that is not the reset call of a next-step-autoreset env:
terminated or truncated moves ep by one and both are looked up again.  A reset call selects with the current E, writes the
action, and counts nothing.  With autoreset disabled truncated stays set past max_episode_steps: the counter moves at every
step.  A sarsa action carried over a boundary was chosen under the old E.

Agent is one learner per env driven a step at a time (act, then learn); run() feeds it one launch's own outputs like
learner_sweep_ref.run, tests/learner_schedule_cpu.py drives it against oracle envs.  What it counts keeps a pass honest:
    E_changes / alpha_changes              steps after which an env's E / alpha differed from the one the step began with
    sel_before_env / expl_before_env       fresh selections (and those that explored) made while ep < M - 1, per env
    sel_last_env / expl_last_env           ... made while ep >= M - 1
    carried_old_E / carried_old_E_differs  sarsa actions taken that were chosen under another E than the step's / and that a
                                           fresh selection under the step's E would not have taken
    reset_calls                            reset calls (selected, ignored, not counted)
besides learner_sweep_ref.new_info's own."""
import numpy as np

import learner_sweep_ref as ref

DISABLED, SAME_STEP, NEXT_STEP = ref.DISABLED, ref.SAME_STEP, ref.NEXT_STEP


class Schedule:
    def __init__(self, n, epsilon=None, alpha=None, row=None):
        assert epsilon is not None or alpha is not None
        tabs = [None if t is None else np.atleast_2d(np.asarray(t)) for t in (epsilon, alpha)]
        self.R, self.M = next(t for t in tabs if t is not None).shape
        assert all(t is None or t.shape == (self.R, self.M) for t in tabs)
        self.T = None if tabs[0] is None else ref.epsilon_threshold(tabs[0])        # int64 [R, M]
        self.A = None if tabs[1] is None else tabs[1].astype(np.float32)
        self.row = np.zeros(n, np.int64) if row is None else np.asarray(row).astype(np.int64)
        assert self.row.shape == (n,) and self.row.min() >= 0 and self.row.max() < self.R

    def current(self, ep, E0, alpha0):
        """(E int64 [n], alpha float32 [n]) in force at counters ep"""
        e = np.minimum(ep, self.M - 1)
        E = E0 if self.T is None else self.T[self.row, e]
        al = alpha0 if self.A is None else self.A[self.row, e]
        return E, al


def new_info(n):
    z = lambda: np.zeros(n, np.int64)
    return dict(ref.new_info(n), E_changes=0, alpha_changes=0, sel_before_env=z(), expl_before_env=z(), sel_last_env=z(), expl_last_env=z(),
                carried_old_E=0, carried_old_E_differs=0, reset_calls=0)


class Agent:
    """n scheduled learners.  sched None: the unscheduled learner of learner_sweep_ref (ep still counts episodes)."""

    def __init__(self, algo, n, alpha, gamma, epsilon, sched, Q, autoreset, ep=None, pending=None):
        assert algo in ref.ALGOS and Q.dtype == np.float32
        self.algo, self.n, self.sched, self.autoreset = algo, n, sched, autoreset
        self.al0, self.ga, self.E0 = ref.per_env(n, alpha, gamma, epsilon)
        self.Q = Q.copy()
        self.ep = np.zeros(n, np.int64) if ep is None else np.asarray(ep).astype(np.int64).copy()
        self.pending = np.zeros(n, bool) if pending is None else np.asarray(pending, bool).copy()
        self.have_carry, self.carry, self.carry_E = np.zeros(n, bool), np.zeros(n, np.int64), np.zeros(n, np.int64)
        self.dropped = np.zeros(n, bool)
        self.info = new_info(n)

    def current(self):
        return (self.E0, self.al0) if self.sched is None else self.sched.current(self.ep, self.E0, self.al0)

    def launch_start(self):
        self.have_carry[:] = False              # (a launch's first step selects afresh)
        self.dropped[:] = False

    def act(self, s, w_e, w_a):
        """the step's actions [n] from states s; the step's E and alpha are fixed here"""
        info = self.info
        self.E_step, self.al_step = self.current()
        fresh_mask = ~self.have_carry
        fresh, explored = ref.select(self.algo, self.Q, s, w_e, w_a, self.E_step, info, fresh_mask)
        last = self.ep >= (self.sched.M - 1 if self.sched is not None else 0)
        info["sel_before_env"] += fresh_mask & ~last
        info["expl_before_env"] += fresh_mask & ~last & explored
        info["sel_last_env"] += fresh_mask & last
        info["expl_last_env"] += fresh_mask & last & explored
        old = self.have_carry & (self.carry_E != self.E_step)
        info["carried_old_E"] += int(old.sum())
        info["carried_old_E_differs"] += int((old & (self.carry != fresh)).sum())
        info["trunc_carry_differs"] += int((self.dropped & (self.carry != fresh)).sum())
        info["carried"] += int(self.have_carry.sum())
        info["carried_differs"] += int((self.have_carry & (self.carry != fresh)).sum())
        info["reset_calls"] += int(self.pending.sum())
        return np.where(self.have_carry, self.carry, fresh)

    def learn(self, s, a, r, s2, te, tr, w_e1, w_a1, w_u):
        """after the env's step: update, carry, count.  s2: the true next states; w_e1, w_a1: the words of tick t + 1"""
        info, sarsa = self.info, self.algo == "sarsa"
        te, tr = np.asarray(te, bool), np.asarray(tr, bool)
        live = ~self.pending                    # (a reset call: nothing is learnt, nothing is counted)
        a2 = ref.select(self.algo, self.Q, s2, w_e1, w_a1, self.E_step)[0] if sarsa else np.zeros(self.n, np.int64)
        ref.update(self.algo, self.Q, s, a, r, s2, te, live, self.al_step, self.ga, w_u, a2, info)
        cut = live & ~te & tr & (self.autoreset != DISABLED)
        info["trunc_resets"] += int(cut.sum())
        self.have_carry = live & sarsa & ~te & ~cut
        self.dropped = cut & sarsa
        self.carry, self.carry_E = a2, np.asarray(self.E_step).copy()
        ended = live & (te | tr)
        self.ep = self.ep + ended
        E2, al2 = self.current()
        info["E_changes"] += int((E2 != self.E_step).sum())
        info["alpha_changes"] += int((al2 != self.al_step).sum())
        self.pending = ended & (self.autoreset == NEXT_STEP)


def run(agent, obs_before, obs, reward, terminated, truncated, P, w_e, w_a, w_u=None):
    """One launch of K steps of `agent` (it moves on) fed with the launch's own outputs, as learner_sweep_ref.run is: obs_before
    [N]; obs, reward, terminated, truncated [K, N]; P [S, A]; w_e, w_a uint32 [K + 1, N]; w_u [>= K, N].  Returns the actions
    int64 [K, N]."""
    K, n = obs.shape
    s = np.asarray(obs_before).astype(np.int64)
    actions = np.zeros((K, n), np.int64)
    agent.launch_start()
    for k in range(K):
        a = actions[k] = agent.act(s, w_e[k], w_a[k])
        te, tr = np.asarray(terminated[k], bool), np.asarray(truncated[k], bool)
        s2 = np.asarray(obs[k]).astype(np.int64)
        if agent.autoreset == SAME_STEP:
            s2 = np.where(te | tr, P[s, a], s2)
        agent.learn(s, a, reward[k], s2, te, tr, w_e[k + 1], w_a[k + 1], None if w_u is None else w_u[k])
        s = np.asarray(obs[k]).astype(np.int64)
    return actions
