"""The yardstick of the learners' eligibility traces (RLToyVectorEnv.set_learner_traces; include/mdpp.h "Eligibility traces",
DESIGN.md 3.29): SARSA(lambda) and Watkins's Q(lambda), a numpy restatement vectorised over envs, float32 throughout, its
Philox words from the oracle (learner_sweep_ref.tick_words).  It imports nothing from the product.

Everything of tests/learner_ref.py holds -- sel, the step's outputs as inputs, the target y, sarsa's carry, the reset call --
except the update.  Per env, with a second table Z float32 [S, A] beside Q (zeros when traces are set), lambda float32 in
[0, 1] and c = gamma lambda (float32), for a step that is not a reset call, q = Q[s][a] read before anything is written:
    d = y - q;  u = alpha d
    1. cut   (q_learning only) the step's action came from the explore branch of sel ((wE >> 1) < E, whatever it drew): Z = +0
    2. mark  accumulating: Z[s][a] = Z[s][a] + 1;  replacing: Z[s][a] = 1
    3. sweep every entry e: z = Z[e];  Q[e] = Q[e] + u z (the product rounded, then the sum);  Z[e] = c z
    4. end   terminated or truncated (where the summary's `episodes` moves): Z = +0, after the sweep
one rounding per operation, no FMA, denormals kept (numpy flushes nothing).

TraceAgent is learner_schedule_ref.Agent -- selection, carry, pending flags, per-env parameters, the per-episode schedule
and its counters -- with that update; learner_schedule_ref.run feeds it a launch's own outputs.  What it counts keeps a pass
honest:
    cuts / uncut            live q_learning steps that cut / did not cut
    cut_greedy_action       ... that cut although the random action was the greedy one
    above_one               marks that left a trace above 1 (accumulating, a revisit inside an episode)
    ends                    steps after which Z was zeroed
    z_nonzero_at_launch_end launches that ended with some non-zero Z
    denormal_traces         trace entries in the denormal range after a sweep, summed over steps
    alpha_change_with_z     (schedule) episode ends at which the alpha in force changed and Z was non-zero until the rule zeroed it"""
import numpy as np

import learner_schedule_ref as sref
import learner_sweep_ref as ref

ACCUMULATING, REPLACING = "accumulating", "replacing"
KINDS = (ACCUMULATING, REPLACING)
DISABLED, SAME_STEP, NEXT_STEP = ref.DISABLED, ref.SAME_STEP, ref.NEXT_STEP
TINY = np.finfo(np.float32).tiny


class TraceAgent(sref.Agent):
    """n learners with traces.  lam: a scalar or an array [n]; Z (copied) or zeros"""

    def __init__(self, algo, n, alpha, gamma, epsilon, lam, kind, Q, autoreset, sched=None, Z=None, ep=None, pending=None):
        assert algo in ("q_learning", "sarsa") and kind in KINDS
        super().__init__(algo, n, alpha, gamma, epsilon, sched, Q, autoreset, ep=ep, pending=pending)
        self.kind = kind
        self.lam = np.broadcast_to(np.asarray(lam, np.float32), (n,)).copy()
        assert ((self.lam >= 0) & (self.lam <= 1)).all()
        self.Z = np.zeros_like(self.Q) if Z is None else np.asarray(Z).copy()
        assert self.Z.dtype == np.float32 and self.Z.shape == self.Q.shape
        self.explored = np.zeros(n, bool)
        self.info.update(cuts=0, uncut=0, cut_greedy_action=0, above_one=0, ends=0, z_nonzero_at_launch_end=0, denormal_traces=0,
                         alpha_change_with_z=0)

    def act(self, s, w_e, w_a):
        a = super().act(s, w_e, w_a)
        # the explore branch of this tick's sel, under the step's E (read by q_learning's cut: it carries nothing)
        self.explored = (w_e >> np.uint32(1)).astype(np.int64) < self.E_step
        self.greedy_now = ref.scan_best(self.Q[np.arange(self.n), s])[0]
        return a

    def learn(self, s, a, r, s2, te, tr, w_e1, w_a1, w_u=None):
        info, sarsa, n = self.info, self.algo == "sarsa", self.n
        idx = np.arange(n)
        te, tr = np.asarray(te, bool), np.asarray(tr, bool)
        r = np.asarray(r, np.float32)
        live = ~self.pending                    # (a reset call touches neither Q nor Z)
        Q, Z = self.Q, self.Z
        # the target, on Q before anything is written
        a2 = ref.select(self.algo, Q, s2, w_e1, w_a1, self.E_step)[0] if sarsa else np.zeros(n, np.int64)
        qn = Q[idx, s2, a2] if sarsa else ref.scan_best(Q[idx, s2])[1]
        with np.errstate(under="ignore"):
            c = self.ga * self.lam
            g = self.ga * qn
            y = np.where(te, r, r + g).astype(np.float32)
            q = Q[idx, s, a]
            d = y - q
            u = self.al_step * d
        assert c.dtype == g.dtype == y.dtype == d.dtype == u.dtype == np.float32
        # 1. cut
        cut = live & (not sarsa) & self.explored
        Z[cut] = np.float32(0.0)
        info["cuts"] += int(cut.sum())
        info["uncut"] += int((live & (not sarsa) & ~self.explored).sum())
        info["cut_greedy_action"] += int((cut & (a == self.greedy_now)).sum())
        # 2. mark
        L = idx[live]
        if self.kind == ACCUMULATING:
            marked = Z[L, s[live], a[live]] + np.float32(1.0)
        else:
            marked = np.full(L.size, 1.0, np.float32)
        assert marked.dtype == np.float32
        Z[L, s[live], a[live]] = marked
        info["above_one"] += int((marked > 1).sum())
        # 3. sweep
        with np.errstate(under="ignore"):
            uz = u[L, None, None] * Z[L]
            newQ = Q[L] + uz
            newZ = c[L, None, None] * Z[L]
        assert uz.dtype == newQ.dtype == newZ.dtype == np.float32
        Q[L], Z[L] = newQ, newZ
        info["denormal_traces"] += int(((newZ != 0) & (np.abs(newZ) < TINY)).sum())
        info["updates"] += int(live.sum())
        # 4. episode end
        ended = live & (te | tr)
        zlive = (Z[ended] != 0).any(axis=(1, 2)) if ended.any() else np.zeros(0, bool)
        Z[ended] = np.float32(0.0)
        info["ends"] += int(ended.sum())
        # carry, schedule, pending: learner_schedule_ref.Agent.learn's
        dropped = live & ~te & tr & (self.autoreset != DISABLED)
        info["trunc_resets"] += int(dropped.sum())
        self.have_carry = live & sarsa & ~te & ~dropped
        self.dropped = dropped & sarsa
        self.carry, self.carry_E = a2, np.asarray(self.E_step).copy()
        self.ep = self.ep + ended
        E2, al2 = self.current()
        info["E_changes"] += int((E2 != self.E_step).sum())
        changed = np.asarray(al2 != self.al_step) & np.ones(n, bool)
        info["alpha_changes"] += int(changed.sum())
        # (the alpha in force changed at an episode end whose traces were non-zero until the rule zeroed them)
        if ended.any():
            info["alpha_change_with_z"] += int((changed[ended] & zlive).sum())
        self.pending = ended & (self.autoreset == NEXT_STEP)


def run(agent, obs_before, obs, reward, terminated, truncated, P, w_e, w_a):
    """One launch of K steps of `agent` (it moves on) fed with the launch's own outputs: learner_schedule_ref.run.  Returns the
    actions int64 [K, N]."""
    act = sref.run(agent, obs_before, obs, reward, terminated, truncated, P, w_e, w_a)
    agent.info["z_nonzero_at_launch_end"] += int((agent.Z != 0).any())
    return act
