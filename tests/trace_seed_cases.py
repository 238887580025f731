"""What tests/test_gpu_trace_seeds.py runs -- eligibility traces on ONE MDP PER ENV, RLToyVectorEnv(seeds=[...]) with
set_learner(..., per_env_mdp=True) and set_learner_traces(..., per_env_mdp=True) -- and what it asserts about
its own coverage, shared with tests/test_trace_seed_cases_host.py, which shows on the CPU that those counts are met by every
case before any GPU run.

The set-up is tests/per_env_mdp_cpu.py's: N = 320 envs (one full workgroup and 64 lanes of a second) on seeds 100 ... 419,
env_id_offset 1000, K = 37, two launches.  The CPU closed loop below is that file's loop -- env i the oracle env of
mdp.build_mdp({**cfg, "seed": seeds[i]}) on the Philox streams of global id off + i -- around the agent of
tests/learner_trace_cases.py's loop, tests/learner_trace_ref.TraceAgent, with an optional per-episode schedule.

Cases:
    the main cross      per_env_mdp_cpu.CASES (s8, s8_noise, cfg2, rdist_delay3, s20) x {q_learning, sarsa} x {accumulating,
                        replacing}, the stream mode and uniform / per-env (alpha, gamma, epsilon, lambda) by rotation (form_of)
    truncation          max_episode_steps = 5 under the three autoreset modes, one (algo, kind) each; named as
                        learner_trace_cases names them, so that its honest() applies its exemptions to them
Hyper-parameters are learner_trace_cases.params': ALPHA, GAMMA, EPS, LAMBDA, or the per-env cycles of env i's LOCAL index."""
import numpy as np

import learner_sweep_ref as ref
import learner_trace_cases as cases
import learner_trace_ref as tref
import per_env_mdp_cpu as pm

N, K, LAUNCHES, SEEDS, OFF, SEED, PHILOX_SEED = pm.N, pm.K, pm.LAUNCHES, pm.SEEDS, pm.OFF, pm.SEED, pm.PHILOX_SEED
ALGOS, KINDS, RNGS, FORMS = cases.ALGOS, cases.KINDS, cases.RNGS, cases.FORMS

HANDLES = dict(pm.CASES)
HANDLES.update({
    "s8_max5": (pm._S8, dict(max_episode_steps=5)),
    "s8_next_max5": (pm._S8, dict(autoreset="next_step", max_episode_steps=5)),
    "cfg2_disabled_max5": (pm.CASES["cfg2"][0], dict(autoreset="disabled", max_episode_steps=5)),
})
MAIN = tuple(pm.CASES)
TRUNCATION = (("s8_max5", "q_learning", tref.ACCUMULATING), ("s8_next_max5", "sarsa", tref.REPLACING),
              ("cfg2_disabled_max5", "q_learning", tref.REPLACING))


def form_of(handle, algo, kind):
    """(rng, form) of a case: the four (algo, kind) pairs of a handle take the four (rng, form) pairs, the handles in turn"""
    k = (list(HANDLES).index(handle) + 2 * ALGOS.index(algo) + KINDS.index(kind)) % 4
    return RNGS[k % 2], FORMS[k // 2]


def all_cases():
    """(handle, algo, kind, rng, form) of every case"""
    out = [(h, a, k) + form_of(h, a, k) for h in MAIN for a in ALGOS for k in KINDS]
    return out + [(h, a, k) + form_of(h, a, k) for h, a, k in TRUNCATION]


def closed_loop(cfg, kw, algo, kind, alpha, gamma, epsilon, lam, seeds=SEEDS, *, seed=SEED, K=K, launches=LAUNCHES,
                philox_seed=PHILOX_SEED, off=OFF, sched=None):
    """launches x K steps of len(seeds) oracle envs on Philox streams, env i on the MDP of seeds[i] with the global id off + i,
    under the handle's autoreset / max_episode_steps (kw), learned by a TraceAgent from zero tables.  Returns (agent, traj):
    traj as learner_trace_cases.closed_loop's."""
    mdps = pm.build_mdps(cfg, seeds)
    n, m = len(mdps), mdps[0]
    autoreset, max_steps = kw.get("autoreset", ref.SAME_STEP), kw.get("max_episode_steps", 0)
    envs = [pm.make_oracles(mi, 1, philox_seed, off + i)[0] for i, mi in enumerate(mdps)]
    s = np.array([o.reset() for o in envs], np.int64)
    agent = tref.TraceAgent(algo, n, alpha, gamma, epsilon, lam, kind, np.zeros((n, m.S, m.A), np.float32), autoreset, sched=sched)
    total = launches * K
    w = {st: ref.tick_words(seed, off, 0, total + 1, n, st) for st in (ref.EXPLORE_STREAM, ref.ACTION_STREAM)}
    steps = np.zeros(n, np.int64)
    traj = {k: np.zeros((total, n), dt) for k, dt in (("actions", np.int64), ("obs", np.int64), ("reward", np.float32), ("terminated", bool),
                                                       ("truncated", bool), ("reset_call", bool))}
    traj["obs0"] = s.copy()
    for t in range(total):
        if t % K == 0:
            agent.launch_start()
        pending = agent.pending.copy()
        live = ~pending
        a = agent.act(s, w[ref.EXPLORE_STREAM][t], w[ref.ACTION_STREAM][t])
        s2, r, te = s.copy(), np.zeros(n, np.float32), np.zeros(n, bool)
        for i in np.flatnonzero(live):
            o, rr, d = envs[i].step(int(a[i]))
            s2[i], r[i], te[i] = o, np.float32(rr), d
        steps[live] += 1
        tr = live & (max_steps > 0) & (steps >= max_steps)
        agent.learn(s, a, r, s2, te, tr, w[ref.EXPLORE_STREAM][t + 1], w[ref.ACTION_STREAM][t + 1])
        ended = live & (te | tr)
        for i in np.flatnonzero(pending | (ended & (autoreset == ref.SAME_STEP))):
            if pending[i]:
                # (a next-step reset call takes a tick of its own: per_env_mdp_cpu.closed_loop)
                envs[i].set_philox(philox_seed, off + i, t + 1, 1)
            s2[i] = envs[i].reset(explicit=False)
            steps[i] = 0
        for k, v in (("actions", a), ("obs", s2), ("reward", r), ("terminated", te), ("truncated", tr), ("reset_call", pending)):
            traj[k][t] = v
        s = s2
        if t % K == K - 1:
            agent.info["z_nonzero_at_launch_end"] += int((agent.Z != 0).any())
    return agent, traj


# The sweep schedule with traces: tests/learner_schedule_cases.py's tables (four rows by i % 4, epsilon and alpha both) on
# s8_max5, whose truncation ends an episode every five steps at the latest: 14 - 30 episodes per env in 74 steps, so M = 24
# has envs past the table's end and envs short of it, and alpha changes at episode ends whose Z the sweep left non-zero
SCHED_HANDLE, SCHED_M, SCHED_KIND = "s8_max5", 24, "both"

# The delay comparison across the seeds of the reference's sweep: learner_trace_cases.DELAY_CASE's config without its seed,
# 320 envs on seeds 0 ... 9, 32 each -- env i on seed i // 32 --, ids 0 ... 319, 1 200 steps, q_learning, replacing traces
DELAY_CFG = {k: v for k, v in cases.DELAY_CASE[0].items() if k != "seed"}
DELAY_KW = cases.DELAY_CASE[1]
DELAY_SEEDS = [i // cases.DELAY_ENVS for i in range(10 * cases.DELAY_ENVS)]
