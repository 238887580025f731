"""What tests/test_gpu_noise_seeds.py runs and what it asserts about its own coverage (per-env noise levels on ONE MDP PER ENV:
RLToyVectorEnv(seeds=[...]).set_learner(..., per_env_mdp=True) then set_noise_levels(..., per_env_mdp=True); the NLEV forms of the
closed-loop kernels with PM = 1 / 2), shared with tests/test_noise_seed_host.py, which shows on the CPU that those conditions can
be met before any GPU run.

The set-up is per_env_mdp_cpu's: N = 320 envs (one full workgroup and 64 lanes of a second) on seeds 100 ... 419,
env_id_offset 1000, K = 37 steps, two launches in a row.  The levels are the values of the reference's six noise sweeps
(noise_levels_cases.TN / RN) and cycle by env index i % 7 over seven pairs: the five diagonal pairs (TN[j], RN[j]) and
(0, 25), (0.25, 0) -- each key also with the other at zero.  7 and 64 are coprime, so every wave of 64 holds all seven pairs
and lanes that skip the space-stream draw (p == 0) sit beside lanes that make it.  Seven uniform twins per case keep a GPU
case within a few seconds."""
import dataclasses

import numpy as np

import learner_sweep_ref as ref
import noise_levels_cases as nlc
import per_env_mdp_cpu as pm
from closed_loop_cpu import make_oracles

N, K, LAUNCHES = pm.N, pm.K, pm.LAUNCHES
SEEDS, OFF, PHILOX_SEED, SEED = pm.SEEDS, pm.OFF, pm.PHILOX_SEED, pm.SEED
ALPHA, GAMMA, EPS = pm.ALPHA, pm.GAMMA, pm.EPS
ALGOS = pm.ALGOS
TN, RN = nlc.TN, nlc.RN
PAIRS = tuple(zip(TN, RN)) + ((0.0, 25.0), (0.25, 0.0))
assert len(PAIRS) == 7 and len(set(PAIRS)) == 7
CREATED = nlc.CREATED             # what a handle that is given levels is created with: both keys, transition_noise > 0

# (no "seed" key: the handle's seeds=[...] give it, env by env)
TABULAR = pm.CASES["s8"][0]
CFG2 = pm.CASES["cfg2"][0]
RDIST = pm.CASES["rdist_delay3"][0]
S20 = pm.CASES["s20"][0]
# five levels of [29][29] float64 cdfs are 33 640 B: beyond the 32 KiB the cdfs may take in LDS, they stay in global memory
S29 = dict(pm._D, state_space_size=29, action_space_size=29, delay=0, sequence_length=1)
assert 5 * 29 * 29 * 8 == 33640 > 32 * 1024 >= 5 * 20 * 20 * 8

_ALL = tuple((a, r) for a in ALGOS for r in ("numpy", "philox"))
# case -> (config without noise keys, handle keywords, the (algo, rng) pairs the twin rule runs over, steps per launch)
# K is raised for a case, never a floor lowered, where test_noise_seed_host.py finds a floor out of reach at 37
CASES = {
    "tabular": (TABULAR, {}, _ALL, K),
    "cfg2": (CFG2, {}, (("q_learning", "numpy"), ("sarsa", "philox")), K),
    "rdist_delay3": (RDIST, {}, (("double_q", "numpy"), ("sarsa", "philox")), K),              # valued rewards: PM=1, the key ring
    "s20": (S20, {}, (("q_learning", "numpy"), ("double_q", "philox")), K),                     # QLDS=0
    "s29": (S29, {}, (("sarsa", "numpy"),), K),                                                 # ... and the cdfs in global memory by size
    "cfg2_next_step": (CFG2, dict(autoreset="next_step"), (("sarsa", "numpy"),), K),
    "cfg2_disabled_max5": (CFG2, dict(autoreset="disabled", max_episode_steps=5), (("double_q", "philox"),), K),
}
TWIN_PARAMS = [(c, a, r) for c, (_, _, pairs, _) in CASES.items() for a, r in pairs]
# floors on a result: (envs with non-zero Q in all, ... in each workgroup's lanes, envs that terminate at least once).  Noise
# only adds non-zero rewards and moves states about, so per_env_mdp_cpu's floors for the noise-free shapes are kept where the
# shape is the same; under "disabled" with max_episode_steps=5 an env stops after five steps: it terminates or it does not
FLOORS = {"tabular": (280, 32, N), "cfg2": (48, 8, N), "rdist_delay3": (120, 8, N), "s20": (280, 32, 300), "s29": (280, 32, 280),
          "cfg2_next_step": (48, 8, N), "cfg2_disabled_max5": (48, 8, 40)}


def level_arrays(n, lo=0):
    """(transition_noise, reward_noise) float64 [n] of envs lo ... lo + n - 1"""
    i = np.arange(lo, lo + n) % 7
    return np.asarray([p for p, _ in PAIRS])[i], np.asarray([s for _, s in PAIRS])[i]


def mixed_cfg(cfg):
    return dict(cfg, **CREATED)


def twin_cfg(cfg, p, sigma):
    """the config of the uniform handle env i of a mixed handle must equal: created at (p, sigma), everything else equal
    (p == 0: the library sees no transition_noise key)"""
    return nlc.twin_cfg(cfg, p, sigma)


def pairs_present(tn, rn):
    return nlc.pairs_present(tn, rn)


def level_mdps(cfg, tn, rn, seeds=SEEDS):
    """the MDP of every env at its own level: the tables of seed seeds[i] (noise keys do not enter their generation:
    tests/test_noise_seed_host.py checks it) with env i's two values"""
    return [dataclasses.replace(m, transition_noise=float(p), reward_noise=float(s)) for m, p, s in zip(pm.build_mdps(cfg, seeds), tn, rn)]


def tables(cfg, seeds=SEEDS):
    """(P int64 [n, S, A], per env the float32 values its noise-free reward can take)"""
    mdps = pm.build_mdps(cfg, seeds)
    P = np.stack([np.asarray(m.P) for m in mdps])
    values = [np.unique(np.concatenate([[0.0], m.reward_table()]).astype(np.float32)) for m in mdps]
    return P, values


def closed_loop(cfg, kw, algo, tn, rn, alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seeds=SEEDS, *, seed=SEED, K=K, launches=LAUNCHES,
                philox_seed=PHILOX_SEED, off=OFF):
    """per_env_mdp_cpu.closed_loop -- one oracle env per seed on the Philox streams of global id off + i, driven by the
    learner's restatement -- with env i at ITS level (tn[i], rn[i]); traj also holds state (acted from) and next_state (the
    true one), as closed_loop_cpu.closed_loop's does"""
    mdps = level_mdps(cfg, tn, rn, seeds)
    n, m = len(mdps), mdps[0]
    autoreset, max_steps = kw.get("autoreset", ref.SAME_STEP), kw.get("max_episode_steps", 0)
    envs = [make_oracles(mi, 1, philox_seed, off + i)[0] for i, mi in enumerate(mdps)]
    s = np.array([o.reset() for o in envs], np.int64)
    al, ga, E = ref.per_env(n, alpha, gamma, epsilon)
    Q = np.zeros((n, 2, m.S, m.A) if algo == "double_q" else (n, m.S, m.A), np.float32)
    pending, steps = np.zeros(n, bool), np.zeros(n, np.int64)
    info = ref.new_info(n)
    total = launches * K
    w = {st: ref.tick_words(seed, off, 0, total + 1, n, st) for st in (ref.EXPLORE_STREAM, ref.ACTION_STREAM, ref.UPDATE_STREAM)}
    have_carry, carry = np.zeros(n, bool), np.zeros(n, np.int64)
    traj = {k: np.zeros((total, n), dt) for k, dt in (("actions", np.int64), ("obs", np.int64), ("reward", np.float32), ("terminated", bool),
                                                       ("truncated", bool), ("reset_call", bool), ("state", np.int64), ("next_state", np.int64))}
    traj["obs0"] = s.copy()
    for t in range(total):
        live = ~pending
        if t % K == 0:
            have_carry[:] = False                        # (a launch's first step selects afresh)
        fresh, _ = ref.select(algo, Q, s, w[ref.EXPLORE_STREAM][t], w[ref.ACTION_STREAM][t], E, info, ~have_carry)
        a = np.where(have_carry, carry, fresh)
        info["carried"] += int(have_carry.sum())
        info["carried_differs"] += int((have_carry & (carry != fresh)).sum())
        s2, r, te = s.copy(), np.zeros(n, np.float32), np.zeros(n, bool)
        for i in np.flatnonzero(live):
            o, rr, d = envs[i].step(int(a[i]))
            s2[i], r[i], te[i] = o, np.float32(rr), d
        steps[live] += 1
        tr = live & (max_steps > 0) & (steps >= max_steps)
        traj["state"][t], traj["next_state"][t] = s, s2
        a2 = ref.select(algo, Q, s2, w[ref.EXPLORE_STREAM][t + 1], w[ref.ACTION_STREAM][t + 1], E)[0] if algo == "sarsa" else None
        ref.update(algo, Q, s, a, r, s2, te, live, al, ga, w[ref.UPDATE_STREAM][t], a2, info)
        cut = live & ~te & tr & (autoreset != ref.DISABLED)
        have_carry = live & (algo == "sarsa") & ~te & ~cut
        carry = a2 if a2 is not None else carry
        ended = live & (te | tr)
        for i in np.flatnonzero(pending | (ended & (autoreset == ref.SAME_STEP))):
            if pending[i]:
                # (a next-step reset call takes a tick of its own: per_env_mdp_cpu.closed_loop says why)
                envs[i].set_philox(philox_seed, off + i, t + 1, 1)
            s2[i] = envs[i].reset(explicit=False)
            steps[i] = 0
        for k, v in (("actions", a), ("obs", s2), ("reward", r), ("terminated", te), ("truncated", tr), ("reset_call", pending)):
            traj[k][t] = v
        pending = ended & (autoreset == ref.NEXT_STEP)
        s = s2
    return info, Q, traj


def _align16(x):
    return (x + 15) & ~15


LDS_BYTES, ZIG_BYTES = 160 * 1024, 6144      # a workgroup's LDS on gfx950; the NOISE kernels' static ziggurat tables


def placement(cfg, algo, rng, *options, levels=5):
    """(QLDS, PM, cdfs staged, dynamic LDS bytes) by the rule of include/mdpp.h (closed_agent_lds on one MDP per env with levels) restated: the
    Q-tables (at most 160 KiB, not under NO_LEARN_LDS), the MDP slots (at most 64 KiB, not under NO_PM_LDS) and the per-level
    cdfs (at most 32 KiB, numpy streams only, not under NO_PM_NLEV_LDS) go to LDS in the first of the subsets {Q, slots, cdfs},
    {Q, slots}, {Q, cdfs}, {Q}, {slots, cdfs}, {slots}, {cdfs}, {} that fits beside the 6 KiB of ziggurat tables.  A lane's slot
    is its carve: P, terminal flags, start cdf, reward bits or rewards, each rounded up to 16 bytes."""
    S, A, L = cfg["state_space_size"], cfg["action_space_size"], cfg["sequence_length"]
    rew = 8 * S ** L if "reward_dist" in cfg else (S ** L + 7) // 8
    slots = 256 * (_align16(S * A) + _align16(S) + _align16(8 * S) + _align16(rew))
    q = 256 * S * A * 4 * (2 if algo == "double_q" else 1)
    cdf = _align16(levels * S * S * 8)
    ok = dict(q=q <= LDS_BYTES and "NO_LEARN_LDS" not in options, m=slots <= 64 * 1024 and "NO_PM_LDS" not in options,
              c=rng == "numpy" and cdf <= 32 * 1024 and "NO_PM_NLEV_LDS" not in options)
    size = dict(q=q, m=slots, c=cdf)
    for subset in ("qmc", "qm", "qc", "q", "mc", "m", "c", ""):
        total = sum(size[k] for k in subset)
        if all(ok[k] for k in subset) and ZIG_BYTES + total <= LDS_BYTES:
            return int("q" in subset), 2 if "m" in subset else 1, "c" in subset, total
    raise AssertionError("the empty subset always fits")


def kernel_name(kind, cfg, algo, rng, qlds, pmv, summary=False):
    """the name the library reports: the template arguments in template order"""
    dbl, head = algo == "double_q", "PHILOX=%d,NOISE=1,UNIT=%d,QLDS=%d" % (rng == "philox", "reward_dist" not in cfg, qlds)
    stem = "summary" if summary else "rollout"
    if kind == "learn":
        return "k_discrete_learn_%s<%s,PE=1%s,NLEV=1,PM=%d>" % (stem, head, ",DOUBLE=1" if dbl else "", pmv)
    return "k_discrete_eval_%s<%s,DOUBLE=%d,NLEV=1,PM=%d>" % (stem, head, dbl, pmv)


def check_floors(case, Q, terminated, what=""):
    """the conditions of FLOORS on a result (Q [n, ...], terminated bool [steps, n]); returns the counts"""
    total, per_wg, term_floor = FLOORS[case]
    nz = pm.nonzero_envs(Q)
    counts = (int(nz.sum()), int(nz[:256].sum()), int(nz[256:].sum()), int(np.asarray(terminated).any(axis=0).sum()))
    assert counts[0] >= total and counts[1] >= per_wg and counts[2] >= per_wg and counts[3] >= term_floor, (what, case, counts)
    return counts


def honest(tn, rn, state, action, next_state, reward, terminated, explored_env, P, values, live):
    """What a pass over mixed levels on one MDP per env must have exercised -- noise_levels_cases.honest restated for per-env
    P.  tn, rn [n]: the envs' levels; state, action, next_state, reward, terminated [T, n]: every step's state acted from,
    action, TRUE next state, float32 reward and flag; live [T, n]: the step is a step of the env (not a reset call);
    explored_env [n]: exploring selections per env; P [n, S, A]; values: per env the float32 values its own MDP's noise-free
    reward takes."""
    n = len(tn)
    noisy = live & (next_state != P[np.arange(n)[None, :], state, action])
    for p in sorted(set(TN)):
        at = tn == p
        assert at.any()
        if p == 0.0:
            assert not noisy[:, at].any(), "level 0 made a noisy transition"
        else:
            assert noisy[:, at].any(), ("no noisy transition at level", p)
        assert terminated[:, at].any(), ("no termination at level", p)
        assert (explored_env[at] > 0).any(), ("no explored step at level", p)
    # sigma = 0 envs pay only values of their OWN MDP's reward table; the mean |reward| grows strictly with sigma
    spread = []
    for s in sorted(set(RN)):
        at = np.flatnonzero(rn == s)
        assert len(at)
        if s == 0.0:
            for i in at:
                paid = np.unique(reward[:, i][live[:, i]])
                assert np.isin(paid, values[i]).all(), ("env of sigma 0 paid a value that is not its MDP's", i, paid, values[i])
        else:
            assert len(np.unique(reward[:, at][live[:, at]])) > 100
        spread.append(np.abs(reward[:, at][live[:, at]].astype(np.float64)).mean())
    assert all(a < b for a, b in zip(spread, spread[1:])), spread
