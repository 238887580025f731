"""The yardstick of a grid handle with per-env noise levels (RLToyVectorEnv.set_grid_noise_levels; include/mdpp.h "Grid noise
levels"): a COMPOSITION, not a new loop.  Env i of a mixed handle equals env i of a handle created uniformly at its pair, so
for each pair the existing restatement -- tests/grid_learner_ref.closed_loop, or tests/grid_schedule_ref.closed_loop under a
schedule; imported, not edited -- runs on the config with that pair and ALL n global env ids, and the columns of the pair's
envs are kept.  It imports nothing from the product but what those two import.

composed(...) returns (infos, Q [n, S, A], traj): infos one dict per pair -- the restatement's own counters over all n envs
of its uniform run, plus, counted on the PAIR'S envs only: redrawn_moves, terminations, truncations, reset_calls,
off_lattice (rewards that no noiseless step of the config can give), explored, greedy --; traj the composed [launches K,
n(, 2)] arrays of grid_learner_ref.closed_loop (and, scheduled, `ep` int64 [n], the composed episode counters)."""
import numpy as np

import grid_learner_ref as gref
import grid_noise_level_cases as nc

_COLUMNS = ("actions", "vectors", "obs", "reward", "terminated", "truncated", "reset_call")


def noiseless_lattice(cfg):
    """float32 values a step of the config can pay without reward noise: (d + [terminal reward]) scale + shift for the dense
    distance gains d in {-2, ..., 2} (an episode's first cell may be the index g, one past the grid: the first move's clip then
    moves both coordinates) or the sparse {0, 1}, and the every-n mask's 0"""
    scale, shift = cfg.get("reward_scale", 1.0), cfg.get("reward_shift", 0.0)
    base = (-2.0, -1.0, 0.0, 1.0, 2.0) if cfg.get("make_denser") else (0.0, 1.0)
    vals = set()
    for b in base:
        for t in (0.0, cfg.get("term_state_reward", 0.0) * scale):
            vals.add(np.float32(b * scale + shift + t))
    return np.array(sorted(vals), np.float32)


def composed(case, algo, n=nc.N, K=nc.K, launches=nc.LAUNCHES, sched=None, greedy=False, q0=None):
    """the case's launches on Philox streams, pair by pair.  sched: a learner_schedule_ref.Schedule (the scheduled learner)."""
    c = nc.CASES[case]
    idx = nc.pair_index(case, n)
    al, ga, ep = c["rates"]
    infos, Q, traj, eps = [], None, None, None
    for j, pair in enumerate(c["pairs"]):
        cfg = nc.uniform_cfg(case, pair)
        common = dict(seed=nc.LEARNER_SEED, K=K, launches=launches, noop=c["noop"], philox_seed=nc.PHILOX_SEED, off=nc.ENV_ID_OFFSET)
        if sched is not None:
            import grid_schedule_ref as gsr
            info, q, e, t = gsr.closed_loop(cfg, c["kw"], algo, al, ga, ep, n, q0, sched, **common)
        else:
            info, q, t = gref.closed_loop(cfg, c["kw"], algo, al, ga, ep, n, q0, greedy=greedy, **common)
            e = None
        mine = idx == j
        if Q is None:
            cols = tuple(k for k in _COLUMNS + ("cell", "next_cell") if k in t)
            Q, traj = q.copy(), {k: t[k].copy() for k in cols + ("obs0",)}
            eps = None if e is None else e.copy()
        Q[mine] = q[mine]
        for k in cols:
            traj[k][:, mine] = t[k][:, mine]
        traj["obs0"][mine] = t["obs0"][mine]
        if e is not None:
            eps[mine] = e[mine]
        live = ~t["reset_call"][:, mine]
        info = dict(info)
        if "next_cell" in t:        # (grid_learner_ref keeps the cells; the scheduled loop counts over all n envs only)
            hi = np.asarray(c["cfg"]["grid_shape"], np.int64) - 1
            expected = np.clip(t["cell"][:, mine] + t["vectors"][:, mine], 0, hi)
            info["redrawn_moves"] = int((live & (expected != t["next_cell"][:, mine]).any(axis=2)).sum())
        info["terminations"] = int((live & t["terminated"][:, mine]).sum())
        info["truncations"] = int((live & t["truncated"][:, mine]).sum())
        info["reset_calls"] = int((~live).sum())
        info["off_lattice"] = int((live & ~np.isin(t["reward"][:, mine], noiseless_lattice(cfg))).sum())
        if "explored_env" in info:
            info["explored"] = int(info["explored_env"][mine].sum())
            info["greedy"] = int((info["selections_env"][mine] - info["explored_env"][mine]).sum())
        infos.append(info)
    if eps is not None:
        traj["ep"] = eps
    return infos, Q, traj


_runs = {}


def cpu_run(case, algo):
    """composed(case, algo) at the cases' N, K and launches, computed once"""
    if (case, algo) not in _runs:
        _runs[case, algo] = composed(case, algo)
    return _runs[case, algo]
