"""What tests/test_gpu_linear_search.py runs: the handles of tests/linear_policy_cases.py (imported, not edited) with an episode
limit, a search on each, and the conditions that keep a bit-for-bit pass honest.  Shared with
tests/test_linear_search_cases_host.py, which runs the same closed loop around the oracle on the CPU, so seeds and step sizes
are settled there.

A search case: ``base`` (the case of linear_policy_cases.CASES whose config, policy draw and PLDS it takes), ``kw`` (constructor
keywords that replace the base's: the episode limit), ``T`` (episodes_per_trial), ``sigma`` (a scalar, or "zeros3": a float32
array that is exactly 0 for every third env), ``up`` / ``down`` / ``sigma_max`` (the success rule), ``near`` (every ``near``-th env
starts next to the target, through the state setter: a config whose envs only ever truncate ends every trial of a wave at the
same step, and the placed envs shift theirs)."""
import numpy as np

import linear_policy_cases as lc

N, K, LAUNCHES, OFF = lc.N, lc.K, 3, lc.OFF
SEED = 5
RNGS = lc.RNGS
F32 = np.float32


def _case(base, limit, T, sigma, up=1.0, down=1.0, sigma_max=np.inf, near=0, kw=None):
    b = lc.CASES[base]
    k = dict(b["kw"], max_episode_steps=limit, **(kw or {}))
    return dict(base=base, config=b["config"], D=b["D"], kw=k, plds=b["plds"], opts=b["opts"], T=T, sigma=sigma, up=up, down=down,
                sigma_max=sigma_max, near=near)


CASES = {
    "c_d2_n0": _case("c_d2_n0", 7, 1, 0.3),
    "c_d2_n0_no_lds": _case("c_d2_n0_no_lds", 7, 1, 0.3),
    "c_d2_n0_sigma_zeros": _case("c_d2_n0", 7, 1, "zeros3"),
    "d3_order2_rel20_box": _case("d3_order2_rel20_box", 6, 2, 0.3, up=1.5, down=0.75, sigma_max=2.0),     # (unclamped, sigma reaches 7.7)
    "d4_delay3_every2_alw": _case("d4_delay3_every2_alw", 5, 1, 0.2, up=1.5, down=0.75, sigma_max=0.4),
    "d4_delay3_every2_alw_no_lds": _case("d4_delay3_every2_alw_no_lds", 5, 1, 0.2, up=1.5, down=0.75, sigma_max=0.4),
    "cfg3": _case("cfg3", 4, 1, 0.05, near=8),
    "cfg5": _case("cfg5", 4, 2, 0.05, near=8),
    "autoreset_same_step": _case("autoreset_same_step", 9, 1, 0.3, up=1.25, down=0.9),
    "autoreset_next_step": _case("autoreset_next_step", 5, 1, 0.3),
    # (autoreset disabled: after step 5 every step is truncated and is an episode of its own.  Trial 0 holds the whole approach, so
    #  short later trials almost never beat it -- 1 % accepted at T = 3, sigma 0.3 on the oracle; 12 % at T = 12, sigma 1.
    #  Not sigma = 1 itself: 1 * z is exact and a fused multiply-add would give the same candidate)
    "max5_autoreset_disabled": _case("max5_autoreset_disabled", 5, 12, 0.9),
}


def theta_of(name, n=N):
    return lc.theta_of(CASES[name]["base"], n)


def sigma_of(name, n=N):
    s = CASES[name]["sigma"]
    if s == "zeros3":
        a = np.full(n, 0.3, F32)
        a[::3] = 0.0
        return a
    return s


def near_state(name, state, mdp):
    """lc.near_state's placement for this case's own ``near``"""
    c = CASES[name]
    if not c["near"]:
        return state
    st = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in state.items()}
    idx = np.arange(0, st["curr_state"].shape[0], c["near"])
    tgt = np.zeros(c["D"], F32)
    tgt[list(mdp.relevant_indices)] = np.asarray(mdp.target_point, F32)
    st["curr_state"][idx] = tgt + F32(0.004)
    st["state_derivatives"][idx] = 0.0
    st["state_derivatives"][idx, 0, :] = st["curr_state"][idx]
    st["total_transitions_episode"][idx] = 0
    st["reached_terminal"][idx] = False
    return st


def figures(ended, trial, accepted, launch_len=K):
    """The figures the conditions are stated on: ended bool [T, n] (where a trial ended), trial and accepted int [n] after the
    run.  Trial 0 is accepted in every case here (no NaN return), so the trials after it count accepted - 1 per env."""
    ended = np.asarray(ended, bool)
    T, n = ended.shape
    trial, accepted = np.asarray(trial, np.int64), np.asarray(accepted, np.int64)
    later = int(np.maximum(trial - 1, 0).sum())
    later_acc = int((accepted - (trial >= 1)).sum())
    mixed = 0
    for w in range(0, n, 64):
        e = ended[:, w:w + 64]
        mixed += int((e.any(1) & ~e.all(1)).sum())
    # a launch boundary inside a trial: an env whose trial did not end at the launch's last step
    open_at_boundary = int(sum((~ended[b - 1]).sum() for b in range(launch_len, T, launch_len)))
    return dict(min_trials=int(trial.min()), max_trials=int(trial.max()), later=later, later_accepted=later_acc,
                later_rejected=later - later_acc, mixed_wave_steps=mixed, open_at_boundary=open_at_boundary)


def assert_figures(name, fig, mixed=True, fraction=0.05):
    assert fig["min_trials"] >= 2, (name, fig)
    assert fig["later_accepted"] >= fraction * fig["later"] and fig["later_accepted"] > 0, (name, fig)
    assert fig["later_rejected"] >= fraction * fig["later"] and fig["later_rejected"] > 0, (name, fig)
    if mixed:
        assert fig["mixed_wave_steps"] > 0, (name, fig)
    assert fig["open_at_boundary"] > 0, (name, fig)
