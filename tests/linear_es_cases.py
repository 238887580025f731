"""What tests/test_gpu_linear_es.py runs: handles of tests/linear_policy_cases.py (imported, not edited) with an episode limit, an
ES on each, and the conditions that keep a bit-for-bit pass honest.  Shared with tests/test_linear_es_cases_host.py, which runs
the same closed loop around the oracle on the CPU, so seeds, scales and rates are settled there.

A case: ``base`` (the case of linear_policy_cases.CASES whose config, policy draw and PLDS it takes), ``kw`` (constructor keywords
that replace the base's: the episode limit), ``T`` (episodes_per_member), ``sigma`` and ``lr`` (group g gets sigma times
1 + g / 4 and lr times 1 + g / 2: every group of a handle has its own scale and gain), ``ties`` (the rewards are sparse: equal scores must occur),
``waits`` (False: no member can ever wait, see the case), ``near`` (every ``near``-th env starts next to the target, through the state setter: a config whose envs only ever truncate ends
every member's episode at the same step, so nobody waits and nobody runs a spare episode; the placed envs terminate early)."""
import numpy as np

import linear_policy_cases as lc

N, K, LAUNCHES, OFF = lc.N, lc.K, 3, lc.OFF
GROUP = 64
G = N // GROUP
SEED = 11
ROWS = 6                # log_generations: fewer than the generations most cases run, so the `gen < M` bound is crossed
RNGS = lc.RNGS
F32 = np.float32


def _case(base, limit, T, sigma, lr, ties=False, near=0, waits=True, kw=None):
    b = lc.CASES[base]
    k = dict(b["kw"], max_episode_steps=limit, **(kw or {}))
    return dict(base=base, config=b["config"], D=b["D"], kw=k, plds=b["plds"], opts=b["opts"], T=T, sigma=sigma, lr=lr, ties=ties,
                near=near, waits=waits)


CASES = {
    "c_d2_n0": _case("c_d2_n0", 7, 1, 0.3, 0.5),
    "c_d2_n0_no_lds_T2": _case("c_d2_n0_no_lds", 7, 2, 0.3, 0.5),
    "d3_order2_rel20_box_sparse": _case("d3_order2_rel20_box", 6, 1, 0.3, 0.5, ties=True),
    "d4_delay3_every2_alw": _case("d4_delay3_every2_alw", 5, 1, 0.2, 0.3),
    "cfg3": _case("cfg3", 4, 1, 0.05, 0.1, near=8),
    "cfg5_T2": _case("cfg5", 4, 2, 0.05, 0.1, near=8),
    "autoreset_same_step": _case("autoreset_same_step", 9, 1, 0.3, 0.5),
    "autoreset_next_step": _case("autoreset_next_step", 5, 1, 0.3, 0.5),
    # (autoreset disabled: after step 5 every step is truncated and is an episode of its own.  A generation then ends at a step at
    #  which EVERY member ends an episode, so nobody ever waits -- by construction, on the GPU too; spare episodes happen)
    "max5_autoreset_disabled_T3": _case("max5_autoreset_disabled", 5, 3, 0.3, 0.5, waits=False),
}

# The sanity check that the strategy optimises: c_d2_n0 (make_denser), one group, the start mean zero (the envs do not move:
# an episode returns 0), every generation logged.  The mean of the last five log_mean rows exceeds the mean of the first five.
OPT = dict(base="c_d2_n0", limit=8, T=1, sigma=0.3, lr=0.6, seed=3, steps=192, rows=12)


def theta_of(name, n=N):
    """the per-env parameters the handle holds before the ES is made (they only fix the per-env layout: init overwrites them)"""
    return lc.theta_of(CASES[name]["base"], n)


def mean_of(name, groups=G):
    """the start means, float32 [groups, D, D + 1]: the base case's draw for the first env of each group"""
    return np.ascontiguousarray(lc.theta_of(CASES[name]["base"], N)[::GROUP][:groups])


def _per_group(v, groups, step=4):
    return (F32(v) * (F32(1) + np.arange(groups, dtype=F32) / F32(step))).astype(F32)


def sigma_of(name, groups=G):
    return _per_group(CASES[name]["sigma"], groups)


def lr_of(name, groups=G):
    return _per_group(CASES[name]["lr"], groups, 2)


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


def figures(ended, gen, info, launch_len=K):
    """The figures the conditions are stated on: ended bool [steps, groups] (where a generation ended), gen int [groups] after the
    run, info: linear_es_ref.new_info() filled by the run."""
    ended = np.asarray(ended, bool)
    steps = ended.shape[0]
    last = [b - 1 for b in range(launch_len, steps + 1, launch_len)]
    mid = int(np.delete(ended, last, axis=0).sum())
    # a launch boundary inside a generation: a group whose generation did not end at the launch's last step
    open_at_boundary = int(sum((~ended[b]).sum() for b in last[:-1]))
    return dict(info, min_gen=int(np.min(gen)), max_gen=int(np.max(gen)), mid_launch=mid, open_at_boundary=open_at_boundary)


def assert_figures(name, fig, staggered=True):
    """staggered: the members' episodes end at different steps (False: a ``near`` case on the oracle, which has no state setter)"""
    assert fig["min_gen"] >= 2, (name, fig)
    assert fig["mid_launch"] > 0 and fig["open_at_boundary"] > 0, (name, fig)
    if staggered and not CASES[name]["waits"]:
        assert fig["waiting"] == 0 and fig["spare"] > 0, (name, fig)
    elif staggered:
        assert fig["waiting"] > 0 and fig["spare"] > 0, (name, fig)
    else:
        assert fig["waiting"] == 0 and fig["spare"] == 0, (name, fig)
    assert fig["non_ties"] > 0, (name, fig)
    if CASES[name]["ties"]:
        assert fig["ties"] > 0, (name, fig)
    assert fig["mean_moved"] > 0 and fig["fma_differs"] > 0, (name, fig)
