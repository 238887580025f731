"""What tests/test_gpu_linear_history.py and tests/test_gpu_linear_history_search.py run: the handles, their per-env linear
policies with memory (set_linear_policy(theta, history=2)) and the conditions that keep a pass honest.  Shared with
tests/test_linear_history_cases_host.py, which checks on the CPU -- the same closed loop around the oracle -- that every case
meets its conditions, so seeds and gains are settled there.

A case is linear_policy_cases._case's dict (config, kw, D, plds, near, limit, draw, opts) and ``kd``: V is drawn with W's spread
plus kd I (a derivative gain: with W = -g I the policy is a PD controller with kp = g - kd).  ``resets`` is False where the
autoreset mode keeps the step count from ever returning to 0 inside a launch.

The condition on episode boundaries is read per launch: in each of the two launches every wave must see at least 8 steps (k >= 1)
on which some but not all of its lanes form their action with a step count of 0.  In the ``near`` cases (D = 12: no env reaches
the target from a reset state within the launches) the boundaries fall apart because the placed envs terminate at once and then
run their episode limit one step out of phase with the others (limit 7: the placed envs act on a count of 0 at k = 1, 8, 15, ...,
the others at k = 7, 14, ...: 11 such steps in the first launch of 37, 10 in the second); the oracle has no state setter, so for those two cases the
condition can only be asserted where the envs are placed, on the GPU."""
import numpy as np

import linear_policy_cases as lc
import linear_policy_ref as ref
import spill_exposed as sx

N, K, LAUNCHES, OFF = lc.N, lc.K, lc.LAUNCHES, lc.OFF
PHILOX = lc.PHILOX
RNGS = lc.RNGS

D2_ORDER2 = dict(lc._M2P, state_space_dim=2, transition_dynamics_order=2, time_unit=1, target_point=[0, 0], target_radius=0.5,
                 make_denser=True, seed=3)


def _case(config, D, *, kd, resets=True, **kw):
    return dict(lc._case(config, D, **kw), kd=kd, resets=resets)


# (linear_policy_cases.D4_DELAY with the target at the origin, where draw_theta's policies steer: envs reach it at different steps,
#  so episode boundaries fall apart inside every wave)
D4_DELAY = dict(lc.D4_DELAY, target_point=[0, 0, 0, 0])
_MODE9 = dict(max_episode_steps=9)
CASES = {
    "d2_order2": _case(D2_ORDER2, 2, kd=0.8, kw=dict(max_episode_steps=12), limit=True),
    "d2_order2_no_lds": _case(D2_ORDER2, 2, kd=0.8, kw=dict(max_episode_steps=12), limit=True, plds=0, opts=("NO_LINEAR_LDS",)),
    "d3_order2_rel20_box": _case(lc.D3_BOX, 3, kd=0.5, kw=dict(max_episode_steps=20), limit=True),
    "d4_delay3_every2": _case(D4_DELAY, 4, kd=0.3, kw=dict(max_episode_steps=9), limit=True, plds=None),
    "d4_delay3_every2_no_lds": _case(D4_DELAY, 4, kd=0.3, kw=dict(max_episode_steps=9), limit=True, plds=0, opts=("NO_LINEAR_LDS",)),
    "d12_order1": _case(lc.CFG3, 12, kd=0.3, kw=dict(max_episode_steps=7), limit=True, plds=0, near=8, draw=lc._SMALL_BIAS),
    "d12_order2_noise": _case(lc.CFG5, 12, kd=0.5, kw=dict(max_episode_steps=7), limit=True, plds=0, near=8, draw=lc._SMALL_BIAS),
    "autoreset_same_step": _case(lc.D2_MODE, 2, kd=0.4, kw=dict(autoreset="same_step", **_MODE9), limit=True),
    "autoreset_next_step": _case(lc.D2_MODE, 2, kd=0.4, kw=dict(autoreset="next_step", **_MODE9), limit=True),
    "autoreset_disabled": _case(lc.D2_MODE, 2, kd=0.4, kw=dict(autoreset="disabled", **_MODE9), limit=True, resets=False),
}


def theta_of(name, n=N):
    """[n, D, 2 D + 1]: draw_theta's W and b, and V uniform with W's spread plus kd I."""
    c = CASES[name]
    D = c["D"]
    seed = 300 + sorted(CASES).index(name.replace("_no_lds", ""))
    wb = ref.draw_theta(n, D, seed, **c["draw"])
    spread = c["draw"].get("spread", 0.3)
    v = np.random.default_rng(seed + 5000).uniform(-spread, spread, (n, D, D))
    v[:, np.arange(D), np.arange(D)] += c["kd"]
    th = np.zeros((n, D, 2 * D + 1), np.float32)
    th[:, :, :D] = wb[:, :, :D]
    th[:, :, D:2 * D] = v.astype(np.float32)
    th[:, :, 2 * D] = wb[:, :, D]
    return th


def without_v(theta):
    """The history = 1 policy with the same W and b: [.., D, D + 1]."""
    D = theta.shape[-2]
    return np.ascontiguousarray(np.concatenate([theta[..., :D], theta[..., 2 * D:]], axis=-1))


def mode_of(name):
    return CASES[name]["kw"].get("autoreset", "same_step")


def conditions(name, theta, launches, amax=1.0, smax=10.0):
    """The figures the honesty conditions are stated on.  launches: per launch (actions, obs, terminated, truncated, o, p, first)
    -- o, p: what the W and V passes read, first: the step count was 0 -- as [K, n, ...] arrays."""
    acts, obs, term, trunc, o, p = (np.concatenate([l[j] for l in launches]) for j in range(6))
    fig = lc.conditions(name, acts, term, trunc, obs, smax=smax, amax=amax)
    no_v = ref.linear_actions(without_v(theta), o, amax)
    fig["v_matters"] = float(np.mean((no_v.view(np.uint32) != acts.view(np.uint32)).any(axis=-1)))
    # steps whose count is 0 INSIDE a launch (k >= 1: k = 0 of the first launch is every lane's), for some but not all lanes of a wave
    n = acts.shape[1]
    if n % 64 == 0:
        per_launch = [sx.divergent_steps([(len(l[6]) - 1, np.asarray(l[6][1:], np.int64))], single=False) for l in launches]
        fig["first_divergent"] = [d.tolist() for d in per_launch]
    # the memory crosses the launch boundary: p != o on the first step of the second launch
    if len(launches) > 1:
        o1, p1 = launches[1][4][0], launches[1][5][0]
        fig["crossing"] = float(np.mean((o1.view(np.uint32) != p1.view(np.uint32)).any(axis=-1)))
    return fig


def assert_conditions(name, fig, terminations=True):
    c = CASES[name]
    assert 0.05 <= fig["clipped"] <= 0.95, (name, fig)
    if terminations:
        assert fig["terminations"] > 0, (name, fig)
    assert fig["on_wall"] > 0, (name, fig)
    if c["limit"]:
        assert fig["truncations"] > 0, (name, fig)
    assert fig["v_matters"] >= 0.5, (name, fig)
    if c["resets"] and terminations and "first_divergent" in fig:
        # in EACH launch, in every wave, at least 8 steps on which some but not all lanes have a step count of 0
        per = np.asarray(fig["first_divergent"])
        assert (per >= 8).all(), (name, fig)
    if "crossing" in fig:
        assert fig["crossing"] > 0.5, (name, fig)


def near_state(name, state, mdp):
    """linear_policy_cases.near_state for this table's cases (that one reads its own table)."""
    c = CASES[name]
    if not c["near"]:
        return state
    st = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in state.items()}
    idx = np.arange(0, st["curr_state"].shape[0], c["near"])
    tgt = np.zeros(c["D"], np.float32)
    tgt[list(mdp.relevant_indices)] = np.asarray(mdp.target_point, np.float32)
    st["curr_state"][idx] = tgt + np.float32(0.004)
    st["state_derivatives"][idx] = 0.0
    st["state_derivatives"][idx, 0, :] = st["curr_state"][idx]
    st["total_transitions_episode"][idx] = 0
    st["reached_terminal"][idx] = False
    return st
