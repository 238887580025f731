"""What tests/test_gpu_linear_rollout.py and tests/test_gpu_linear_summary.py run: the handles, their per-env linear policies
and the conditions that keep a pass honest.  Shared with tests/test_linear_policy_cases_host.py, which checks on the CPU --
the same closed loop around the oracle -- that every case meets its conditions, so seeds and gains are settled there.

A case: config, kw (constructor keywords), D, the policy's draw (linear_policy_ref.draw_theta's arguments), ``plds`` (the
PLDS value the kernel's name must show: 1, 0, or None = whatever the device grants), ``near`` (every ``near``-th env starts the
first launch next to the target with the derivatives at rest, through the state setter: the config itself cannot bring an
env there within the launches) and ``limit`` (the case has a max_episode_steps: truncations must happen)."""
import numpy as np

import linear_policy_ref as ref

N, K, LAUNCHES, OFF = 320, 37, 2, 1000
PHILOX = dict(rng="philox", philox_seed=77)

_M2P = dict(state_space_type="continuous", reward_function="move_to_a_point", state_space_max=10, action_space_max=1, inertia=1)
C_D2_N0 = dict(state_space_type="continuous", action_space_type="continuous", state_space_dim=2, action_space_dim=2,
               transition_dynamics_order=1, inertia=1, time_unit=1.0, state_space_max=10, action_space_max=1,
               target_point=[0, 0], target_radius=0.5, make_denser=True, reward_function="move_to_a_point",
               action_loss_weight=0.01, delay=0, reward_scale=1.0, transition_noise=0, reward_noise=0, seed=0)
_C12 = dict(_M2P, state_space_dim=12, relevant_indices=[0, 1, 2, 3], irrelevant_features=True, target_point=[0, 0, 0, 0],
            target_radius=0.05, make_denser=True)
CFG3 = dict(_C12, transition_dynamics_order=1, time_unit=1, seed=0)
CFG5 = dict(_C12, transition_dynamics_order=2, time_unit=0.1, transition_noise=0.05, reward_noise=0.05, seed=0)
D3_BOX = dict(_M2P, state_space_dim=3, transition_dynamics_order=2, time_unit=0.5, relevant_indices=[2, 0], irrelevant_features=True,
              target_point=[0.5, -0.5], target_radius=0.4, make_denser=False, terminal_states=[[3.0, 3.0], [-4.0, 2.0]],
              term_state_edge=2.0, term_state_reward=-0.5, reward_scale=2.0, reward_shift=0.125, seed=5)
D4_DELAY = dict(_M2P, state_space_dim=4, transition_dynamics_order=1, time_unit=1, target_point=[1, -1, 0.5, 0], target_radius=0.6,
                make_denser=True, delay=3, reward_every_n_steps=2, action_loss_weight=0.25, seed=7)
D2_F64 = dict(_M2P, state_space_dim=2, transition_dynamics_order=1, time_unit=1, target_radius=0.5, make_denser=True, delay=2, seed=9)
D2_MODE = dict(_M2P, state_space_dim=2, transition_dynamics_order=1, time_unit=1, target_point=[0.25, 0.5], target_radius=0.5,
               make_denser=True, reward_noise=0.1, seed=11)


def _case(config, D, *, kw=None, plds=1, near=0, limit=False, draw=None, opts=()):
    return dict(config=config, D=D, kw=dict(kw or {}), plds=plds, near=near, limit=limit, draw=dict(draw or {}), opts=tuple(opts))


_SMALL_BIAS = dict(bias=0.01, spread=0.2)
CASES = {
    "c_d2_n0": _case(C_D2_N0, 2),
    "c_d2_n0_no_lds": _case(C_D2_N0, 2, plds=0, opts=("NO_LINEAR_LDS",)),
    "d3_order2_rel20_box": _case(D3_BOX, 3, kw=dict(max_episode_steps=20), limit=True),
    "d4_delay3_every2_alw": _case(D4_DELAY, 4),
    "d4_delay3_every2_alw_no_lds": _case(D4_DELAY, 4, plds=0, opts=("NO_LINEAR_LDS",)),
    "cfg3": _case(CFG3, 12, plds=None, draw=_SMALL_BIAS),
    "cfg5": _case(CFG5, 12, plds=0, near=8, draw=_SMALL_BIAS),
    "d2_default_target_f64": _case(D2_F64, 2),
    "autoreset_same_step": _case(D2_MODE, 2, kw=dict(autoreset="same_step", max_episode_steps=9), limit=True),
    "autoreset_next_step": _case(D2_MODE, 2, kw=dict(autoreset="next_step", max_episode_steps=9), limit=True),
    "autoreset_disabled": _case(D2_MODE, 2, kw=dict(autoreset="disabled")),
    "max5_autoreset_disabled": _case(D2_MODE, 2, kw=dict(autoreset="disabled", max_episode_steps=5), limit=True),
}
RNGS = ("numpy", "philox")


def theta_of(name, n=N):
    c = CASES[name]
    seed = 100 + sorted(CASES).index(name.replace("_no_lds", ""))
    return ref.draw_theta(n, c["D"], seed, **c["draw"])


def near_state(name, state, mdp):
    """The state record with every ``near``-th env moved next to the target, at rest, at the start of an episode."""
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


def conditions(name, actions, term, trunc, obs, smax=10.0, amax=1.0):
    """The figures the honesty conditions are stated on, from a run's outputs ([T, n, ...] arrays)."""
    a = np.asarray(actions)
    clipped = float(np.mean(np.abs(a) == np.float32(amax)))
    return dict(clipped=clipped, terminations=int(np.asarray(term).sum()), truncations=int(np.asarray(trunc).sum()),
                on_wall=int((np.abs(np.asarray(obs)) == np.float32(smax)).sum()))


def assert_conditions(name, fig, terminations=True):
    c = CASES[name]
    assert 0.05 <= fig["clipped"] <= 0.95, (name, fig)
    if terminations:
        assert fig["terminations"] > 0, (name, fig)
    assert fig["on_wall"] > 0, (name, fig)
    if c["limit"]:
        assert fig["truncations"] > 0, (name, fig)
