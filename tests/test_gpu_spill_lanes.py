"""Every kernel of tests/spill_exposed.py's EXPOSED -- a kernel of a default-flag translation unit that spills SGPRs and
VGPRs, so SGPRs parked in VGPR lanes may be lost where that VGPR is spilled inside divergent control flow (docs/round6.md
section 10) -- launched by name and compared with the oracle on EVERY lane, with resets that diverge inside waves.

512 envs = 8 full waves, same-step autoreset.  The configurations end episodes at per-env times: a target radius large
against state_space_max (about one env in ten ends on each step), terminal boxes in some of the GEN forms, a step limit in
a few (the counters are staggered by then).  The returned flags prove it: every wave sees at least 8 steps on which some
of its lanes reset and the others do not (spill_exposed.assert_resets_diverge)."""
import warnings

import pytest

import spill_exposed as sx
from test_gpu_parity import _venv
from test_gpu_sweep import _check_vs_oracle

pytestmark = pytest.mark.gpu

N = 512
_RADIUS = {4: 1.0, 8: 1.5, 12: 2.0}      # (6-15 % of the envs end on each step at state_space_max 1 and time_unit 1)
_ROLLOUT_CALLS = (72, 1, 1, 1, 40)
_STEP_CALLS = (1,) * 32


def _cfg(D, order, nrel, seed, pn=0.05, rn=0.05, **extra):
    c = dict(state_space_type="continuous", action_space_type="continuous", state_space_dim=D, action_space_dim=D,
             relevant_indices=list(range(nrel)), target_point=[0.0] * nrel, target_radius=_RADIUS[nrel], state_space_max=1.0,
             action_space_max=1, transition_dynamics_order=order, inertia=1, time_unit=1.0, make_denser=True,
             reward_function="move_to_a_point", seed=seed)
    if nrel < D:
        c["irrelevant_features"] = True
    if pn:
        c["transition_noise"] = pn
    if rn:
        c["reward_noise"] = rn
    c.update(extra)
    return c


def _boxes(nrel, **extra):
    """GEN by terminal hypercubes: two boxes of edge 0.6 in the relevant coordinates"""
    return dict(terminal_states=[[0.6] * nrel, [-0.6] * nrel], term_state_edge=0.6, **extra)


_PX = dict(rng="philox", philox_seed=11)
# name: (config, env kwargs beyond same-step autoreset, kernel options, calls)
CASES = {
    "r8o2n4_np2": (_cfg(8, 2, 4, 1), {}, (), _ROLLOUT_CALLS),
    "r8o2n4_px2": (_cfg(8, 2, 4, 2, rn=0), _PX, (), _ROLLOUT_CALLS),
    "r8o2n4_px2_gen": (_cfg(8, 2, 4, 3, **_boxes(4)), _PX, (), _ROLLOUT_CALLS),
    "r8o2n8_np2": (_cfg(8, 2, 8, 4, pn=0), dict(max_episode_steps=13), (), _ROLLOUT_CALLS),
    "r8o2n8_px2": (_cfg(8, 2, 8, 5), _PX, (), _ROLLOUT_CALLS),
    "r8o2n8_np2_gen": (_cfg(8, 2, 8, 6, delay=2), {}, (), _ROLLOUT_CALLS),
    "r8o2n8_px2_gen": (_cfg(8, 2, 8, 7, reward_every_n_steps=3), _PX, (), _ROLLOUT_CALLS),
    "r12o1n4_np2": (_cfg(12, 1, 4, 8), {}, (), _ROLLOUT_CALLS),
    "r12o1n4_px2": (_cfg(12, 1, 4, 9), dict(_PX, max_episode_steps=13), (), _ROLLOUT_CALLS),
    "r12o1n4_px2_gen": (_cfg(12, 1, 4, 10, delay=1), _PX, (), _ROLLOUT_CALLS),
    "r12o1n12_np2": (_cfg(12, 1, 12, 11, rn=0), {}, (), _ROLLOUT_CALLS),
    "r12o1n12_px2": (_cfg(12, 1, 12, 12), _PX, (), _ROLLOUT_CALLS),
    "r12o1n12_np2_gen": (_cfg(12, 1, 12, 13, **_boxes(12, delay=1)), {}, (), _ROLLOUT_CALLS),
    "r12o1n12_px2_gen": (_cfg(12, 1, 12, 14, reward_every_n_steps=2), _PX, (), _ROLLOUT_CALLS),
    "r12o2n4_np1": (_cfg(12, 2, 4, 15), {}, ("NO_PARK",), _ROLLOUT_CALLS),
    "r12o2n4_np2": (_cfg(12, 2, 4, 16), {}, (), _ROLLOUT_CALLS),
    "r12o2n4_px1": (_cfg(12, 2, 4, 17), _PX, ("NO_TRIO",), _ROLLOUT_CALLS),
    "r12o2n4_px2": (_cfg(12, 2, 4, 18), dict(_PX, max_episode_steps=13), (), _ROLLOUT_CALLS),
    "r12o2n4_np1_gen": (_cfg(12, 2, 4, 19, **_boxes(4)), {}, ("NO_TRIO",), _ROLLOUT_CALLS),
    "r12o2n4_np2_gen": (_cfg(12, 2, 4, 20, delay=2), {}, (), _ROLLOUT_CALLS),
    "r12o2n4_px2_gen": (_cfg(12, 2, 4, 21, **_boxes(4, delay=1)), _PX, (), _ROLLOUT_CALLS),
    "r12o2n12_np1": (_cfg(12, 2, 12, 22, rn=0), {}, ("NO_TRIO",), _ROLLOUT_CALLS),
    "r12o2n12_np2": (_cfg(12, 2, 12, 23), {}, (), _ROLLOUT_CALLS),
    "r12o2n12_px1": (_cfg(12, 2, 12, 24), _PX, ("NO_TRIO",), _ROLLOUT_CALLS),
    "r12o2n12_px2": (_cfg(12, 2, 12, 25, pn=0), _PX, (), _ROLLOUT_CALLS),
    "r12o2n12_np1_gen": (_cfg(12, 2, 12, 26, reward_every_n_steps=3), {}, ("NO_PARK",), _ROLLOUT_CALLS),
    "r12o2n12_np2_gen": (_cfg(12, 2, 12, 27, **_boxes(12)), dict(max_episode_steps=13), (), _ROLLOUT_CALLS),
    "r12o2n12_px1_gen": (_cfg(12, 2, 12, 28, delay=2), _PX, ("NO_TRIO",), _ROLLOUT_CALLS),
    "r12o2n12_px2_gen": (_cfg(12, 2, 12, 29, **_boxes(12)), _PX, (), _ROLLOUT_CALLS),
    # the one-step kernels: numpy streams with transition noise, single steps
    "s12o2n4_par": (_cfg(12, 2, 4, 30), {}, (), _STEP_CALLS),
    "s12o2n12_par": (_cfg(12, 2, 12, 31, rn=0), {}, (), _STEP_CALLS),
    "s12o2n12_par_gen": (_cfg(12, 2, 12, 32, delay=1), dict(max_episode_steps=13), (), _STEP_CALLS),
}


def test_every_exposed_kernel_has_a_case():
    assert sorted(sx.EXPOSED.values()) == sorted(CASES)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("key", sorted(sx.EXPOSED), ids=lambda k: sx.EXPOSED[k])
def test_spill_exposed_kernel_every_lane_with_divergent_resets_vs_oracle(key):
    name = sx.EXPOSED[key]
    cfg, kw, opts, calls = CASES[name]
    kw = dict(kw, autoreset="same_step")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = _venv(num_envs=N, **kw, **cfg)
    if opts:
        env.set_kernel_options(*opts)
    single = key[1][sx.CFAST_PARAMS.index("K1")] == 1
    for K in (1,) if single else sorted(k for k in set(calls) if k > 1):
        got = env.rollout_kernel_name(K)
        assert sx.parse_dispatched(got) == key, (name, K, got, sx.describe(key))
    ends = []
    mode = "timelimit" if kw.get("max_episode_steps") else "same_step"
    _check_vs_oracle(env, name, cfg, mode, kw, 4000 + sum(map(ord, name)), stride=1, calls=calls, flags=ends)
    assert not (env.status() & 0x80000000).any()
    env.close()
    per_wave = sx.assert_resets_diverge(ends, single)
    print(name, sx.describe(key), "steps with divergent resets per wave:", per_wave.tolist())
