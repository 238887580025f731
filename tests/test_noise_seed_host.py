"""Per-env noise levels on one MDP per env, without a GPU (set_noise_levels(..., per_env_mdp=True): a noise x seed sweep in one
launch): the opt-in rule of RLToyVectorEnv.set_noise_levels against a stand-in for the library that keeps the C rule of
include/mdpp.h, the option bit, the export and the six new units, the placement rule's arithmetic, and a CPU closed loop --
one oracle env per seed at its own level, driven by the learner's restatement -- showing that what
tests/test_gpu_noise_seeds.py asserts about its own coverage (noise_seed_cases.honest and FLOORS) is reachable for every case
it runs, before any GPU run."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import noise_seed_cases as cases
import per_env_mdp_cpu as pm
from mdp_playground_amd import _capi, build
from mdp_playground_amd import mdp as mdp_mod
from mdp_playground_amd.vector_env import RLToyVectorEnv

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NOT_BUILT = b"mdpp_set_noise_levels: per-env noise levels on one MDP per env: not built"
ONE_SHARED = b"mdpp_set_noise_levels: learner rollouts need one shared MDP (this handle has one MDP per env: seeds=[...])"


# ---- (a) the opt-in rule
class FakeLib:
    """the rule of include/mdpp.h for the two flags and mdpp_set_noise_levels, nothing else"""

    def __init__(self, num_tables, learn_pm):
        self.num_tables, self.learn_pm, self.nl_pm, self.nl_on, self.err, self.calls = num_tables, learn_pm, False, False, b"", []

    def mdpp_noise_levels_per_env_mdp(self, h, on):
        self.calls.append(("nl_pm", on))
        if self.num_tables != 1:
            if self.nl_pm and not on:
                self.nl_on = False
            self.nl_pm = bool(on)
        return 0

    def mdpp_learner_per_env_mdp(self, h, on):
        if self.num_tables != 1:
            if self.learn_pm and not on:
                self.nl_on = self.nl_on and not self.nl_pm
                self.nl_pm = False
            self.learn_pm = bool(on)
        return 0

    def mdpp_clear_learner(self, h):
        return 0

    def mdpp_set_noise_levels(self, h, tn, rn, stream):
        self.calls.append(("set", None))
        if self.num_tables != 1 and not self.learn_pm:
            self.err = ONE_SHARED
            return -4
        if self.num_tables != 1 and not (self.nl_pm and self.learn_pm):
            self.err = NOT_BUILT
            return _capi.EUNSUPPORTED
        self.nl_on = True
        return 0

    def mdpp_clear_noise_levels(self, h):
        self.nl_on = False
        return 0

    def mdpp_last_error(self, h):
        return self.err


def _stub(n=8, per_env=True, learn_pm=True):
    lib = FakeLib(n if per_env else 1, learn_pm)
    return types.SimpleNamespace(_lib=lib, _h=None, num_envs=n, _per_env=per_env, _learn_pm=learn_pm, _nl_pm=False, _noise_levels_set=False,
                                 _learn_rates=None, config=dict(cases.CREATED), _learn_check_kind=lambda: None, _stream=lambda: None,
                                 _drop_noise_levels_per_env_mdp=lambda: None), lib


def _set(env, *a, **kw):
    return RLToyVectorEnv.set_noise_levels(env, *a, **kw)


def test_the_opt_in_is_accepted_on_a_per_env_mdp_learner_and_only_with_it():
    env, lib = _stub()
    rn = np.full(8, 0.25)
    with pytest.raises(NotImplementedError, match="per-env noise levels on one MDP per env: not built") as e:
        _set(env, reward_noise=rn)                       # without the opt-in: today's refusal, today's message
    assert str(e.value) == NOT_BUILT.decode()
    assert not lib.nl_pm and not lib.nl_on and not env._noise_levels_set and ("nl_pm", 1) not in lib.calls
    _set(env, reward_noise=rn, per_env_mdp=True)
    assert lib.nl_pm and lib.nl_on and env._nl_pm and env._noise_levels_set
    _set(env, transition_noise=np.full(8, 0.1), per_env_mdp=True)       # again: the flag is not sent twice
    assert lib.calls.count(("nl_pm", 1)) == 1
    with pytest.raises(NotImplementedError, match="not built"):        # the call without it leaves the levels in force as they are
        _set(env, reward_noise=rn)
    assert lib.nl_pm and lib.nl_on and env._nl_pm and env._noise_levels_set
    RLToyVectorEnv.clear_noise_levels(env)                              # clears the levels and the opt-in
    assert not lib.nl_pm and not lib.nl_on and not env._nl_pm and not env._noise_levels_set
    with pytest.raises(NotImplementedError, match="not built"):
        _set(env, reward_noise=rn)


def test_the_opt_in_without_the_per_env_mdp_learner_raises_the_learners_refusal_and_leaves_no_flag():
    env, lib = _stub(learn_pm=False)
    with pytest.raises(NotImplementedError, match="need one shared MDP"):
        _set(env, reward_noise=np.full(8, 0.25), per_env_mdp=True)
    assert not lib.nl_pm and not env._nl_pm and not env._noise_levels_set and lib.calls[-1] == ("nl_pm", 0)


def test_the_opt_in_on_a_shared_mdp_is_a_value_error_before_anything_is_sent():
    env, lib = _stub(per_env=False, learn_pm=False)
    with pytest.raises(ValueError, match="per_env_mdp"):
        _set(env, reward_noise=np.full(8, 0.25), per_env_mdp=True)
    with pytest.raises(ValueError, match="per_env_mdp"):              # ... also ahead of a bad array
        _set(env, reward_noise=np.full(3, 0.25), per_env_mdp=True)
    assert lib.calls == []
    _set(env, reward_noise=np.full(8, 0.25))                           # the plain call on a shared MDP is what it was
    assert lib.nl_on and not lib.nl_pm and lib.calls == [("set", None)]
    with pytest.raises(ValueError, match="reward_noise"):              # bad arrays are refused as ever with the opt-in
        _set(_stub()[0], reward_noise=np.full(3, 0.25), per_env_mdp=True)


def test_set_learner_none_clears_levels_given_with_the_opt_in_and_only_those():
    env, lib = _stub()
    env._drop_noise_levels_per_env_mdp = lambda: RLToyVectorEnv._drop_noise_levels_per_env_mdp(env)
    _set(env, reward_noise=np.full(8, 0.25), per_env_mdp=True)
    RLToyVectorEnv.set_learner(env, None)
    assert not lib.learn_pm and not lib.nl_pm and not lib.nl_on and not env._nl_pm and not env._noise_levels_set and not env._learn_pm
    env, lib = _stub(per_env=False, learn_pm=False)                     # a shared MDP keeps its levels through set_learner(None)
    env._drop_noise_levels_per_env_mdp = lambda: RLToyVectorEnv._drop_noise_levels_per_env_mdp(env)
    _set(env, reward_noise=np.full(8, 0.25))
    RLToyVectorEnv.set_learner(env, None)
    assert lib.nl_on and env._noise_levels_set


# ---- (b) names
def test_the_option_bit_the_export_and_the_six_units():
    assert _capi.OPTIONS["NO_PM_NLEV_LDS"] == 1 << 22 and _capi.OPTIONS["NO_PM_LDS"] == 1 << 21 and _capi.OPTIONS["NO_NLEV_LDS"] == 1 << 20
    assert len(set(_capi.OPTIONS.values())) == len(_capi.OPTIONS)
    assert "mdpp_noise_levels_per_env_mdp" in _capi.EXPORTS and _capi.MDPP_ABI_VERSION == 8       # additive: the version stays
    header = open(os.path.join(ROOT, "include", "mdpp.h")).read()
    assert re.search(r"MDPP_OPT_NO_PM_NLEV_LDS\s*=\s*1u\s*<<\s*22\b", header) and "#define MDPP_ABI_VERSION 8" in header
    assert re.search(r"\bint\s+mdpp_noise_levels_per_env_mdp\s*\(\s*mdpp_env\s*\*\s*h\s*,\s*int\s+on\s*\)\s*;", header)
    lib = ctypes.CDLL(_capi.LIB_PATH)
    assert hasattr(lib, "mdpp_noise_levels_per_env_mdp")
    lib.mdpp_noise_levels_per_env_mdp.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert lib.mdpp_noise_levels_per_env_mdp(None, 1) == -1      # MDPP_EINVAL: no handle (nothing touches the GPU)
    for unit, base in [("mdpp_discrete_learn%s_pe_pm_nlev%s.hip" % (d, s), "mdpp_discrete_learn.hpp") for d in ("", "_double") for s in ("", "_summary")] + \
                      [("mdpp_discrete_eval_pm_nlev%s.hip" % s, "mdpp_discrete_eval.hpp") for s in ("", "_summary")]:
        assert unit in build.SOURCES and build.INCLUDED_SOURCES[unit] == [base], unit
        assert unit not in build.EXTRA_FLAGS                      # the build flags are the default ones
        assert os.path.exists(os.path.join(build.CSRC, unit)), unit


# ---- (c) the placement rule
def test_the_worked_placements():
    """S = A = 8, L = 1, unit rewards, numpy streams, five levels"""
    assert cases.placement(cases.TABULAR, "q_learning", "numpy") == (1, 2, True, 40960 + 2560 + 65536)
    assert cases.ZIG_BYTES + 40960 + 2560 + 65536 == 115200 <= cases.LDS_BYTES == 163840
    # double_q: Q is 131 072 B; with the slots it does not fit, with the cdfs it does
    assert cases.ZIG_BYTES + 131072 + 40960 > cases.LDS_BYTES
    assert cases.placement(cases.TABULAR, "double_q", "numpy") == (1, 1, True, 131072 + 2560)
    assert cases.ZIG_BYTES + 131072 + 2560 == 139776
    # S = A = 20: Q (409 600 B) and the slots (155 648 B) are beyond their bounds; the cdfs are staged
    assert cases.placement(cases.S20, "q_learning", "numpy") == (0, 1, True, 16000)
    assert cases.placement(cases.S29, "sarsa", "numpy") == (0, 1, False, 0)            # 33 640 B of cdfs: global memory by size
    assert cases.placement(cases.RDIST, "sarsa", "philox") == (1, 1, False, 65536)     # valued rewards: 656 B per lane, PM=1; Philox reads no cdf
    assert cases.placement(cases.CFG2, "q_learning", "numpy") == (1, 2, True, 256 * (64 + 16 + 64 + 64) + 2560 + 65536)


def test_every_subset_is_reachable_by_option_on_the_tabular_shape_in_the_rules_order():
    seen = {}
    for opts in [(), ("NO_PM_NLEV_LDS",), ("NO_PM_LDS",), ("NO_PM_LDS", "NO_PM_NLEV_LDS"), ("NO_LEARN_LDS",), ("NO_LEARN_LDS", "NO_PM_NLEV_LDS"),
                 ("NO_LEARN_LDS", "NO_PM_LDS"), ("NO_LEARN_LDS", "NO_PM_LDS", "NO_PM_NLEV_LDS")]:
        seen[opts] = cases.placement(cases.TABULAR, "q_learning", "numpy", *opts)[:3]
    assert list(seen.values()) == [(1, 2, True), (1, 2, False), (1, 1, True), (1, 1, False), (0, 2, True), (0, 2, False), (0, 1, True), (0, 1, False)]
    assert cases.placement(cases.TABULAR, "q_learning", "numpy", "NO_NLEV_LDS")[:3] == (1, 2, True)       # the shared-MDP option is not this one
    assert cases.kernel_name("learn", cases.TABULAR, "double_q", "numpy", 1, 1) == "k_discrete_learn_rollout<PHILOX=0,NOISE=1,UNIT=1,QLDS=1,PE=1,DOUBLE=1,NLEV=1,PM=1>"
    assert cases.kernel_name("eval", cases.RDIST, "sarsa", "philox", 1, 1, summary=True) == "k_discrete_eval_summary<PHILOX=1,NOISE=1,UNIT=0,QLDS=1,DOUBLE=0,NLEV=1,PM=1>"


# ---- (d) the level cycle
def test_the_level_cycle_puts_all_seven_pairs_into_every_wave():
    tn, rn = cases.level_arrays(cases.N)
    assert cases.pairs_present(tn, rn) == sorted(cases.PAIRS)
    assert sorted(set(tn)) == sorted(cases.TN) and sorted(set(rn)) == sorted(cases.RN)
    for lo in range(0, cases.N, 64):
        assert len(cases.pairs_present(tn[lo:lo + 64], rn[lo:lo + 64])) == 7
    assert ((tn[:-1] == 0.0) & (tn[1:] > 0.0)).any() and ((tn[:-1] > 0.0) & (tn[1:] == 0.0)).any()   # a lane that skips the draw beside one that makes it
    assert (0.0, 25.0) in cases.PAIRS and (0.25, 0.0) in cases.PAIRS
    h0, h1 = cases.level_arrays(160), cases.level_arrays(160, 160)      # a shard's slice continues the cycle
    assert np.array_equal(np.concatenate([h0[0], h1[0]]), tn) and np.array_equal(np.concatenate([h0[1], h1[1]]), rn)


@pytest.mark.parametrize("case", ["tabular", "rdist_delay3"])
def test_noise_keys_do_not_enter_the_generation_of_an_envs_tables(case):
    cfg = cases.CASES[case][0]
    tn, rn = cases.level_arrays(14)
    for i, m in enumerate(cases.level_mdps(cfg, tn, rn, cases.SEEDS[:14])):
        want = mdp_mod.build_mdp({**cases.twin_cfg(cfg, tn[i], rn[i]), "seed": cases.SEEDS[i]})
        assert np.array_equal(m.P, want.P) and np.array_equal(m.terminal_states, want.terminal_states) and np.array_equal(m.init_dist, want.init_dist)
        assert np.array_equal(m.reward_table(), want.reward_table())
        assert (m.transition_noise or 0.0) == (want.transition_noise or 0.0) == tn[i] and m.reward_noise == want.reward_noise == rn[i]
        created = mdp_mod.build_mdp({**cases.mixed_cfg(cfg), "seed": cases.SEEDS[i]})
        assert np.array_equal(m.P, created.P) and np.array_equal(m.reward_table(), created.reward_table())


# ---- (e) the coverage the GPU test asserts can be met: a CPU closed loop, one oracle env per seed at its own level
@pytest.mark.parametrize("case,algo", sorted({(c, a) for c, a, _ in cases.TWIN_PARAMS}))
def test_cpu_closed_loop_meets_honest_and_the_floors(case, algo):
    cfg, kw, _, k = cases.CASES[case]
    tn, rn = cases.level_arrays(cases.N)
    info, Q, traj = cases.closed_loop(cfg, kw, algo, tn, rn, K=k)
    assert traj["actions"].shape == (cases.LAUNCHES * k, cases.N)
    P, values = cases.tables(cfg)
    cases.honest(tn, rn, traj["state"], traj["actions"], traj["next_state"], traj["reward"], traj["terminated"], info["explored_env"], P, values,
                 ~traj["reset_call"])
    counts = cases.check_floors(case, Q, traj["terminated"], algo)
    print(case, algo, "non-zero Q: all, lanes 0-255, lanes 256-319; envs that terminated:", counts,
          {k_: v for k_, v in info.items() if not isinstance(v, np.ndarray)})
    assert info["explored"] > 0 and info["greedy_strict"] > 0, info


def test_env_i_of_the_loop_is_env_i_of_the_uniform_loop_at_its_pair():
    """the twin rule on the CPU: three envs of the mixed loop against per_env_mdp_cpu.closed_loop created uniformly at their
    pairs"""
    cfg, kw, _, k = cases.CASES["tabular"]
    tn, rn = cases.level_arrays(cases.N)
    _, Q, traj = cases.closed_loop(cfg, kw, "sarsa", tn, rn, K=k)
    for i in (3, 255, 258):
        _, q1, t1 = pm.closed_loop(cases.twin_cfg(cfg, tn[i], rn[i]), kw, "sarsa", cases.ALPHA, cases.GAMMA, cases.EPS, K=k)
        for key in ("actions", "obs", "terminated", "truncated"):
            assert np.array_equal(traj[key][:, i], t1[key][:, i]), (i, key)
        assert np.array_equal(traj["reward"][:, i].view(np.int32), t1["reward"][:, i].view(np.int32)), i
        assert np.array_equal(Q[i].view(np.int32), q1[i].view(np.int32)), i
