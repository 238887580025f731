"""Per-env noise levels on the host (no GPU): the validation and reduction RLToyVectorEnv.set_noise_levels applies
(mdp_playground_amd/policy.py), the per-level Philox (T, M) pairs against philox_pnoise_threshold / philox_pnoise_magic
restated here, the per-level cdf table against DiscreteMDP.noise_cdf(), the names of the C ABI, and a CPU closed loop -- the
oracle env per level driven by the learner's restatement, 32 envs per level -- showing that what tests/test_gpu_noise_levels.py
asserts about its own coverage can be met by the reference semantics alone, for every case it runs."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from closed_loop_cpu import closed_loop
import noise_levels_cases as cases
from mdp_playground_amd import _capi, build, policy
from mdp_playground_amd import mdp as mdp_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- (a) array validation
def test_noise_level_array_accepts_none_scalars_and_arrays():
    import torch
    assert policy.noise_level_array("transition_noise", None, 4) is None and policy.noise_level_array("reward_noise", None, 4) is None
    a = policy.noise_level_array("transition_noise", 0.25, 4)
    assert a.dtype == np.float64 and a.tolist() == [0.25] * 4                         # a scalar is broadcast
    assert policy.noise_level_array("reward_noise", 7, 3).tolist() == [7.0] * 3
    a = policy.noise_level_array("reward_noise", np.array([0, 1, 25], np.int32), 3)
    assert a.dtype == np.float64 and a.tolist() == [0.0, 1.0, 25.0]
    a = policy.noise_level_array("transition_noise", torch.tensor([0.0, 0.01, 1.0], dtype=torch.float32), 3)
    assert a.dtype == np.float64 and a.tolist() == [0.0, float(np.float32(0.01)), 1.0]
    assert policy.noise_level_array("transition_noise", [0.5, 0.5], 2).tolist() == [0.5, 0.5]
    z = policy.noise_level_array("transition_noise", np.array([-0.0, 0.1]), 2)
    assert not np.signbit(z[0])                                                        # -0.0 is the level 0.0
    src = np.array([0.1, 0.2])
    policy.noise_level_array("transition_noise", src, 2)[0] = 9.0                      # (a copy: the caller's array is not touched)
    assert src[0] == 0.1


@pytest.mark.parametrize("key,bad", [
    ("transition_noise", np.full(3, 0.1)), ("transition_noise", np.full((4, 1), 0.1)), ("transition_noise", np.full((2, 2), 0.1)),
    ("transition_noise", np.array([0.1, np.nan, 0.1, 0.1])), ("transition_noise", np.array([0.1, 1.5, 0.1, 0.1])),
    ("transition_noise", np.array([0.1, -0.01, 0.1, 0.1])), ("transition_noise", 1.01), ("transition_noise", float("nan")),
    ("transition_noise", np.array([True, False, True, True])), ("transition_noise", np.array(["a", "b", "c", "d"])),
    ("reward_noise", np.full(5, 1.0)), ("reward_noise", np.full((1, 4), 1.0)), ("reward_noise", np.array([1.0, np.nan, 1.0, 1.0])),
    ("reward_noise", np.array([1.0, -1.0, 1.0, 1.0])), ("reward_noise", np.array([1.0, np.inf, 1.0, 1.0])), ("reward_noise", -0.5),
    ("reward_noise", np.zeros(0))])
def test_noise_level_array_refuses_with_a_message_that_names_the_key(key, bad):
    with pytest.raises(ValueError, match=key):
        policy.noise_level_array(key, bad, 4)


def test_unknown_key_is_refused():
    with pytest.raises(ValueError):
        policy.noise_level_array("p_noise", 0.1, 4)


# ---- (b) level reduction
def test_levels_are_the_distinct_values_in_ascending_order_and_seventeen_are_refused():
    tn, _ = cases.level_arrays(320)
    levels, index = policy.noise_levels_reduce(tn)
    assert levels.dtype == np.float64 and levels.tolist() == sorted(cases.TN)
    assert index.dtype == np.uint8 and index.shape == (320,) and np.array_equal(levels[index], tn)
    levels, index = policy.noise_levels_reduce(np.array([0.25, 0.1, 0.25, 0.0, 0.1]))
    assert levels.tolist() == [0.0, 0.1, 0.25] and index.tolist() == [2, 1, 2, 0, 1]
    levels, index = policy.noise_levels_reduce(np.full(7, 0.3))
    assert levels.tolist() == [0.3] and not index.any()                                # all-equal: one level (level 0 is NOT "no noise")
    sixteen = np.arange(16) / 16.0
    assert policy.MAX_NOISE_LEVELS == _capi.MAX_NOISE_LEVELS == 16
    assert len(policy.noise_levels_reduce(np.tile(sixteen, 3))[0]) == 16
    policy.noise_level_array("transition_noise", np.tile(sixteen, 2), 32)
    seventeen = np.arange(17) / 17.0
    with pytest.raises(ValueError, match="17 distinct"):
        policy.noise_levels_reduce(seventeen)
    with pytest.raises(ValueError, match="transition_noise"):
        policy.noise_level_array("transition_noise", seventeen, 17)
    policy.noise_level_array("reward_noise", np.arange(40.0), 40)                      # (reward_noise has no level limit: sigma travels per env)
    src = open(os.path.join(ROOT, "include", "mdpp.h")).read()
    assert "#define MDPP_MAX_NOISE_LEVELS 16" in src


# ---- (c) the Philox pair of a level: philox_pnoise_threshold / philox_pnoise_magic (mdpp_rng.hpp) restated
def _threshold(p):
    t = np.ceil(np.float64(p) * 4294967296.0)
    return 4294967295 if t >= 4294967295.0 else (0 if t <= 0.0 else int(t))


def _magic(T, S):
    if S < 2 or T <= S - 1:
        return 0
    q = Fraction((S - 1) << 64, T)
    return int(q) + (q.denominator != 1)                                               # ceil(2^64 (S - 1) / T)


@pytest.mark.parametrize("S", [2, 8, 20, 29, 255])
def test_per_level_thresholds_and_magics(S):
    levels = np.array(sorted(cases.TN + (1e-12, 1e-9, 5e-8, 0.5, 1.0)))
    T, M = policy.noise_level_thresholds(levels, S)
    assert T.dtype == np.uint32 and M.dtype == np.uint64
    assert T.tolist() == [_threshold(p) for p in levels] and M.tolist() == [_magic(int(t), S) for t in T]
    assert T[0] == 0 and M[0] == 0                                                     # p == 0: the state is the table's
    assert (T[1:] > 0).all()                                                           # T == 0 <=> p == 0: the kernel's "no draw" test
    assert T[-1] == 2 ** 32 - 1
    # the rule the pair implements: floor(w (S - 1) / T) for w < T is the top word of the 32 x 64-bit product w M
    rs = np.random.default_rng(S)
    for t, m in zip(T.tolist(), M.tolist()):
        if m == 0:
            continue
        for w in [0, t - 1] + rs.integers(0, t, 50).tolist():
            assert (w * m) >> 64 == (w * (S - 1)) // t


# ---- (d) the per-level cdf table
@pytest.mark.parametrize("S", [2, 8, 20, 29])
def test_per_level_cdfs_equal_noise_cdf_of_an_mdp_built_at_that_level(S):
    levels = np.array(cases.TN)
    tab = policy.noise_level_cdfs(levels, S)
    assert tab.dtype == np.float64 and tab.shape == (5, S, S)
    assert not tab[0].any()                                                            # level 0.0 makes no draw: never read
    cfg = dict(cases.TABULAR, state_space_size=S, action_space_size=S)
    for l, p in enumerate(levels):
        m = mdp_mod.build_mdp(dict(cfg, transition_noise=float(p)))
        want = m.noise_cdf()
        if p == 0.0:
            assert want is None
            continue
        assert np.array_equal(tab[l].view(np.int64), want.view(np.int64)), (S, p)
        assert (tab[l][:, -1] == 1.0).all() and (np.diff(tab[l], axis=1) > 0).all()


# ---- (e) names
def test_the_entry_points_are_declared_bound_and_their_units_listed():
    src = open(os.path.join(ROOT, "include", "mdpp.h")).read()
    for name in ("mdpp_set_noise_levels", "mdpp_get_noise_levels", "mdpp_clear_noise_levels"):
        assert name in _capi.EXPORTS
        assert re.search(r"\b%s\s*\(" % name, src), name
    lib = _capi.load()
    assert len(lib.mdpp_set_noise_levels.argtypes) == 4 and len(lib.mdpp_get_noise_levels.argtypes) == 3
    assert _capi.MDPP_ABI_VERSION == 8                                                 # additive: the version stays
    assert "MDPP_OPT_NO_NLEV_LDS = 1u << 20" in src and _capi.OPTIONS["NO_NLEV_LDS"] == 1 << 20
    for unit, base in (("mdpp_discrete_learn_pe_nlev.hip", "mdpp_discrete_learn.hpp"), ("mdpp_discrete_learn_double_pe_nlev.hip", "mdpp_discrete_learn.hpp"),
                       ("mdpp_discrete_learn_pe_nlev_summary.hip", "mdpp_discrete_learn.hpp"),
                       ("mdpp_discrete_learn_double_pe_nlev_summary.hip", "mdpp_discrete_learn.hpp"),
                       ("mdpp_discrete_eval_nlev.hip", "mdpp_discrete_eval.hpp"), ("mdpp_discrete_eval_nlev_summary.hip", "mdpp_discrete_eval.hpp")):
        assert unit in build.SOURCES and build.INCLUDED_SOURCES[unit] == [base]
        assert unit not in build.EXTRA_FLAGS                                           # the build flags are the default ones


def test_the_level_cycles_put_all_25_pairs_into_every_wave():
    tn, rn = cases.level_arrays(320)
    assert len(cases.pairs_present(tn, rn)) == 25
    for lo in range(0, 320, 64):
        assert len(cases.pairs_present(tn[lo:lo + 64], rn[lo:lo + 64])) == 25
    assert len(cases.pairs_present(*cases.level_arrays(25, 7))) == 25                  # any 25 consecutive envs
    t63, r63 = cases.level_arrays(63)
    assert len(cases.pairs_present(t63, r63)) == 25
    assert (tn[:-1] == 0.0).any() and ((tn[:-1] == 0.0) & (tn[1:] > 0.0)).any()        # a lane that skips the draw beside one that makes it


# ---- (f) the coverage the GPU test asserts can be met: a closed loop on the CPU, the oracle env per level
@pytest.mark.parametrize("case,algo", sorted({(c, a) for c, a, _ in cases.TWIN_PARAMS}))
def test_cpu_closed_loop_meets_the_coverage_the_gpu_test_asserts(case, algo):
    cfg, kw, _ = cases.CASES[case]
    P = np.asarray(mdp_mod.build_mdp(dict(cfg)).P)
    n = 32
    cols = {k: [] for k in ("state", "actions", "next_state", "reward", "terminated", "reset_call")}
    tn, rn, explored = [], [], []
    for l in range(5):                                        # level l of both keys: 32 envs of a handle created at that pair
        info, _, traj = closed_loop(cases.twin_cfg(cfg, cases.TN[l], cases.RN[l]), kw, algo, cases.ALPHA, cases.GAMMA, cases.EPS, n,
                                    seed=cases.SEED, K=cases.K, launches=cases.LAUNCHES, off=l * n)
        for k in cols:
            cols[k].append(traj[k])
        tn += [cases.TN[l]] * n
        rn += [cases.RN[l]] * n
        explored.append(info["explored_env"])
    c = {k: np.concatenate(v, axis=1) for k, v in cols.items()}
    cases.honest(np.asarray(tn), np.asarray(rn), c["state"], c["actions"], c["next_state"], c["reward"], c["terminated"],
                 np.concatenate(explored), P, ~c["reset_call"])
