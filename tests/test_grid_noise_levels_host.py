"""Per-env noise levels of grid handles without a GPU: the plumbing of the new entry points (header section, exports, bindings,
methods, build units), the conditions that keep a GPU pass of tests/test_gpu_grid_noise_levels.py honest -- every case's
composition (tests/grid_noise_levels_ref.py) runs here on the CPU, on the Philox streams the GPU test uses, and must meet them
by the restatement alone --, and the argument errors of set_grid_noise_levels that need no device."""
import os
import re

import numpy as np
import pytest

import grid_learner_ref as gref
import grid_noise_level_cases as nc
import grid_noise_levels_ref as nref

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW_SYMBOLS = ("mdpp_set_grid_noise_levels", "mdpp_get_grid_noise_levels", "mdpp_clear_grid_noise_levels")
NEW_UNITS = ("mdpp_grid_levels_learn.hip", "mdpp_grid_summary_levels_learn.hip", "mdpp_grid_levels_sched_learn.hip",
             "mdpp_grid_summary_levels_sched_learn.hip", "mdpp_grid_episodes_levels_learn.hip", "mdpp_grid_episodes_levels_sched_learn.hip")
OLD_UNITS = ("mdpp_grid_learn.hip", "mdpp_grid_summary_learn.hip", "mdpp_grid_sched_learn.hip", "mdpp_grid_summary_sched_learn.hip",
             "mdpp_grid_episodes_learn.hip", "mdpp_grid_episodes_sched_learn.hip")


# ---- plumbing ----
def test_header_has_the_section_and_every_new_symbol_is_declared_exported_and_bound():
    from mdp_playground_amd import _capi
    src = open(os.path.join(ROOT, "include", "mdpp.h")).read()
    assert "/* Grid noise levels." in src
    assert src.index("/* Grid learner schedules and the episode log.") < src.index("/* Grid noise levels.") < src.index("/* Linear policies:")
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _capi.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _capi.EXPORTS, name
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.mdpp_set_grid_noise_levels.argtypes) == 4 and len(lib.mdpp_get_grid_noise_levels.argtypes) == 3
    assert "Grid noise levels (mdpp_set_grid_noise_levels)" in src                 # the HIP graphs section
    assert len(lib.mdpp_grid_learn_kernel_name.argtypes) == 4                      # (its signature stays)
    assert _capi.GRID_OPTIONS == {"NO_GRID_QLDS": 1 << 24}                         # (no option bit was needed)


def test_methods_and_build_units():
    from mdp_playground_amd import build
    from mdp_playground_amd.vector_env import RLToyVectorEnv
    for m in ("set_grid_noise_levels", "grid_noise_levels", "clear_grid_noise_levels"):
        assert callable(getattr(RLToyVectorEnv, m)), m
    for u in NEW_UNITS:
        assert u in build.SOURCES and build.INCLUDED_SOURCES[u] == ["mdpp_grid_learn.hpp"] and u not in build.EXTRA_FLAGS
        assert os.path.exists(os.path.join(build.CSRC, u))
        assert "log" not in u and "trace" not in u and not u.endswith("_summary.hip")
    for u in OLD_UNITS:
        assert u in build.SOURCES and u not in build.EXTRA_FLAGS
    assert "mdpp_grid_learn_body.inc" in build.HEADERS


def test_the_cases_are_the_ones_of_the_table():
    assert (nc.N, nc.K, nc.LAUNCHES) == (320, 37, 2)
    assert {c: (v["cfg"]["grid_shape"], v["kw"]["autoreset"], v["kw"]["max_episode_steps"], nc.n_actions(c), v["qlds"], v["rates"], v["pairs"])
            for c, v in nc.CASES.items()} == {
        "g34_both": ((3, 4), "same_step", 9, 4, 1, (0.5, 0.9, 0.3), ((0.0, 0.0), (0.1, 0.5), (0.5, 0.0), (1.0, 2.0))),
        "g55_noop_next_ponly": ((5, 5), "next_step", 7, 5, 0, (0.5, 0.75, 0.35), ((0.0, None), (0.25, None), (0.6, None))),
        "g88_disabled_ronly": ((8, 8), "disabled", 29, 4, 0, (0.75, 0.5, 0.5), ((None, 0.0), (None, 1.0), (None, 5.0))),
        "g17_both_i32": ((1, 7), "same_step", 11, 4, 1, (0.5, 0.9, 0.3), ((0.0, 0.5), (0.3, 0.0), (0.05, 3.0)))}
    for case, c in nc.CASES.items():
        idx, m = nc.pair_index(case), len(c["pairs"])
        assert (idx[64:128] == 0).all() and (idx[128:192] == m - 1).all()         # one whole wave at the first pair, one at the last
        for w in (0, 3, 4):                                                        # the other waves mix every pair
            assert set(idx[64 * w:64 * (w + 1)].tolist()) == set(range(m))
        lv = nc.levels(case)
        for key, col in (("transition_noise", 0), ("reward_noise", 1)):
            assert (lv[key] is None) == (key not in c["cfg"]) == (c["pairs"][0][col] is None)
            if lv[key] is not None:
                assert lv[key].dtype == np.float64 and np.array_equal(lv[key], np.array([p[col] for p in c["pairs"]])[idx])
    # a uniform handle at p = 0 has no transition key; reward_noise = 0 stays named
    assert "transition_noise" not in nc.uniform_cfg("g34_both", (0.0, 0.0)) and nc.uniform_cfg("g34_both", (0.0, 0.0))["reward_noise"] == 0.0
    assert nc.uniform_name("g55_noop_next_ponly", (0.0, None), "numpy") == "k_grid_learn_rollout<PHILOX=0,NOISE=0,QLDS=0,EVAL=0,SUMMARY=0>"
    assert nc.expected_name("g17_both_i32", "philox", summary=True, sched=True) == \
        "k_grid_learn_rollout<PHILOX=1,NOISE=1,QLDS=1,EVAL=0,SUMMARY=1,NLEV=1,SCHED=1>"
    s = nc.schedule()
    assert s["epsilon"].shape == s["alpha"].shape == (2, 4) and np.array_equal(s["row"], np.arange(nc.N) % 2)


# ---- the conditions that keep a GPU pass honest ----
@pytest.mark.parametrize("algo", gref.ALGOS)
@pytest.mark.parametrize("case", sorted(nc.CASES))
def test_case_meets_its_conditions_on_the_cpu(case, algo):
    infos, Q, traj = nref.cpu_run(case, algo)
    c = nc.CASES[case]
    assert len(infos) == len(c["pairs"])
    for (p, sigma), info in zip(c["pairs"], infos):
        what = (case, algo, p, sigma)
        assert (info["redrawn_moves"] > 0) == bool(p), what                     # re-drawn moves iff p > 0
        assert info["terminations"] > 0 and info["truncations"] > 0, what
        assert (info["reset_calls"] > 0) == (c["kw"]["autoreset"] == "next_step"), what
        assert (info["off_lattice"] > 0) == bool(sigma), what                   # rewards off the noiseless lattice iff sigma > 0
        assert info["explored"] > 0 and info["greedy"] > 0, what
    print(case, algo, [{k: i[k] for k in ("redrawn_moves", "terminations", "truncations", "reset_calls", "off_lattice")} for i in infos])


def test_conditions_met_once_over_all_cases():
    differ = whole = 0
    for case in sorted(nc.CASES):
        c = nc.CASES[case]
        ps = np.array([0.0 if p[0] is None else p[0] for p in c["pairs"]])[nc.pair_index(case)]
        hi = np.asarray(c["cfg"]["grid_shape"], np.int64) - 1
        for algo in gref.ALGOS:
            infos, Q, traj = nref.cpu_run(case, algo)
            redrawn = (np.clip(traj["cell"] + traj["vectors"], 0, hi) != traj["next_cell"]).any(axis=2) & ~traj["reset_call"]
            for w in range(0, nc.N, 64):
                lane_p, r = ps[w:w + 64], redrawn[:, w:w + 64]
                if "transition_noise" in c["cfg"] and (lane_p == 0).all():
                    whole += 1                                                     # a wave wholly at p = 0 (on a handle with the key)
                    assert not r.any()
                # two lanes of one wave at different p of which one re-draws its move at a step where the other keeps it
                if len(set(lane_p.tolist())) > 1:
                    mixed = r.any(axis=1) & ~r.all(axis=1)
                    lo, hi_p = lane_p == lane_p.min(), lane_p == lane_p.max()
                    differ += int((mixed & r[:, hi_p].any(axis=1) & ~r[:, lo].all(axis=1)).sum())
    assert differ > 0 and whole > 0


# ---- argument errors that need no device ----
def _stub(case, n=nc.N):
    """a handle's Python side alone: the checks under test run before any library call"""
    from mdp_playground_amd.vector_env import RLToyVectorEnv
    env = object.__new__(RLToyVectorEnv)
    env._h, env.num_envs, env.kind, env.config = None, n, "grid", dict(nc.CASES[case]["cfg"])
    return env


def test_argument_errors_name_the_key_before_any_device_work():
    env = _stub("g34_both")
    n = nc.N
    nan = np.zeros(n); nan[n - 1] = np.nan
    over = np.zeros(n); over[3] = 1.0 + 2.0 ** -52
    neg = np.zeros(n); neg[0] = -1e-300
    for key, bad in (("transition_noise", np.zeros(n - 1)), ("reward_noise", np.zeros(n + 1)),              # a wrong length
                     ("transition_noise", np.zeros((n, 1))), ("reward_noise", np.zeros((1, n))),              # 2-D
                     ("transition_noise", nan), ("reward_noise", nan),                                       # NaN
                     ("transition_noise", over), ("transition_noise", neg), ("transition_noise", 1.5),       # out of [0, 1]
                     ("reward_noise", neg), ("reward_noise", -0.5), ("reward_noise", np.full(n, np.inf))):   # negative, not finite
        with pytest.raises(ValueError, match=key):
            env.set_grid_noise_levels(**{key: bad})
    # a key the config lacks (named, whatever the other argument is)
    with pytest.raises(ValueError, match="transition_noise: the handle was created without the key"):
        _stub("g88_disabled_ronly").set_grid_noise_levels(transition_noise=np.zeros(n), reward_noise=np.ones(n))
    with pytest.raises(ValueError, match="reward_noise: the handle was created without the key"):
        _stub("g55_noop_next_ponly").set_grid_noise_levels(reward_noise=0.5)
    # nothing given: nothing to do, no library call
    assert env.set_grid_noise_levels() is None
    # a handle that is not a grid
    env.kind = "discrete"
    with pytest.raises(NotImplementedError, match="serve grid envs only"):
        env.set_grid_noise_levels(reward_noise=0.5)


def test_the_sibling_of_noise_level_array_applies_the_same_checks_without_the_limit():
    from mdp_playground_amd import policy
    many = np.linspace(0.0, 1.0, 64)
    with pytest.raises(ValueError, match="distinct values"):
        policy.noise_level_array("transition_noise", many, 64)                     # (the discrete form's limit stays)
    a = policy.grid_noise_level_array("transition_noise", many, 64)
    assert a.dtype == np.float64 and np.array_equal(a, many)
    z = policy.grid_noise_level_array("transition_noise", np.array([-0.0, 0.5]), 2)
    assert not np.signbit(z[0])                                                    # -0.0 becomes 0.0
    assert policy.grid_noise_level_array("reward_noise", None, 4) is None
    assert np.array_equal(policy.grid_noise_level_array("reward_noise", 2, 3), np.full(3, 2.0))
    with pytest.raises(ValueError):
        policy.grid_noise_level_array("noise", 0.5, 3)
