"""The grid learners without a GPU: values worked by hand that pin the restatement (tests/grid_learner_ref.py), the plumbing of
the new entry points (header, exports, bindings, option bit, methods), and the conditions that keep a GPU pass of
tests/test_gpu_grid_learn.py honest -- every case's closed loop runs here on the CPU, on the Philox streams the GPU test
uses, and must meet them by the restatement alone."""
import os
import re

import numpy as np
import pytest

import grid_learner_cases as gc
import grid_learner_ref as gref
import learner_sweep_ref as ref

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW_SYMBOLS = ("mdpp_set_grid_learner", "mdpp_clear_grid_learner", "mdpp_set_grid_learner_params", "mdpp_step_n_grid_learn",
               "mdpp_step_n_grid_eval", "mdpp_step_n_grid_learn_summary", "mdpp_step_n_grid_eval_summary", "mdpp_get_grid_q",
               "mdpp_set_grid_q", "mdpp_grid_learn_kernel_name")


# ---- values worked by hand ----
def test_state_index_of_the_cell_one_past_a_non_square_grid():
    # grid_shape (3, 4): rows of g1 + 1 = 5 entries, so cell (g0, 0) = (3, 0) is index 3 * 5 + 0 = 15 (transposed: 3 * 4 = 12, or
    # with rows of g1 entries: 12 as well), the last cell (3, 4) is 19 and S = 4 * 5 = 20
    assert gref.n_states((3, 4)) == 20
    assert int(gref.state_index(3, 0, (3, 4))) == 15
    assert int(gref.state_index(0, 4, (3, 4))) == 4
    assert int(gref.state_index(3, 4, (3, 4))) == 19
    Q = np.arange(2 * 20 * 4, dtype=np.float32).reshape(2, 20, 4)
    assert gref.as_grid(Q, (3, 4)).shape == (2, 4, 5, 4) and gref.as_grid(Q, (3, 4))[1, 3, 0, 2] == Q[1, 15, 2]
    assert np.array_equal(gref.as_flat(gref.as_grid(Q, (3, 4))), Q)


def test_the_five_action_vectors():
    assert gref.action_vector(np.arange(5)).tolist() == [[1, 0], [-1, 0], [0, 1], [0, -1], [0, 0]]
    assert np.array_equal(gref.action_vector(np.arange(5)), gref.ACTION_VECTORS)
    assert gref.action_vector(np.array([[3, 0]])).shape == (1, 2, 2)


def test_an_all_zero_row_selects_action_0():
    Q = np.zeros((3, 20, 5), np.float32)
    Q[1, 7] = [0.0, -0.0, 0.0, 0.0, -0.0]                   # (zeros of both signs tie too)
    Q[2, 7] = [-1.0, 0.5, 0.5, 0.25, 0.5]                   # the lowest of three maxima
    a, explored = ref.select("q_learning", Q, np.full(3, 7), np.zeros(3, np.uint32), np.zeros(3, np.uint32), np.zeros(3, np.int64))
    assert a.tolist() == [0, 0, 1] and not explored.any()


def test_one_update_in_unfused_float32_arithmetic():
    # q = 0, alpha = 0.5, gamma = f32(0.7), r = f32(1.1), max_j Q[s'] = f32(-19 / 7):
    #   g = gamma * qn = 0xbff33332;  y = r + g = 0xbf4cccca;  d = y - q = y;  u = alpha * d = 0xbeccccca;  q + u = 0xbeccccca
    # with r + gamma * qn fused into one rounding y would be 0xbf4ccccb and the new entry 0xbecccccb
    Q = np.zeros((1, 20, 4), np.float32)
    Q[0, 9] = [-3.0, np.float32(-19 / 7), -4.0, -5.0]
    ref.update("q_learning", Q, np.array([2]), np.array([1]), np.array([1.1], np.float32), np.array([9]), np.array([False]),
               np.array([True]), np.array([0.5], np.float32), np.array([0.7], np.float32))
    assert Q[0, 2, 1].view(np.uint32) == 0xBECCCCCA
    from fractions import Fraction as F
    fused_y = np.float32(float(F(float(np.float32(1.1))) + F(float(np.float32(0.7))) * F(float(np.float32(-19 / 7)))))
    assert fused_y.view(np.uint32) == 0xBF4CCCCB and np.float32(fused_y * np.float32(0.5)).view(np.uint32) == 0xBECCCCCB
    # terminated: y = r, whatever the next row holds
    Q[0, 2, 1] = 0
    ref.update("q_learning", Q, np.array([2]), np.array([1]), np.array([1.1], np.float32), np.array([9]), np.array([True]),
               np.array([True]), np.array([0.5], np.float32), np.array([0.7], np.float32))
    assert Q[0, 2, 1] == np.float32(np.float32(1.1) * np.float32(0.5))


# ---- plumbing ----
def test_header_has_the_section_and_every_new_symbol_is_declared_exported_and_bound():
    from mdp_playground_amd import _capi
    src = open(os.path.join(ROOT, "include", "mdpp.h")).read()
    assert "/* Grid learners:" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _capi.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _capi.EXPORTS, name
        assert getattr(lib, name).argtypes is not None, name
    assert lib.mdpp_grid_learn_kernel_name.restype is not None
    assert "A grid learner (mdpp_step_n_grid_learn" in src          # the HIP graphs section


def test_option_bit_and_methods():
    from mdp_playground_amd import _capi
    from mdp_playground_amd.vector_env import RLToyVectorEnv
    src = open(os.path.join(ROOT, "include", "mdpp.h")).read()
    assert re.search(r"MDPP_OPT_NO_GRID_QLDS\s*=\s*1u\s*<<\s*24", src)
    assert _capi.GRID_OPTIONS == {"NO_GRID_QLDS": 1 << 24}
    assert 1 << 24 == 2 * max(_capi.OPTIONS.values()) and "NO_GRID_QLDS" not in _capi.OPTIONS      # the next free bit
    assert len(re.findall(r"MDPP_OPT_[A-Z0-9_]+\s*=\s*1u\s*<<\s*(\d+)", src)) == 25
    for m in ("set_grid_learner", "set_grid_learner_rates", "rollout_grid_learn", "rollout_grid_eval", "alloc_rollout_grid",
              "get_grid_q", "set_grid_q", "grid_learn_kernel_name"):
        assert callable(getattr(RLToyVectorEnv, m)), m


def test_new_units_are_built_with_their_header():
    from mdp_playground_amd import build
    for u in ("mdpp_grid_learn.hip", "mdpp_grid_summary_learn.hip"):
        assert u in build.SOURCES and build.INCLUDED_SOURCES[u] == ["mdpp_grid_learn.hpp"] and u not in build.EXTRA_FLAGS


# ---- the conditions that keep a GPU pass honest ----
@pytest.mark.parametrize("algo", gref.ALGOS)
@pytest.mark.parametrize("case", sorted(gc.CASES))
def test_case_meets_its_conditions_on_the_cpu(case, algo):
    info, Q, traj = gc.cpu_run(case, algo)
    c = gc.CASES[case]
    assert info["explored"] > 0 and info["greedy_ties"] + info["greedy_strict"] > 0
    assert info["stay_steps"] > 0                              # s' == s: a move into a wall, or the noop
    assert info["terminations"] > 0
    assert info["updates"] > 0 and not np.array_equal(Q, np.zeros_like(Q) if gc.initial_tables(case) is None else gc.initial_tables(case))
    if c["kw"].get("max_episode_steps"):
        assert info["truncations"] > 0
    # the actions are the map's vectors, the observations cells of the grid or one past it
    assert np.array_equal(traj["vectors"], gref.ACTION_VECTORS[traj["actions"]])
    assert traj["actions"].max() == gc.n_actions(case) - 1
    g = np.asarray(c["cfg"]["grid_shape"])
    assert (traj["obs"] >= 0).all() and (traj["obs"] <= g).all() and (traj["next_cell"] < g).all()


def test_conditions_met_once_over_all_cases():
    total, sarsa = gref.new_info(gc.N), gref.new_info(gc.N)
    noisy_redrawn = next_step_resets = sarsa_cut = 0
    for case in sorted(gc.CASES):
        for algo in gref.ALGOS:
            info = gc.cpu_run(case, algo)[0]
            ref.merge_info(total, info)
            if algo == "sarsa":
                ref.merge_info(sarsa, info)
                sarsa_cut += info["trunc_resets"]
            if "transition_noise" in gc.CASES[case]["cfg"]:
                noisy_redrawn += info["redrawn_moves"]
            else:
                assert info["redrawn_moves"] == 0
            if gc.CASES[case]["kw"]["autoreset"] == "next_step":
                next_step_resets += info["reset_calls"]
            else:
                assert info["reset_calls"] == 0
    assert (total["start_on_g"] > 0).all()                     # an episode starting on index g, in each coordinate
    assert sarsa["carried"] > 0 and sarsa["carried_differs"] > 0
    assert sarsa_cut > 0                                       # a carry dropped at a truncation that resets
    assert noisy_redrawn > 0 and next_step_resets > 0
