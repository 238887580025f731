"""Linear policies with memory without a GPU: the numpy restatement (tests/linear_history_ref.py) against values worked by hand,
the interface -- header text, bindings, build table, the built library's symbols and kernels -- and the figure the feature
rests on: on a double integrator a policy that also reads the previous observation can brake, a memoryless one cannot."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest

import linear_history_ref as href
import linear_policy_ref as ref
import spill_exposed as sx
from mdp_playground_amd import _capi, build
from mdp_playground_amd import mdp as mdp_mod

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mdpp_set_linear_policy_history", "mdpp_linear_policy_history", "mdpp_linear_memory")
UNITS = ("mdpp_continuous_linear_h2.hip", "mdpp_continuous_summary_linear_h2.hip", "mdpp_continuous_search_h2.hip",
         "mdpp_continuous_summary_search_h2.hip", "mdpp_continuous_es_h2.hip", "mdpp_continuous_summary_es_h2.hip")
KERNELS = ("k_continuous_linear_rollout", "k_continuous_linear_summary", "k_continuous_search_rollout", "k_continuous_search_summary",
           "k_continuous_es_rollout", "k_continuous_es_summary")


def _theta(W, V, b):
    W, V, b = np.asarray(W, F32), np.asarray(V, F32), np.asarray(b, F32)
    return np.ascontiguousarray(np.concatenate([W, V, b[:, None]], axis=1))


def _act(W, V, b, o, p, amax=10.0):
    return href.history_actions(_theta(W, V, b), np.asarray([o], F32), np.asarray([p], F32), amax)[0]


def test_the_sum_runs_b_then_w_then_v():
    """b = 1e8 (float32 spacing 8), w o = -1e8, v p = 3: b + w o = 0, then + 3 = 3.  Taken V first, 1e8 + 3 rounds back to 1e8
    and the sum is 0; taken with b last, -1e8 + 3 rounds to -1e8 and the sum is 0 too."""
    a = _act([[-1e8]], [[3.0]], [1e8], [1.0], [1.0])
    assert a.tolist() == [3.0]
    assert F32(F32(F32(1e8) + F32(3.0)) + F32(-1e8)) == 0.0 and F32(F32(F32(-1e8) + F32(3.0)) + F32(1e8)) == 0.0
    # ... and within V the columns run 0, 1: b + 0 + 0 = 1e8, + (-1e8) = 0, + 3 = 3 -- not 1e8 + 3 first
    a = _act([[0.0, 0.0], [0.0, 0.0]], [[-1e8, 3.0], [0.0, 0.0]], [1e8, 0.0], [5.0, 5.0], [1.0, 1.0])
    assert a.tolist() == [3.0, 0.0]


def test_no_fused_multiply_add_in_the_v_pass():
    """v = p = 1 + 2^-12: the product 1 + 2^-11 + 2^-24 rounds to 1 + 2^-11, and b = -(1 + 2^-11) makes the sum exactly 0;
    fma(v, p, b) would keep 2^-24."""
    w = F32(1 + 2.0 ** -12)
    b = F32(-(1 + 2.0 ** -11))
    a = _act([[0.0]], [[w]], [b], [123.0], [w])
    assert a.view(np.uint32).tolist() == [0]
    assert float(w) * float(w) + float(b) == 2.0 ** -24


def test_clamp_and_nan():
    assert _act([[2.0]], [[3.0]], [0.0], [1.0], [1.0], amax=1.0).tolist() == [1.0]
    assert _act([[-2.0]], [[-3.0]], [0.0], [1.0], [1.0], amax=1.0).tolist() == [-1.0]
    assert _act([[0.5]], [[0.25]], [0.0], [1.0], [1.0], amax=1.0).tolist() == [0.75]
    a = _act([[1.0, 0.0], [0.0, 1.0]], [[0.0, np.nan], [0.0, 0.0]], [0.0, 0.0], [0.5, 0.5], [0.0, 0.0], amax=1.0)
    assert np.isnan(a[0]) and a[1] == 0.5              # NaN * 0 is NaN: it stays, and only in its row


def test_p_is_o_on_a_step_count_of_zero_and_the_memory_otherwise():
    th = _theta([[0.0]], [[1.0]], [0.0])               # a = p
    obs0 = np.asarray([[2.0], [2.0], [2.0]], F32)
    carry = href.new_carry(obs0, steps0=[0, 3, 0])
    carry["mem"][:] = [[7.0], [7.0], [7.0]]
    obs = np.asarray([[[3.0], [3.0], [3.0]], [[4.0], [4.0], [4.0]], [[5.0], [5.0], [5.0]]], F32)
    term = np.asarray([[0, 0, 1], [0, 0, 0], [0, 0, 0]], np.uint8)
    acts, p, first, after = href.launch(th, carry, obs0, obs, term, np.zeros_like(term), "same_step", 100.0)
    assert acts[:, 0, 0].tolist() == [2.0, 2.0, 3.0]   # count 0: p = o = 2; then the memory: 2, 3
    assert acts[:, 1, 0].tolist() == [7.0, 2.0, 3.0]   # count 3: the memory it came with
    assert acts[:, 2, 0].tolist() == [2.0, 3.0, 3.0]   # ended at step 0: at step 1 the count is 0 again, p = o = 3 (not the memory 2)
    assert first.T.tolist() == [[True, False, False], [False, False, False], [True, True, False]]
    assert after["mem"][:, 0].tolist() == [4.0, 4.0, 4.0] and after["steps"].tolist() == [3, 6, 2]
    # next-step autoreset: step 1 is env 2's reset call -- it acts on the memory (its count is still 1), the memory becomes o,
    # and at step 2 the count is 0
    acts, p, first, after = href.launch(th, carry, obs0, obs, term, np.zeros_like(term), "next_step", 100.0)
    assert acts[:, 2, 0].tolist() == [2.0, 2.0, 4.0] and first[:, 2].tolist() == [True, False, True]
    assert after["pending"].tolist() == [False] * 3 and after["steps"].tolist() == [3, 6, 1]
    # disabled: the count never returns to 0
    acts, p, first, after = href.launch(th, carry, obs0, obs, term, np.zeros_like(term), "disabled", 100.0)
    assert acts[:, 2, 0].tolist() == [2.0, 2.0, 3.0] and after["steps"].tolist() == [3, 6, 3]


def test_v_zero_is_the_memoryless_policy():
    r = np.random.default_rng(1)
    th1 = ref.draw_theta(9, 3, 5)
    th2 = np.zeros((9, 3, 7), F32)
    th2[:, :, :3], th2[:, :, 6] = th1[:, :, :3], th1[:, :, 3]
    o = r.uniform(-3, 3, (4, 9, 3)).astype(F32)
    p = r.uniform(-3, 3, (4, 9, 3)).astype(F32)
    assert np.array_equal(href.history_actions(th2, o, p, 1.0).view(np.uint32), ref.linear_actions(th1, o, 1.0).view(np.uint32))


def test_header_binding_and_build_table():
    src = open(os.path.join(ROOT, "include", "mdpp.h")).read()
    for name in NEW:
        assert name in _capi.EXPORTS, name
        assert re.search(r"\b%s\s*\(mdpp_env \*h" % name, src), name
    assert re.search(r"#define\s+MDPP_ABI_VERSION\s+8\b", src) and _capi.MDPP_ABI_VERSION == 8       # new functions only
    for text in ("Linear policies with memory", "theta[.., r, D + c] = V[r][c]", "E = D (2 D + 1)",
                 "After the action is formed the memory becomes o", "HIST=2>",
                 "the memory\n *   buffer is READ AND WRITTEN at replay"):
        assert text in src, text
    for u in UNITS:
        assert u in build.SOURCES and u not in build.EXTRA_FLAGS, u              # default flags
        fam = u.replace("_summary", "").replace("_h2", "")
        assert fam in build.INCLUDED_SOURCES[u] and "mdpp_linear_history.hpp" in build.INCLUDED_SOURCES[u], u
        text = open(os.path.join(build.CSRC, u)).read()
        assert "#define MDPP_LINEAR_HIST 2" in text and ('#include "%s"' % fam) in text, u
        assert ("_SUMMARY 1" in text) == ("_summary_" in u), u
    # one statement of the act for the three agents
    for fam in ("linear", "search", "es"):
        unit = open(os.path.join(build.CSRC, "mdpp_continuous_%s.hip" % fam)).read()
        assert unit.count("linear_act_h2<DMAX>(") == 1, fam
    hdr = open(os.path.join(build.CSRC, "mdpp_linear_history.hpp")).read()
    assert hdr.count("void linear_act_h2(") == 1 and "asm" not in hdr


def test_built_library_exports_the_entry_points_and_refuses_a_null_handle():
    lib = _capi.load()
    assert len(lib.mdpp_set_linear_policy_history.argtypes) == 5 and len(lib.mdpp_linear_memory.argtypes) == 4
    buf = (C.c_float * 8)()
    p = C.cast(buf, C.c_void_p)
    assert lib.mdpp_set_linear_policy_history(None, p, 0, 2, None) == -1
    assert lib.mdpp_linear_memory(None, p, 0, None) == -1
    assert lib.mdpp_linear_policy_history(None) == 0


def test_every_new_kernel_name_parses(tmp_path):
    """The six units' code objects: every kernel is one of the six, with six literal template arguments, the last HIST = 2 --
    4 shapes x PHILOX x NOISE x PLDS = 32 per unit -- and the units of history 1 keep their five-argument names."""
    from test_kernel_spills import _unit_kernels
    for u, kernel in zip(UNITS, KERNELS):
        keys = [sx.parse_mangled(k[0]) for k in _unit_kernels(u, str(tmp_path))]
        assert len(keys) == 32 and len(set(keys)) == 32, (u, len(keys))
        for name, args in keys:
            assert name == kernel and args is not None and len(args) == 6 and args[5] == 2, (u, name, args)
        assert sorted({(a[0], a[1]) for _, a in keys}) == [(2, 2), (4, 2), (12, 1), (12, 2)], u
        old = [sx.parse_mangled(k[0]) for k in _unit_kernels(u.replace("_h2", ""), str(tmp_path))]
        mine = [a for n, a in old if n == kernel]
        assert len(mine) == 32 and all(a is not None and len(a) == 5 for a in mine), u
    # the dispatched spelling: HIST=2 after everything else
    m = re.fullmatch(r"(k_\w+)<(.*)>", "k_continuous_linear_rollout<D=4,ORDER=2,PHILOX=1,NOISE=0,PLDS=1,HIST=2>")
    assert m.group(1) == KERNELS[0] and [x.split("=")[0] for x in m.group(2).split(",")] == ["D", "ORDER", "PHILOX", "NOISE", "PLDS", "HIST"]


def test_python_objects_take_their_column_count_from_the_policy():
    import torch
    from mdp_playground_amd.linear_es import LinearES
    from mdp_playground_amd.linear_search import LinearSearch
    th = torch.arange(5 * 2 * 5, dtype=torch.float32).reshape(5, 2, 5)
    s = LinearSearch(th, 0.25, seed=3)
    assert s.cols == 5 and tuple(s.best.shape) == (10, 5) and torch.equal(s.best_theta(), th)
    assert s.best[7].tolist() == th[:, 1, 2].tolist()              # entry e = r (2 D + 1) + c
    s.check(5, 2, th.device, "t", cols=5)
    with pytest.raises(ValueError):
        s.check(5, 2, th.device, "t")                               # a history = 1 handle
    s2 = LinearSearch(torch.zeros((5, 2, 5), dtype=torch.float32), 1.0, seed=0)
    s2.load_state_dict(s.state_dict())
    assert torch.equal(s2.best, s.best)
    with pytest.raises(ValueError):
        LinearSearch(torch.zeros((5, 2, 3), dtype=torch.float32), 1.0, seed=0).load_state_dict(s.state_dict())
    m = torch.arange(2 * 3 * 7, dtype=torch.float32).reshape(2, 3, 7)
    es = LinearES(m, 0.5, 0.1, seed=1)
    assert es.cols == 7 and tuple(es.mean.shape) == (21, 2) and torch.equal(es.mean_theta(), m)
    es.check(128, 3, m.device, "t", cols=7)
    with pytest.raises(ValueError):
        es.check(128, 3, m.device, "t")
    for bad in (torch.zeros((5, 2, 4)), torch.zeros((5, 2, 6))):
        with pytest.raises(ValueError):
            LinearSearch(bad, 0.1, seed=1)
        with pytest.raises(ValueError):
            LinearES(bad[:1], 0.1, 0.1, seed=1)


# --- the figure: a double integrator needs the previous observation

_MOTIVE = dict(state_space_type="continuous", reward_function="move_to_a_point", state_space_dim=2, transition_dynamics_order=2,
               time_unit=1, inertia=1, state_space_max=10, action_space_max=1, target_point=[0, 0], target_radius=0.1,
               make_denser=True, seed=0)
GAINS = (0.01, 0.02, 0.05, 0.1, 0.2, 0.5, 1, 2)


def _run(theta, n=16, T=400, limit=100):
    """n envs on Philox streams (seed 77, env ids 1000 ..), T steps each, same-step reset; (episodes ended at the target,
    episodes ended at the limit, observations with a component on +-state_space_max)"""
    from test_linear_policy_cases_host import _oracle
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = mdp_mod.build_mdp(dict(_MOTIVE))
    at_target = at_limit = on_wall = 0
    smax = F32(m.state_space_max)
    for i in range(n):
        o = _oracle(m)
        o.set_philox(77, 1000 + i)
        obs = np.asarray(o.reset(), F32)
        mem, steps = obs.copy(), 0
        for t in range(T):
            p = obs if steps == 0 else mem
            a = href.history_actions(theta, obs[None], p[None], m.action_space_max)[0]
            mem = obs.copy()
            nxt, _, _, d = o.step(a)
            steps += 1
            nxt = np.asarray(nxt, F32)
            on_wall += int((np.abs(nxt) == smax).any())
            if d or steps >= limit:
                at_target += int(bool(d))
                at_limit += int(not d)
                nxt = np.asarray(o.reset(explicit=False), F32)
                steps = 0
            obs = nxt
    return at_target, at_limit, on_wall


def test_a_policy_with_memory_brakes_where_no_memoryless_gain_does():
    eye = np.eye(2, dtype=F32)
    zero = np.zeros((2, 2), F32)
    none = {g: _run(_theta(-F32(g) * eye, zero, [0.0, 0.0])) for g in GAINS}
    pd = _run(_theta(-F32(1.0) * eye, F32(0.8) * eye, [0.0, 0.0]))
    best = max(v[0] for v in none.values())
    print("memoryless (at target, at limit, on wall):", none)
    print("a = clip(-1.0 o + 0.8 p):", pd, " best memoryless:", best)
    assert pd[1] == 0 and pd[2] == 0, pd                # every episode ends at the target, no observation on a wall
    assert pd[0] >= 2 * best and best > 0, (pd, none)
