"""The linear policy search without a GPU: the numpy restatement (tests/linear_search_ref.py) against values worked by hand, and
the interface -- header text, bindings, stream id, build table, the Python object's argument checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import linear_search_ref as lsr
from mdp_playground_amd import _capi, build

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mdpp_step_n_linear_search", "mdpp_step_n_linear_search_summary", "mdpp_linear_search_kernel_name")


def _z(values):
    """a normals function that hands out `values` (and records the keys it was asked for)"""
    asked = []

    def normals(seed, env, tick, n):
        asked.append((seed, env, tick, n))
        return np.asarray(values, F32)[:n]
    normals.asked = asked
    return normals


def _one(theta=((1, 0, 0.5), (0, 2, 0.25)), sigma=0.5):
    return lsr.new_state(np.asarray([theta], F32), sigma)


def _end(s, ret, z, **kw):
    s["ret"][0] = ret
    kw = dict(dict(seed=9, env_id=1000, T=1), **kw)
    return lsr.end_episode(s, 0, normals=z, **kw)


def test_entry_order_and_the_start_state():
    s = _one()
    assert s["best"].shape == (6, 1) and s["best"][:, 0].tolist() == [1, 0, 0.5, 0, 2, 0.25]       # e = r (D + 1) + c
    assert s["score"][0] == -np.inf and s["trial"][0] == 0 and s["accepted"][0] == 0 and s["sigma"].dtype == F32
    z = _z([1, 2, 3, 4, 5, 6])
    assert _end(s, 1.5, z)
    # trial 0 is accepted (1.5 >= -inf); the next candidate is best + 0.5 z, entry by entry in the same order
    assert s["cand"][0].tolist() == [[1.5, 1.0, 2.0], [2.0, 4.5, 3.25]]
    assert z.asked == [(9, 1000, 1, 6)]                                  # keyed by the NEW trial index
    assert (s["score"][0], s["trial"][0], s["accepted"][0], s["acc"][0], s["ret"][0], s["eps"][0]) == (1.5, 1, 1, 0.0, 0.0, 0)


def test_no_sigma_change_at_trial_0_then_up_on_accept_down_on_reject():
    s = _one()
    z = _z([0] * 6)
    _end(s, 1.0, z, up=2.0, down=0.25)
    assert s["sigma"][0] == F32(0.5)                                     # trial 0: accepted, sigma untouched
    _end(s, 1.0, z, up=2.0, down=0.25)                                   # equal score: accepted on >=
    assert s["sigma"][0] == F32(1.0) and s["accepted"][0] == 2 and s["score"][0] == 1.0
    _end(s, 0.5, z, up=2.0, down=0.25)                                   # worse: rejected
    assert s["sigma"][0] == F32(0.25) and s["accepted"][0] == 2 and s["score"][0] == 1.0 and s["trial"][0] == 3


def test_a_rejected_candidate_leaves_the_incumbent_and_the_next_one_starts_from_it():
    s = _one()
    _end(s, 1.0, _z([1, 1, 1, 1, 1, 1]))
    best = s["best"].copy()
    assert s["cand"][0].reshape(-1).tolist() == [1.5, 0.5, 1.0, 0.5, 2.5, 0.75]
    _end(s, 0.0, _z([2, 0, 0, 0, 0, -2]))
    assert np.array_equal(s["best"], best)
    assert s["cand"][0].reshape(-1).tolist() == [2.0, 0.0, 0.5, 0.0, 2.0, -0.75]
    _end(s, 3.0, _z([0] * 6))                                            # accepted: the candidate becomes the incumbent
    assert s["best"][:, 0].tolist() == [2.0, 0.0, 0.5, 0.0, 2.0, -0.75]


def test_sigma_max_clamps_only_the_growing_branch():
    s = _one(sigma=0.5)
    z = _z([0] * 6)
    _end(s, 0.0, z)
    _end(s, 1.0, z, up=4.0, down=8.0, sigma_max=1.5)
    assert s["sigma"][0] == F32(1.5)
    _end(s, 0.0, z, up=4.0, down=8.0, sigma_max=1.5)                     # sigma * down is not clamped
    assert s["sigma"][0] == F32(12.0)


def test_a_nan_return_is_rejected_at_trial_0_too():
    s = _one()
    _end(s, np.nan, _z([1] * 6))
    assert (s["accepted"][0], s["trial"][0], s["score"][0]) == (0, 1, -np.inf)
    assert s["best"][:, 0].tolist() == [1, 0, 0.5, 0, 2, 0.25]           # the incumbent is the start policy
    assert s["cand"][0].reshape(-1).tolist() == [1.5, 0.5, 1.0, 0.5, 2.5, 0.75]
    _end(s, -7.0, _z([0] * 6), down=0.5)
    assert s["accepted"][0] == 1 and s["score"][0] == -7.0 and s["sigma"][0] == F32(0.5)      # accepted at trial 1: sigma * up


def test_trials_of_several_episodes_sum_their_returns():
    s = _one()
    z = _z([0] * 6)
    assert not _end(s, 1.0, z, T=3) and not _end(s, 2.0, z, T=3)
    assert (s["acc"][0], s["eps"][0], s["trial"][0], s["ret"][0]) == (3.0, 2, 0, 0.0) and z.asked == []
    assert _end(s, 0.25, z, T=3)
    assert (s["score"][0], s["acc"][0], s["eps"][0], s["trial"][0]) == (3.25, 0.0, 0, 1)


def test_no_fused_multiply_add_in_the_candidate():
    # sigma = z = 1 + 2^-12: the product 1 + 2^-11 + 2^-24 rounds to 1 + 2^-11, and best = -(1 + 2^-11) makes the sum 0;
    # fma(sigma, z, best) keeps the 2^-24
    w = F32(1 + 2.0 ** -12)
    b = F32(-(1 + 2.0 ** -11))
    assert lsr.perturb([b], w, [w]).tolist() == [0.0]
    assert lsr.perturb_fma([b], w, [w]).tolist() == [2.0 ** -24]


def test_run_launch_by_hand_including_the_next_step_reset_call():
    s = lsr.new_state(np.asarray([[[0, 0, 0.5], [0, 0, -0.5]]], F32), 0.5)
    obs = np.zeros((4, 1, 2), F32)
    r = np.asarray([[1.0], [2.0], [100.0], [4.0]], F32)
    te = np.asarray([[0], [1], [0], [0]], np.uint8)
    tr = np.zeros((4, 1), np.uint8)
    z = _z([1, 1, -1, 1, 1, 1])
    act, s2, pend, ended = lsr.run_launch(s, np.zeros((1, 2), F32), obs, r, te, tr, seed=1, env0=7, T=1, amax=1.0, next_step=True, normals=z)
    # steps 0, 1 under the start policy; the trial ends at step 1 with 3.0; step 2 is the reset call (not counted) and already
    # acts with the new candidate, bias 0.5 - 0.5 = 0 and -0.5 + 0.5 = 0; step 3 counts
    assert act[:, 0].tolist() == [[0.5, -0.5], [0.5, -0.5], [0.0, 0.0], [0.0, 0.0]]
    assert ended[:, 0].tolist() == [False, True, False, False] and pend.tolist() == [False]
    assert (s2["score"][0], s2["ret"][0], s2["trial"][0]) == (3.0, 4.0, 1) and z.asked == [(1, 7, 1, 6)]
    assert s["trial"][0] == 0                                            # the input state is left alone


def test_the_normals_are_the_oracles_philox_stream_18():
    from oracle import oracle as ora
    z = lsr._normals(5, 1003, 2, 7)
    assert z.dtype == F32 and np.array_equal(z, ora.philox_normals(5, 1003, 2, 18, 1, 7)[0].astype(F32))
    assert np.array_equal(z[:4], lsr._normals(5, 1003, 2, 4))            # a prefix of the same stream
    assert not np.array_equal(z, lsr._normals(5, 1003, 3, 7)) and not np.array_equal(z, lsr._normals(5, 1004, 2, 7))
    assert lsr.STREAM == 18


def test_header_binding_and_stream_id():
    src = open(os.path.join(ROOT, "include", "mdpp.h")).read()
    for name in NEW:
        assert name in _capi.EXPORTS, name
        assert re.search(r"\b%s\s*\(mdpp_env \*h" % name, src), name
    assert re.search(r"#define\s+MDPP_ABI_VERSION\s+8\b", src) and _capi.MDPP_ABI_VERSION == 8
    assert "Linear policy search" in src and "improved = (acc >= score)" in src and "stream id 18" in src
    assert "the struct travels BY VALUE" in src                          # the "HIP graphs" paragraph
    internal = open(os.path.join(build.CSRC, "mdpp_internal.hpp")).read()
    assert re.search(r"kPhiloxLinearSearchStream\s*=\s*18\b", internal)
    assert sorted(_capi.OPTIONS.values()) == [1 << k for k in range(24)]                    # no new option bit
    # the struct of the header, field for field
    m = re.search(r"typedef struct mdpp_linear_search \{(.*?)\} mdpp_linear_search;", src, re.S)
    fields = [f.strip().lstrip("*") for decl in m.group(1).split(";") if decl.strip() for f in decl.strip().split(None, 1)[1].split(",")]
    assert fields == [f for f, _ in _capi.MdppLinearSearch._fields_]
    assert C.sizeof(_capi.MdppLinearSearch) == 8 * 8 + 8 + 4 + 3 * 4


def test_build_table_has_both_units_and_the_step_has_the_hook():
    for u in ("mdpp_continuous_search.hip", "mdpp_continuous_summary_search.hip"):
        assert u in build.SOURCES and u not in build.EXTRA_FLAGS
        assert "mdpp_continuous_closed.hpp" in build.INCLUDED_SOURCES[u]
        assert os.path.exists(os.path.join(build.CSRC, u))
    assert "mdpp_continuous_search.hip" in build.INCLUDED_SOURCES["mdpp_continuous_summary_search.hip"]
    assert len([u for u in build.SOURCES if u.endswith("_summary.hip")]) == 22
    body = open(os.path.join(build.CSRC, "mdpp_continuous_closed.hpp")).read()
    assert body.count("agent.observe(rw, done || truncated);") == 1


def test_built_library_exports_the_entry_points_and_refuses_a_null_handle():
    lib = _capi.load()
    assert len(lib.mdpp_step_n_linear_search.argtypes) == 9 and len(lib.mdpp_step_n_linear_search_summary.argtypes) == 9
    assert len(lib.mdpp_linear_search_kernel_name.argtypes) == 3
    buf = (C.c_float * 8)()
    p = C.cast(buf, C.c_void_p)
    s = _capi.MdppLinearSearch()
    assert lib.mdpp_step_n_linear_search(None, 1, C.byref(s), p, p, p, p, p, None) == -1
    assert lib.mdpp_step_n_linear_search_summary(None, 1, C.byref(s), p, p, p, p, p, None) == -1
    assert lib.mdpp_linear_search_kernel_name(None, 1, 0) == b""


def test_python_object_checks_its_arguments_before_any_device_work():
    import torch
    from mdp_playground_amd.linear_search import LinearSearch
    th = torch.zeros((5, 2, 3), dtype=torch.float32)
    th[:, 0, 2] = torch.arange(5)
    s = LinearSearch(th, 0.25, seed=3, episodes_per_trial=2, sigma_up=1.5, sigma_down=0.5)
    assert tuple(s.best.shape) == (6, 5) and s.best[2].tolist() == [0, 1, 2, 3, 4] and torch.equal(s.best_theta(), th)
    assert s.sigma.tolist() == [0.25] * 5 and s.score.tolist() == [-np.inf] * 5 and s.trial.dtype == torch.int32
    assert s.sigma_max == np.inf and s.episodes_per_trial == 2
    c = s.c_struct()
    assert (c.best, c.accepted, c.seed, c.episodes_per_trial, c.sigma_up) == (s.best.data_ptr(), s.accepted.data_ptr(), 3, 2, 1.5)
    s.ret[:] = 2.0
    s.abandon_episode(torch.tensor([True, False, False, False, True]))
    assert s.ret.tolist() == [0, 2, 2, 2, 0]
    s.abandon_episode()
    assert s.ret.tolist() == [0] * 5
    d = s.state_dict()
    s2 = LinearSearch(torch.ones((5, 2, 3), dtype=torch.float32), 1.0, seed=0)
    s2.load_state_dict(d)
    assert all(torch.equal(x, y) for x, y in zip(s.tensors(), s2.tensors())) and (s2.seed, s2.episodes_per_trial, s2.sigma_up) == (3, 2, 1.5)
    sg = np.asarray([0, 0.5, 0, 1, 2], F32)
    assert LinearSearch(th, sg, seed=1).sigma.tolist() == sg.tolist()
    for bad in (dict(sigma=-0.1), dict(sigma=np.nan), dict(sigma=sg.astype(np.float64)), dict(sigma=sg[:4]),
                dict(sigma=np.asarray([0, 1, np.nan, 1, 1], F32)), dict(sigma=np.asarray([0, 1, -1, 1, 1], F32)),
                dict(episodes_per_trial=0), dict(episodes_per_trial=1.5), dict(sigma_up=-1.0), dict(sigma_down=np.nan),
                dict(sigma_up=np.inf), dict(sigma_max=-1.0), dict(sigma_max=np.nan), dict(seed=-1)):
        kw = dict(dict(sigma=0.1, seed=1), **bad)
        with pytest.raises(ValueError):
            LinearSearch(th, kw.pop("sigma"), **kw)
    for bad_theta in (th.double(), th[:, :, :2], th[0]):
        with pytest.raises(ValueError):
            LinearSearch(bad_theta, 0.1, seed=1)
