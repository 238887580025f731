"""The linear policy of closed-loop continuous rollouts, without a GPU: the numpy restatement (tests/linear_policy_ref.py) against
values worked by hand, and the interface -- header, binding, build table, the built library's exports."""
import ctypes as C
import os
import re

import numpy as np

import linear_policy_ref as ref
from mdp_playground_amd import _capi, build

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mdpp_set_linear_policy", "mdpp_get_linear_policy", "mdpp_clear_linear_policy", "mdpp_step_n_linear",
       "mdpp_step_n_linear_summary", "mdpp_linear_kernel_name")


def _act(theta, o, amax=1.0):
    return ref.linear_actions(np.asarray(theta, F32), np.asarray([o], F32), amax)[0]


def test_clipped_and_unclipped_components():
    # a0 = 0.5 + 1 * 0.25 + 0 * 3 = 0.75; a1 = 0 + 0 * 0.25 + 2 * 3 = 6 -> 1; and the lower bound
    a = _act([[1, 0, 0.5], [0, 2, 0]], [0.25, 3.0])
    assert a.dtype == F32 and a.tolist() == [0.75, 1.0]
    assert _act([[1, 0, 0.5], [0, -2, 0]], [0.25, 3.0]).tolist() == [0.75, -1.0]
    assert _act([[1, 0, 0.5], [0, 2, 0]], [0.25, 3.0], amax=8.0).tolist() == [0.75, 6.0]


def test_nan_passes_through():
    a = _act([[1, 0, np.nan], [0, 1, 0]], [0.25, 0.5])
    assert np.isnan(a[0]) and a[1] == F32(0.5)
    a = _act([[1, 0, 0], [0, 1, 0]], [np.nan, 0.5])     # (0 * NaN is NaN: a NaN observation reaches every row)
    assert np.isnan(a[0]) and np.isnan(a[1])


def test_summation_order_is_bias_first_then_columns_left_to_right():
    # b = 1e8, W o = (1, -1e8): (1e8 + 1) rounds to 1e8 in float32, then - 1e8 = 0; any other order gives 1
    a = _act([[1, 1, 1e8], [0, 0, 0]], [1.0, -1e8], amax=10.0)
    assert a.tolist() == [0.0, 0.0]
    assert (F32(1e8) + F32(-1e8)) + F32(1.0) == F32(1.0)                  # the order that is NOT the policy's


def test_no_fused_multiply_add():
    # w = o = 1 + 2^-12: w o = 1 + 2^-11 + 2^-24 rounds (to even) to 1 + 2^-11, and b = -(1 + 2^-11) makes the sum 0;
    # fma(w, o, b) keeps the 2^-24
    w = F32(1 + 2.0 ** -12)
    b = F32(-(1 + 2.0 ** -11))
    a = _act([[w, 0, b], [0, 0, 0]], [w, 0.0])
    assert a.tolist() == [0.0, 0.0]
    assert float(w) * float(w) + float(b) == 2.0 ** -24


def test_per_env_and_shared_parameters_and_leading_axes():
    th = ref.draw_theta(5, 3, seed=1)
    o = np.random.default_rng(2).uniform(-3, 3, (4, 5, 3)).astype(F32)
    a = ref.linear_actions(th, o, 1.0)
    for k in range(4):
        for i in range(5):
            assert np.array_equal(a[k, i], ref.linear_actions(th[i], o[k, i][None], 1.0)[0])
    assert not np.array_equal(ref.linear_actions(th[0], o[0], 1.0)[1], a[0, 1])       # env 0's parameters are not env 1's


def test_summary_rule_by_hand():
    r = np.asarray([[1.0], [2.0], [0.5], [4.0]], F32)
    te = np.asarray([[0], [1], [0], [0]], np.uint8)
    tr = np.asarray([[0], [0], [0], [1]], np.uint8)
    s, pend = ref.summarise(ref.new_summary(1), r, te, tr)
    assert (s["episodes"][0], s["return_sum"][0], s["length_sum"][0], s["ret"][0], s["len"][0]) == (2, 7.5, 4, 0.0, 0)
    # next-step autoreset: step 2 is the reset call (its reward is not counted, nor its step)
    s, pend = ref.summarise(ref.new_summary(1), r, te, tr, next_step=True)
    assert (s["episodes"][0], s["return_sum"][0], s["length_sum"][0], s["ret"][0], s["len"][0]) == (2, 7.0, 3, 0.0, 0)
    assert pend.tolist() == [True]
    s2, pend = ref.summarise(s, r[:1], te[:1], tr[:1], next_step=True, pending=pend)
    assert (s2["ret"][0], s2["len"][0]) == (0.0, 0) and pend.tolist() == [False]


def test_header_binding_and_option_bit():
    src = open(os.path.join(ROOT, "include", "mdpp.h")).read()
    for name in NEW:
        assert name in _capi.EXPORTS, name
        assert re.search(r"\b%s\s*\(mdpp_env \*h" % name, src), name
    assert re.search(r"#define\s+MDPP_ABI_VERSION\s+8\b", src) and _capi.MDPP_ABI_VERSION == 8
    assert re.search(r"MDPP_OPT_NO_LINEAR_LDS\s*=\s*1u\s*<<\s*23\b", src)
    assert _capi.OPTIONS["NO_LINEAR_LDS"] == 1 << 23
    assert sorted(_capi.OPTIONS.values()) == [1 << k for k in range(24)]        # bit 23 was free, and every bit has one name
    assert "the parameter buffer is READ at replay" in src            # the "HIP graphs" paragraph


def test_build_table_has_both_units_and_their_header():
    for u in ("mdpp_continuous_linear.hip", "mdpp_continuous_summary_linear.hip"):
        assert u in build.SOURCES
        assert "mdpp_continuous_closed.hpp" in build.INCLUDED_SOURCES[u]
        assert os.path.exists(os.path.join(build.CSRC, u))
    assert "mdpp_continuous_linear.hip" in build.INCLUDED_SOURCES["mdpp_continuous_summary_linear.hip"]
    assert os.path.exists(os.path.join(build.CSRC, "mdpp_continuous_closed.hpp"))
    # the open-loop kernel's unit does not include the closed-loop step: its code cannot have changed
    assert "mdpp_continuous_closed.hpp" not in open(os.path.join(build.CSRC, "mdpp_continuous.hip")).read()


def test_built_library_exports_the_entry_points_and_refuses_a_null_handle():
    lib = _capi.load()
    EINVAL = -1
    src = open(os.path.join(ROOT, "include", "mdpp.h")).read()
    assert re.search(r"MDPP_EINVAL\s*=\s*-1\b", src)
    assert len(lib.mdpp_step_n_linear.argtypes) == 8 and len(lib.mdpp_step_n_linear_summary.argtypes) == 8
    assert len(lib.mdpp_set_linear_policy.argtypes) == 4 and len(lib.mdpp_linear_kernel_name.argtypes) == 3
    buf = (C.c_float * 8)()
    p = C.cast(buf, C.c_void_p)
    assert lib.mdpp_set_linear_policy(None, p, 0, None) == EINVAL
    assert lib.mdpp_get_linear_policy(None, p, None) == EINVAL
    assert lib.mdpp_clear_linear_policy(None) == EINVAL
    assert lib.mdpp_step_n_linear(None, 1, p, p, p, p, p, None) == EINVAL
    assert lib.mdpp_step_n_linear_summary(None, 1, p, p, p, p, p, None) == EINVAL
    assert lib.mdpp_linear_kernel_name(None, 1, 0) == b""
