"""Eligibility traces of the learners on the host (no GPU): the restatement tests/learner_trace_ref.py against steps worked out
by hand on the 3-state chain of test_learner_host.py (alpha = gamma = lambda = 0.5 and powers of two: c = 0.25 and every
figure is exact in float32), lambda = 0 against tests/learner_ref.py bit for bit, and the header's text, the binding and the
exported names."""
import os
import re

import numpy as np
import pytest

import learner_ref
import learner_sweep_ref as ref
import learner_trace_ref as tref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GREEDY, EXPLORE = 0xFFFFFFFF, 0          # explore words: never below E <= 2^31 - 1 / below every E >= 1
A0, A1 = 0, 0x80000000                   # action words at A = 2: (w 2) >> 32 = 0 / 1
P3 = np.array([[1, 0], [2, 0], [2, 2]])  # 0 -a0-> 1 -a0-> 2 (terminal); action 1 leads back to 0
H = np.float32(0.5)


def _w(v):
    return np.array([v], np.uint32)


def _agent(algo, kind, Q=None, Z=None, lam=0.5, alpha=0.5, gamma=0.5, autoreset=ref.SAME_STEP, pending=None):
    Q = np.zeros((1, 3, 2), np.float32) if Q is None else np.asarray(Q, np.float32).reshape(1, 3, 2)
    Z = None if Z is None else np.asarray(Z, np.float32).reshape(1, 3, 2)
    return tref.TraceAgent(algo, 1, alpha, gamma, 0.5, lam, kind, Q, autoreset, Z=Z, pending=pending)


def _step(ag, s, we, wa, r, s2, te=False, tr=False, we1=GREEDY, wa1=A0):
    a = ag.act(np.array([s]), _w(we), _w(wa))
    ag.learn(np.array([s]), a, np.array([r], np.float32), np.array([s2]), np.array([te]), np.array([tr]), _w(we1), _w(wa1))
    return int(a[0])


# ---- (a) accumulating against replacing on a revisit within an episode
@pytest.mark.parametrize("kind,z_after,q_after", [(tref.ACCUMULATING, 0.3125, 0.96875), (tref.REPLACING, 0.25, 0.875)])
def test_a_revisit_accumulates_or_replaces(kind, z_after, q_after):
    """sarsa (no cut), state 0, action 1 twice (it leads back to 0), r = 1:
    step 1: y = 1 + 0.5 Q[0][1] = 1, d = 1, u = 0.5; mark Z[0][1] = 1; sweep Q[0][1] = 0.5, Z[0][1] = 0.25
    step 2: y = 1 + 0.5 0.5 = 1.25, d = 0.75, u = 0.375; accumulating marks 0.25 + 1 = 1.25 = 1 + c, replacing 1:
            Q[0][1] = 0.5 + 0.375 1.25 = 0.96875 / 0.5 + 0.375 = 0.875;  Z[0][1] = 0.25 1.25 = 0.3125 / 0.25"""
    ag = _agent("sarsa", kind)
    ag.launch_start()
    assert _step(ag, 0, EXPLORE, A1, 1.0, 0, we1=EXPLORE, wa1=A1) == 1
    assert ag.Q[0, 0, 1] == 0.5 and ag.Z[0, 0, 1] == 0.25 and ag.info["above_one"] == 0
    assert _step(ag, 0, GREEDY, A0, 1.0, 0, we1=EXPLORE, wa1=A1) == 1          # (the carried a', not the greedy word's choice)
    assert ag.Q[0, 0, 1] == np.float32(q_after) and ag.Z[0, 0, 1] == np.float32(z_after)
    assert ag.info["above_one"] == (kind == tref.ACCUMULATING) and ag.info["carried"] == 1
    assert np.count_nonzero(ag.Q) == 1 and np.count_nonzero(ag.Z) == 1


# ---- (b) the sweep reaches every entry; the product is rounded, then the sum
def test_sweep_rounds_the_product_then_the_sum():
    """u = z = 1 + 2^-12: u z = 1 + 2^-11 + 2^-24 rounds (to even) to 1 + 2^-11, so Q[e] = -(1 + 2^-11) becomes exactly 0; a
    fused multiply-add would leave 2^-24.  u = alpha d with alpha = 1, a terminal step (y = r) and q = 0: u = r."""
    x = np.float32(1.0 + 2.0 ** -12)
    qe = np.float32(-(1.0 + 2.0 ** -11))
    assert np.float32(np.float64(x) * np.float64(x) + np.float64(qe)) == np.float32(2.0 ** -24)      # what an FMA gives
    Q = np.zeros((3, 2), np.float32); Z = np.zeros((3, 2), np.float32)
    Q[0, 1], Z[0, 1] = qe, x                  # an entry that is not the step's (s, a) = (1, 0)
    Q[2, 1], Z[2, 1] = 3.0, 2.0               # the last entry of the table
    ag = _agent("sarsa", tref.REPLACING, Q, Z, alpha=1.0)
    ag.launch_start()
    _step(ag, 1, GREEDY, A0, x, 2, te=True)
    assert ag.info["ends"] == 1
    assert ag.Q[0, 0, 1] == 0.0 and not np.signbit(ag.Q[0, 0, 1])
    assert ag.Q[0, 1, 0] == x                                                   # q + u 1
    assert ag.Q[0, 2, 1] == np.float32(3.0) + np.float32(x * np.float32(2.0))   # ... and the last entry was swept
    assert not ag.Z.any()                                                       # (terminated: zeroed after the sweep)


# ---- (c), (d) the cut
@pytest.mark.parametrize("algo,we,z_other", [("q_learning", EXPLORE, 0.0), ("q_learning", GREEDY, 0.125), ("sarsa", EXPLORE, 0.125)])
def test_cut_on_the_explore_branch_only_and_never_for_sarsa(algo, we, z_other):
    """Q[0] = [1, 0]: greedy is action 0, and the exploring step draws action 0 too -- it cuts all the same.  Z[1][0] = 0.5
    beforehand: cut -> 0, else c 0.5 = 0.125; the marked entry ends at c = 0.25 either way"""
    Q = np.zeros((3, 2), np.float32); Z = np.zeros((3, 2), np.float32)
    Q[0, 0], Z[1, 0] = 1.0, 0.5
    ag = _agent(algo, tref.ACCUMULATING, Q, Z)
    ag.launch_start()
    assert _step(ag, 0, we, A0, 0.0, 1) == 0
    assert ag.Z[0, 1, 0] == np.float32(z_other) and ag.Z[0, 0, 0] == 0.25
    cut = algo == "q_learning" and we == EXPLORE
    assert ag.info["cuts"] == cut and ag.info["cut_greedy_action"] == cut
    # y = 0 + 0.5 max Q[1] = 0, d = -1, u = -0.5: Q[0][0] = 1 - 0.5 = 0.5; Q[1][0] = 0 + (-0.5) z
    assert ag.Q[0, 0, 0] == 0.5 and ag.Q[0, 1, 0] == (0.0 if cut else -0.25)


# ---- (e) episode ends
@pytest.mark.parametrize("te,tr", [(True, False), (False, True)])
@pytest.mark.parametrize("autoreset", [ref.SAME_STEP, ref.NEXT_STEP, ref.DISABLED])
def test_traces_are_zeroed_at_termination_and_at_truncation_after_the_sweep(te, tr, autoreset):
    Z = np.full((3, 2), 0.5, np.float32)
    ag = _agent("q_learning", tref.REPLACING, Z=Z, autoreset=autoreset)
    ag.launch_start()
    _step(ag, 1, GREEDY, A0, 1.0, 2 if te else 0, te=te, tr=tr)
    assert not ag.Z.any() and not np.signbit(ag.Z).any() and ag.info["ends"] == 1
    # the sweep came first: y = 1 (+ 0), u = 0.5: Q[e] = 0.5 0.5 = 0.25 elsewhere, 0.5 at (1, 0)
    want = np.full((3, 2), 0.25, np.float32); want[1, 0] = 0.5
    assert np.array_equal(ag.Q[0], want)
    assert ag.pending[0] == (autoreset == ref.NEXT_STEP)


# ---- (f) a reset call
def test_a_reset_call_touches_neither_table():
    rs = np.random.default_rng(1)
    Q, Z = rs.normal(size=(3, 2)).astype(np.float32), rs.random((3, 2)).astype(np.float32)
    ag = _agent("q_learning", tref.ACCUMULATING, Q, Z, autoreset=ref.NEXT_STEP, pending=[True])
    ag.launch_start()
    _step(ag, 1, EXPLORE, A1, 5.0, 0, te=True)
    assert np.array_equal(ag.Q[0].view(np.int32), Q.view(np.int32)) and np.array_equal(ag.Z[0].view(np.int32), Z.view(np.int32))
    assert not ag.pending[0] and ag.info["updates"] == 0 and ag.info["cuts"] == 0 and ag.info["reset_calls"] == 1


# ---- (g) denormal traces
def test_a_trace_decays_into_the_denormal_range_and_is_still_applied():
    """Z[2][1] = 2^-126 (the smallest normal): the sweep leaves c z = 2^-128, a denormal; the next sweep adds u 2^-128 to Q[2][1]"""
    Z = np.zeros((3, 2), np.float32)
    Z[2, 1] = np.float32(2.0 ** -126)
    ag = _agent("sarsa", tref.REPLACING, Z=Z, alpha=1.0)
    ag.launch_start()
    _step(ag, 0, GREEDY, A0, 0.0, 1)
    assert ag.Z[0, 2, 1] == np.float32(2.0 ** -128) and ag.Z[0, 2, 1] != 0 and ag.info["denormal_traces"] == 1
    _step(ag, 1, GREEDY, A0, 1.0, 0)                          # y = 1, u = 1
    assert ag.Q[0, 2, 1] == np.float32(2.0 ** -128) and ag.Q[0, 2, 1] != 0
    assert ag.Z[0, 2, 1] == np.float32(2.0 ** -130)


# ---- (h) lambda = 0 is the traceless learner
@pytest.mark.parametrize("kind", tref.KINDS)
@pytest.mark.parametrize("autoreset", [ref.SAME_STEP, ref.NEXT_STEP, ref.DISABLED])
@pytest.mark.parametrize("algo", ["q_learning", "sarsa"])
def test_lambda_0_equals_learner_ref_bit_for_bit(algo, autoreset, kind):
    """a made-up launch (the step's outputs are inputs): 24 envs, 60 steps, S = 5, A = 3, positive rewards from zero tables,
    so Q holds no -0"""
    rs = np.random.default_rng(7)
    n, K, S, A = 24, 60, 5, 3
    P = rs.integers(0, S, (S, A))
    obs0, obs = rs.integers(0, S, n), rs.integers(0, S, (K, n))
    rew = rs.random((K, n)).astype(np.float32)
    term, trunc = rs.random((K, n)) < 0.1, rs.random((K, n)) < 0.1
    w_e, w_a = (rs.integers(0, 2 ** 32, (K + 1, n), dtype=np.uint64).astype(np.uint32) for _ in range(2))
    act0, Q0, pending0, info0 = learner_ref.run(algo, 0.3, 0.9, 0.25, np.zeros((n, S, A), np.float32), obs0, obs, rew, term, trunc, P, autoreset, w_e, w_a)
    ag = tref.TraceAgent(algo, n, 0.3, 0.9, 0.25, 0.0, kind, np.zeros((n, S, A), np.float32), autoreset)
    act = tref.run(ag, obs0, obs, rew, term, trunc, P, w_e, w_a)
    assert np.array_equal(act, act0) and np.array_equal(ag.Q.view(np.int32), Q0.view(np.int32)) and np.array_equal(ag.pending, pending0)
    assert not ag.Z.any() and (Q0 != 0).any() and not np.signbit(Q0[Q0 == 0]).any()
    assert info0["explored"] > 0 and info0["updates"] > 0 and (algo != "sarsa" or info0["carried_differs"] > 0)


def test_per_env_lambda_and_c():
    ag = tref.TraceAgent("sarsa", 3, 0.5, [0.5, 1.0, 0.25], 0.5, [1.0, 0.3, 0.0], tref.REPLACING, np.zeros((3, 3, 2), np.float32), ref.SAME_STEP)
    ag.launch_start()
    s = np.zeros(3, np.int64)
    a = ag.act(s, np.full(3, GREEDY, np.uint32), np.zeros(3, np.uint32))
    ag.learn(s, a, np.ones(3, np.float32), np.ones(3, np.int64), np.zeros(3, bool), np.zeros(3, bool), np.full(3, GREEDY, np.uint32), np.zeros(3, np.uint32))
    assert np.array_equal(ag.Z[:, 0, 0], np.array([0.5, 1.0, 0.25], np.float32) * np.array([1.0, 0.3, 0.0], np.float32))


# ---- the header, the binding, the exported names, the build
def test_the_header_states_the_rules_and_the_abi_is_bound():
    from mdp_playground_amd import _capi, build
    src = open(os.path.join(ROOT, "include", "mdpp.h")).read()
    flat = re.sub(r"\s*\n \*\s*", " ", src)
    for text in ("Eligibility traces: SARSA(lambda) and Watkins's Q(lambda)", "MDPP_TRACE_ACCUMULATING = 1, MDPP_TRACE_REPLACING = 2",
                 "cut (q_learning only)", "accumulating Z[s][a] = Z[s][a] + 1.0f; replacing Z[s][a] = 1.0f",
                 "z = Z[e]; Q[e] = Q[e] + u z (the product is rounded, then the sum); Z[e] = c z",
                 "Denormal traces are kept, not flushed", "mdpp_set_q leaves Z alone",
                 "Z is READ AND WRITTEN in the handle's buffer at replay"):
        assert text in flat, text
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = {"mdpp_set_learner_traces": 4, "mdpp_set_learner_lambda": 3, "mdpp_clear_learner_traces": 1, "mdpp_get_traces": 3,
              "mdpp_set_traces": 3, "mdpp_learner_traces": 1}
    lib = _capi.load()
    for name, nargs in protos.items():
        assert name in _capi.EXPORTS
        proto = re.search(r"int %s\s*\(([^)]*)\)" % name, code)
        assert proto and len(proto.group(1).split(",")) == nargs, name
        assert len(getattr(lib, name).argtypes) == nargs, name
    assert _capi.TRACE_KINDS == {"accumulating": 1, "replacing": 2}
    assert _capi.MDPP_ABI_VERSION == 8 and "#define MDPP_ABI_VERSION 8" in src        # (entry points were added, nothing moved)
    assert lib.mdpp_set_learner_traces(None, 1, 0.5, None) == -1 and lib.mdpp_learner_traces(None) == 0
    units = [s for s in build.SOURCES if "trace" in s]
    assert sorted(units) == sorted(["mdpp_discrete_trace.hip", "mdpp_discrete_trace_pe.hip", "mdpp_discrete_trace_pe_sched.hip",
                                    "mdpp_discrete_summary_trace.hip", "mdpp_discrete_summary_trace_pe.hip", "mdpp_discrete_summary_trace_pe_sched.hip"])
    for u in units:
        assert os.path.exists(os.path.join(build.CSRC, u)) and u not in build.EXTRA_FLAGS
        assert "mdpp_discrete_trace.hpp" in build.INCLUDED_SOURCES[u]


def test_the_python_layer_validates_before_the_library_is_reached():
    from mdp_playground_amd import policy
    assert policy.learner_param_array("lam", 0.5, 4) is None
    assert policy.learner_param_array("lam", [0.0, 1.0, 0.5, 0.25], 4).dtype == np.float32
    for bad in ([0.5, 1.5, 0.0, 0.0], [0.5, float("nan"), 0.0, 0.0], [0.5] * 3, [[0.5] * 4]):
        with pytest.raises(ValueError):
            policy.learner_param_array("lam", bad, 4)
