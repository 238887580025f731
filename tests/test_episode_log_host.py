"""The episode log on the host (no GPU): the restatement tests/episode_log_ref.py on short sequences worked out by hand, its
two exact invariants, EpisodeLog's clear() / filled() / episodes_of() / curve() on CPU tensors, the names of the C ABI and the
entry points' argument refusals as far as they run without a device, and a CPU closed loop (the oracle env, 32 envs, K = 37,
two launches) showing that the M of every case is the median it is said to be and that what tests/test_gpu_episode_log.py
asserts about its own coverage can be met by every (case, algorithm) it runs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import episode_log_cases as cases
import episode_log_ref as lref
import eval_summary_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _f32(*rows):
    return np.array(rows, np.float32)


def _i64(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


# ---- (a) the rule by hand
def test_rule_by_hand_termination_truncation_a_skipped_reset_call_an_episode_across_two_launches_the_cap_and_a_pop():
    # the sequences of tests/test_eval_summary_host.py's hand-worked summary:
    # env 0: r = 1, 2 (terminated) | 0.5, 0.25, 4 (truncated) | 8 ...            -> launch 2: 16 (terminated)
    # env 1: r = 1 (terminated) | reset call (its row is skipped) | 2, 3, 0     -> launch 2: 5, then 7 (truncated)
    rew = _f32([1, 1], [2, 0], [0.5, 2], [0.25, 3], [4, 0], [8, 0])
    term = np.array([[0, 1], [1, 0], [0, 0], [0, 0], [0, 0], [0, 0]], bool)
    trunc = np.array([[0, 0], [0, 0], [0, 0], [0, 0], [1, 0], [0, 0]], bool)
    rc = np.array([[0, 0], [0, 1], [0, 0], [0, 0], [0, 0], [0, 0]], bool)
    rew[5, 1], rc[5, 1] = 100.0, True          # (a reset call's row never counts, whatever it holds)
    c = lref.new_counters()
    log0 = lref.new_log(2, 2, cases.SENTINEL_RET, cases.SENTINEL_LEN)
    lg, st = lref.run(rew, term, trunc, rc, lref.new_state5(2), log0, c)
    assert lg["count"].tolist() == [2, 1]
    assert lg["ret"].tolist() == [[3.0, 1.0], [4.75, cases.SENTINEL_RET]]             # episode-major: row m, env i
    assert lg["len"].tolist() == [[2, 1], [3, cases.SENTINEL_LEN]]                    # the unwritten entry keeps what it held
    assert st["episodes"].tolist() == [2, 1] and st["return_sum"].tolist() == [7.75, 1.0] and st["length_sum"].tolist() == [5, 1]
    assert st["ret"].tolist() == [8.0, 5.0] and st["len"].tolist() == [1, 3]
    assert c == dict(over_M=0, under_M=1, zero=0, spanning_logged=0, wave_rows_differ=0, ended_terminated=2, ended_truncated=1, reset_calls=2)
    assert log0["count"].tolist() == [0, 0] and (log0["len"] == cases.SENTINEL_LEN).all()     # (the state handed in is not modified)
    # a pop() between the launches: the three sums leave, the log does not move and goes on from its own count
    st = lref.pop5(st)
    assert st["episodes"].tolist() == [0, 0] and st["ret"].tolist() == [8.0, 5.0]
    lg2, st2 = lref.run(_f32([16, 5], [0, 7]), np.array([[1, 0], [0, 0]], bool), np.array([[0, 0], [0, 1]], bool), np.zeros((2, 2), bool), st, lg, c)
    # env 0's third episode (8 + 16, two steps) finds the log full: count goes on, nothing is written; env 1's second (5 + 5 + 7,
    # five steps: it began in launch 1) takes row 1
    assert lg2["count"].tolist() == [3, 2]
    assert lg2["ret"].tolist() == [[3.0, 1.0], [4.75, 17.0]] and lg2["len"].tolist() == [[2, 1], [3, 5]]
    assert st2["episodes"].tolist() == [1, 1] and st2["return_sum"].tolist() == [24.0, 17.0] and st2["length_sum"].tolist() == [2, 5]
    assert c["over_M"] == 1 and c["under_M"] == 0 and c["spanning_logged"] == 1 and c["ended_truncated"] == 2
    assert lg2["count"].dtype == np.int32 and lg2["ret"].dtype == np.float64 and lg2["len"].dtype == np.int32


def test_capacity_one_keeps_the_first_episode_and_terminated_with_truncated_is_one_episode():
    rew = _f32([1], [2], [4], [8])
    end = np.array([[1], [0], [1], [1]], bool)
    lg, st = lref.run(rew, end, end, np.zeros((4, 1), bool), lref.new_state5(1), lref.new_log(1, 1))
    assert lg["count"].tolist() == [3] and lg["ret"].tolist() == [[1.0]] and lg["len"].tolist() == [[1]]
    assert st["episodes"].tolist() == [3] and st["return_sum"].tolist() == [15.0]


def test_the_five_summary_values_are_eval_summary_refs_and_the_two_invariants_hold_bit_for_bit():
    rs = np.random.default_rng(5)
    n, K, M = 70, 29, 6
    st, lg, st_ref, c = lref.new_state5(n), lref.new_log(n, M), sref.new_state5(n), lref.new_counters()
    pending = None
    for launch in range(3):
        # rewards whose float64 sums round: the order of the additions shows in the last bit
        rew = (rs.normal(size=(K, n)) * 10.0 ** rs.integers(-6, 7, size=(K, n))).astype(np.float32)
        term, trunc = rs.random((K, n)) < 0.08, rs.random((K, n)) < 0.05
        rc, pending = sref.reset_calls(term, trunc, sref.NEXT_STEP, pending)
        lg, st = lref.run(rew, term, trunc, rc, st, lg, c)
        st_ref = sref.summary(rew, term, trunc, rc, st_ref)
        for name, dt in sref.FIELDS:
            g, w = st[name], st_ref[name]
            assert g.dtype == dt and np.array_equal(_i64(g) if dt == np.float64 else g, _i64(w) if dt == np.float64 else w), (launch, name)
    assert c["over_M"] > 0 and c["under_M"] > 0 and c["reset_calls"] > 0 and c["spanning_logged"] > 0 and c["wave_rows_differ"] > 0
    # zeroed together, no pop(): count == episodes; length_sum and return_sum are the log's sums wherever the log is complete
    assert np.array_equal(lg["count"], st["episodes"])
    whole = lg["count"] <= M
    assert whole.any() and (~whole).any()
    for i in range(n):
        filled = min(int(lg["count"][i]), M)
        if whole[i]:
            assert int(lg["len"][:filled, i].sum()) == int(st["length_sum"][i])
            assert _i64(lref.left_to_right_sum(lg, i)) == _i64(st["return_sum"][i]), i
        else:
            assert int(lg["len"][:filled, i].sum()) < int(st["length_sum"][i])
    # (the order matters: a pairwise or reversed sum of the same entries misses some env's last bit)
    assert any(_i64(lg["ret"][:int(lg["count"][i]), i][::-1].sum()) != _i64(st["return_sum"][i]) for i in np.flatnonzero(whole))


# ---- (b) EpisodeLog on CPU tensors
def test_episode_log_clear_filled_episodes_of_and_check_on_cpu_tensors():
    import torch
    from mdp_playground_amd.summary import EpisodeLog
    lg = EpisodeLog(3, 4, "cpu")
    assert [t.dtype for t in lg.tensors()] == [torch.int32, torch.float64, torch.int32]
    assert [tuple(t.shape) for t in lg.tensors()] == [(3,), (4, 3), (4, 3)] and all(not t.any() for t in lg.tensors())
    assert all(t is x for t, x in zip(lg.tensors(), (lg.count, lg.ret, lg.len))) and all(t.is_contiguous() for t in lg.tensors())
    lg.count[:] = torch.tensor([2, 0, 9])
    lg.ret[:, 0] = torch.tensor([1.5, 2.5, 77.0, 77.0])
    lg.len[:, 0] = torch.tensor([3, 4, 77, 77])
    lg.ret[:, 2] = torch.tensor([1.0, 2.0, 3.0, 4.0])
    lg.len[:, 2] = torch.tensor([1, 2, 3, 4])
    assert lg.filled().tolist() == [2, 0, 4] and lg.filled().dtype == torch.int32
    r, ln = lg.episodes_of(0)
    assert isinstance(r, np.ndarray) and r.dtype == np.float64 and ln.dtype == np.int32
    assert r.tolist() == [1.5, 2.5] and ln.tolist() == [3, 4]
    assert [x.tolist() for x in lg.episodes_of(1)] == [[], []]
    assert [x.tolist() for x in lg.episodes_of(2)] == [[1.0, 2.0, 3.0, 4.0], [1, 2, 3, 4]]
    lg.check(3, torch.device("cpu"), "t")
    for bad in (lambda: lg.check(4, torch.device("cpu"), "t"), lambda: lg.check(3, torch.device("meta"), "t")):
        with pytest.raises(ValueError):
            bad()
    lg.clear()
    assert all(not t.any() for t in lg.tensors())
    lg.len = lg.len.to(torch.int64)
    with pytest.raises(ValueError, match="log.len"):
        lg.check(3, torch.device("cpu"), "t")
    lg = EpisodeLog(3, 4, "cpu")
    lg.ret = torch.zeros((3, 4), dtype=torch.float64).t()                # the right shape, env-major underneath
    with pytest.raises(ValueError, match="log.ret"):
        lg.check(3, torch.device("cpu"), "t")
    for n, m in ((3, 0), (3, -1), (2 ** 16, 2 ** 15)):
        with pytest.raises(ValueError):
            EpisodeLog(n, m, "meta")
    assert EpisodeLog(2 ** 16 - 1, 2 ** 15, "meta").ret.shape == (2 ** 15, 2 ** 16 - 1)


def test_curve_counts_the_envs_that_reached_a_row_with_groups_and_a_row_nobody_reached():
    import torch
    from mdp_playground_amd.summary import EpisodeLog
    lg = EpisodeLog(4, 3, "cpu")
    lg.count[:] = torch.tensor([2, 1, 5, 0])                              # env 2 ran past the cap, env 3 ended none
    lg.ret[:] = torch.tensor([[1.0, 3.0, 5.0, 99.0], [2.0, 99.0, 7.0, 99.0], [99.0, 99.0, 9.0, 99.0]])
    lg.len[:] = torch.tensor([[1, 3, 5, 99], [2, 99, 7, 99], [99, 99, 9, 99]])
    n, mr, ml = lg.curve()
    assert n.tolist() == [3, 2, 1] and mr.tolist() == [3.0, 4.5, 9.0] and ml.tolist() == [3.0, 4.5, 9.0]
    assert mr.dtype == torch.float64 and tuple(mr.shape) == (3,)
    n, mr, ml = lg.curve(groups=[0, 0, 1, 1])
    assert n.tolist() == [[2, 1], [1, 1], [0, 1]]
    assert mr[:2].tolist() == [[2.0, 5.0], [2.0, 7.0]] and ml[:2].tolist() == [[2.0, 5.0], [2.0, 7.0]]
    assert torch.isnan(mr[2, 0]) and torch.isnan(ml[2, 0]) and mr[2, 1] == 9.0        # a row nobody of group 0 reached
    n, mr, _ = lg.curve(groups=torch.tensor([2, 2, 0, 0]), num_groups=4)
    assert tuple(n.shape) == (3, 4) and n[:, 1].tolist() == [0, 0, 0] and n[:, 3].tolist() == [0, 0, 0] and torch.isnan(mr[:, 1]).all()
    assert n[:, 2].tolist() == [2, 1, 0] and n[:, 0].tolist() == [1, 1, 1]
    lg.count[2] = 0
    n, mr, _ = lg.curve()
    assert n.tolist() == [2, 1, 0] and torch.isnan(mr[2])
    for bad in ([0, 1], [0, 0, 1, 5]):
        with pytest.raises(ValueError):
            lg.curve(groups=bad, num_groups=2)
    # episodes_of feeds stats_csv's evaluation rows
    from mdp_playground_amd import stats_csv
    assert hasattr(stats_csv.StatsWriter, "write_eval_episode")


# ---- (c) names and refusals
def test_the_entry_point_is_declared_exported_and_bound_and_nothing_else_of_the_abi_moved():
    from mdp_playground_amd import _capi, build
    src = open(os.path.join(ROOT, "include", "mdpp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert "mdpp_step_n_eval_log" not in _capi.EXPORTS and "mdpp_step_n_eval_log" not in src        # (no log under evaluation)
    for name in ("mdpp_step_n_learn_log",):
        assert name in _capi.EXPORTS
        proto = re.search(r"int %s\s*\(([^)]*)\)" % name, code)
        assert proto and len(proto.group(1).split(",")) == 12, name
    lib = _capi.load()
    assert len(lib.mdpp_step_n_learn_log.argtypes) == 12
    assert len(lib.mdpp_step_n_learn_summary.argtypes) == 8 and len(lib.mdpp_step_n_eval_summary.argtypes) == 8
    assert _capi.MDPP_ABI_VERSION == 8 and "#define MDPP_ABI_VERSION 8" in src
    assert not any("log" in s for s in build.SOURCES)                     # no translation unit was added
    assert len([s for s in build.SOURCES if s.endswith("_summary.hip")]) == 22


def test_the_entry_point_refuses_a_null_handle_and_the_python_layer_its_arguments_before_any_device_work():
    import torch
    from mdp_playground_amd import _capi
    from mdp_playground_amd.summary import EpisodeLog, EpisodeSummary
    from mdp_playground_amd.vector_env import RLToyVectorEnv
    lib = _capi.load()
    for fn in (lib.mdpp_step_n_learn_log,):
        assert fn(None, 4, *([None] * 8), 3, None) == -1                  # MDPP_EINVAL: no handle
    # the Python checks come before the library is reached: an object that has only what they read
    class Stub:
        num_envs, device, kind = 5, torch.device("cpu"), "discrete"
        _learn_check_kind = lambda self: None
        _rollout_summary = RLToyVectorEnv._rollout_summary
        _lib = lib
        _h = None

        def _stream(self):
            raise AssertionError("the library was reached")
    env, summ = Stub(), EpisodeSummary(5, "cpu")
    strided = EpisodeLog(5, 3, "cpu")
    strided.len = torch.zeros((3, 10), dtype=torch.int32)[:, ::2]
    wrong = EpisodeLog(5, 3, "cpu")
    wrong.count = wrong.count.to(torch.int64)
    with pytest.raises(TypeError):                                        # rollout_eval keeps no log
        RLToyVectorEnv.rollout_eval(env, 4, summary=summ, log=EpisodeLog(5, 3, "cpu"))
    for call in (RLToyVectorEnv.rollout_learn,):
        with pytest.raises(ValueError, match="log goes with summary"):
            call(env, 4, log=EpisodeLog(5, 3, "cpu"))
        with pytest.raises(ValueError, match="log goes with summary"):
            call(env, 4, out=(), summary=summ, log=EpisodeLog(5, 3, "cpu"))
        for bad in (EpisodeLog(4, 3, "cpu"), EpisodeLog(5, 3, "meta"), strided, wrong, "log", (1, 2, 3)):
            with pytest.raises(ValueError):
                call(env, 4, summary=summ, log=bad)
        with pytest.raises(AssertionError, match="the library was reached"):
            call(env, 4, summary=summ, log=EpisodeLog(5, 3, "cpu"))
    assert C.sizeof(C.c_void_p) == 8


# ---- (d) the coverage the GPU test asserts can be met, and M is the median it is said to be
_LOOPS = {}


def _loop(case, algo):
    if (case, algo) not in _LOOPS:
        _LOOPS[(case, algo)] = cases.cpu_loop(case, algo, 32)
    return _LOOPS[(case, algo)]


@pytest.mark.parametrize("case", list(cases.CASES))
def test_m_is_the_median_of_the_cases_own_cpu_episode_counts(case):
    pooled = np.concatenate([cases.counts_of(*_loop(case, a)[1:]) for a in cases.ALGOS])
    assert cases.LOG_M[case] == cases.median_m(pooled) >= 2, (case, cases.median_m(pooled), pooled.min(), pooled.max())


@pytest.mark.parametrize("algo", cases.ALGOS)
@pytest.mark.parametrize("case", list(cases.CASES))
def test_cpu_closed_loop_meets_the_coverage_the_gpu_test_asserts(case, algo):
    R, TE, TR, RC = _loop(case, algo)
    M = cases.LOG_M[case]
    st, lg, c = lref.new_state5(32), lref.new_log(32, M, cases.SENTINEL_RET, cases.SENTINEL_LEN), lref.new_counters()
    for launch in range(cases.LAUNCHES):
        sl = slice(launch * cases.K, (launch + 1) * cases.K)
        lg, st = lref.run(R[sl], TE[sl], TR[sl], RC[sl], st, lg, c)
    print(case, algo, M, c)
    cases.honest(case, algo, c)
    # a scoped condition is one the case does not meet: were it met, the scoping would be stale
    key = dict(over="over_M", under="under_M", spans="spanning_logged", rows="wave_rows_differ")
    for cond in cases.SCOPED.get((case, algo), {}):
        assert c[key[cond]] == 0, (case, algo, cond, c)
    assert np.array_equal(lg["count"], st["episodes"]) and np.array_equal(lg["count"], cases.counts_of(TE, TR, RC))
    for i in range(32):
        n = min(int(lg["count"][i]), M)
        assert (lg["len"][n:, i] == cases.SENTINEL_LEN).all() and (lg["len"][:n, i] > 0).all()
        if lg["count"][i] <= M:
            assert _i64(lref.left_to_right_sum(lg, i)) == _i64(st["return_sum"][i]) and int(lg["len"][:n, i].sum()) == int(st["length_sum"][i])
