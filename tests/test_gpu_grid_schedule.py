"""The grid learners' per-episode schedules and episode log on the GPU (k_grid_learn_sched_rollout, k_grid_learn_log_rollout;
include/mdpp.h "Grid learner schedules and the episode log"): RLToyVectorEnv.set_grid_learner_schedule / clear_ / grid_learner_schedule /
grid_learner_episodes / set_grid_learner_episodes and rollout_grid_learn(K, summary=, log=).

Every case of tests/grid_schedule_cases.py x {numpy, philox} x {q_learning, sarsa} runs at N = 320, K = 37, two launches, and is
held to (1) the open-loop twin, (2) the restatement tests/grid_schedule_ref.py on the same streams -- every action, every
output, the final tables as int32 bits and the counters -- and (3) the kernel's name with ",SCHED=1".
tests/test_grid_schedule_host.py shows on the CPU that the cases exercise what a pass claims."""
import ctypes as C

import numpy as np
import pytest
import torch

import episode_log_ref as lref
import eval_summary_ref as eref
import graph_replay_util as gru
import grid_learner_cases as gc
import grid_learner_ref as gref
import grid_schedule_cases as gsc
import grid_schedule_ref as gsr
import learner_schedule_ref as sref

pytestmark = pytest.mark.gpu

N, K, M_LOG = gsc.N, gsc.K, gsc.LOG_M
SEED = gc.LEARNER_SEED
SENT_RET, SENT_LEN = -7.5, -7
EINVAL = -1                   # MDPP_EINVAL


def _mk(case, rng, n=N, **over):
    from mdp_playground_amd import RLToyVectorEnv
    c = gc.CASES[case]
    extra = dict(rng="philox", philox_seed=gc.PHILOX_SEED) if rng == "philox" else {}
    return RLToyVectorEnv(num_envs=n, env_id_offset=gc.ENV_ID_OFFSET, **extra, **dict(c["kw"], **over), **c["cfg"])


def _np(x):
    return x.cpu().numpy().copy()


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def _dev(env, q, case):
    return None if q is None else torch.as_tensor(gref.as_grid(q, gc.CASES[case]["cfg"]["grid_shape"]), device=env.device)


def _set(env, case, algo, q0="case", sched="case", rates=None):
    """the case's learner and (sched="case") its schedule"""
    c = gc.CASES[case]
    al, ga, ep = rates or c["rates"]
    q0 = gc.initial_tables(case, env.num_envs) if isinstance(q0, str) else q0
    env.set_grid_learner(algo, alpha=al, gamma=ga, epsilon=ep, seed=SEED, q=_dev(env, q0, case), noop=c["noop"])
    if sched == "case":
        env.set_grid_learner_schedule(**gsc.schedule(case, env.num_envs))


def _streams(env):
    from mdp_playground_amd import _capi as capi
    return [env.seeded_streams[s] for s in (capi.STREAM_ENV, capi.STREAM_SPACE, capi.STREAM_ACTION)]


def _assert_same_outputs(got, want, what):
    for name, g, w in zip(("obs", "reward", "terminated", "truncated", "actions"), got, want):
        g, w = _np(g) if torch.is_tensor(g) else np.asarray(g), _np(w) if torch.is_tensor(w) else np.asarray(w)
        if name == "reward":
            g, w = _bits(g.astype(np.float32)), _bits(w.astype(np.float32))
        assert g.shape == w.shape and np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5])


def _assert_same_handles(a, b, rng):
    from mdp_playground_amd import _capi as capi
    sa, sb = a.get_augmented_state(), b.get_augmented_state()
    assert sa.keys() == sb.keys()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    if rng == "numpy":
        for st in (capi.STREAM_ENV, capi.STREAM_SPACE, capi.STREAM_ACTION):
            assert np.array_equal(a.get_rng_streams(st), b.get_rng_streams(st)), st
    assert not a.status().any() and not b.status().any()
    assert gru.tick(a) == gru.tick(b)


def _assert_same_q(a, want, what):
    q = _np(a.get_grid_q()) if not isinstance(a, np.ndarray) else a
    w = _np(want.get_grid_q()) if not isinstance(want, np.ndarray) else want
    assert q.shape == w.shape and np.array_equal(_bits(q), _bits(w)), (what, np.argwhere(_bits(q) != _bits(w))[:5])


def _assert_launch_is_restated(out, traj, sl, what):
    _assert_same_outputs(out, (traj["obs"][sl], traj["reward"][sl], traj["terminated"][sl], traj["truncated"][sl], traj["vectors"][sl]), what)


def _state5(s):
    return {name: _np(t) for (name, _), t in zip(lref.FIELDS5, s.tensors())}


def _new_log(env, m=M_LOG):
    lg = env.episode_log(m)
    lg.ret.fill_(SENT_RET)
    lg.len.fill_(SENT_LEN)
    return lg


def _assert_same5(s, want, what):
    got = _state5(s) if not isinstance(s, dict) else s
    for name, _ in lref.FIELDS5:
        g, w = got[name], want[name]
        assert g.dtype == w.dtype and np.array_equal(g.view(np.uint8), w.view(np.uint8)), (what, name)


def _assert_same_log(lg, want, what):
    for name, t in zip(("count", "ret", "len"), lg.tensors()):
        g, w = _np(t), want[name]
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g.view(np.uint8), w.view(np.uint8)), (what, name)


# ---- the cases: twin, restatement, counters, name
@pytest.mark.parametrize("case", sorted(gsc.CASES))
def test_scheduled_learners_twin_restatement_counters_and_name(case):
    """every case x {numpy, philox} x {q_learning, sarsa} (one test per case: the suite's count of GPU tests stays small)"""
    for rng in ("numpy", "philox"):
        for algo in gref.ALGOS:
            _scheduled_learner_twin_restatement_counters_and_name(case, rng, algo)


def _scheduled_learner_twin_restatement_counters_and_name(case, rng, algo):
    a, b = _mk(case, rng), _mk(case, rng)
    _set(a, case, algo)
    name = a.grid_learn_kernel_name(K)
    assert name == gsc.expected_name(case, rng), name
    assert a.grid_learn_kernel_name(K, summary=True) == gsc.expected_name(case, rng, summary=True)
    assert a.grid_learn_kernel_name(K, eval=True) == gc.expected_name(case, rng, eval=True)          # evaluation names do not change
    assert not _np(a.grid_learner_episodes()).any()
    sch = a.grid_learner_schedule()
    want = gsc.schedule(case)
    assert all((sch[k] is None) == (want[k] is None) and (want[k] is None or np.array_equal(sch[k], np.atleast_2d(want[k]) if k != "row" else want[k]))
               for k in want)
    info, Q, ep, traj = gsc.cpu_run(case, algo, _streams(a) if rng == "numpy" else None)
    assert np.array_equal(_np(a._obs), traj["obs0"])
    for launch in range(gsc.LAUNCHES):
        what = (case, rng, algo, launch)
        out = a.rollout_grid_learn(K)
        _assert_launch_is_restated(out, traj, slice(launch * K, (launch + 1) * K), what)
        _assert_same_outputs(out[:4], b.rollout(out[4]), what)
    _assert_same_handles(a, b, rng)
    _assert_same_q(a, gref.as_grid(Q, gc.CASES[case]["cfg"]["grid_shape"]), (case, rng, algo))
    got_ep = _np(a.grid_learner_episodes())
    assert got_ep.dtype == np.int32 and np.array_equal(got_ep, ep), (case, rng, algo)
    a.close(); b.close()


def test_one_entry_schedule_equals_an_unscheduled_handle_with_those_values():
    case = "g17_noise"
    s = gsc.schedule(case)
    for rng in ("numpy", "philox"):
        a, b = _mk(case, rng), _mk(case, rng)
        _set(a, case, "sarsa")
        _set(b, case, "sarsa", sched=None, rates=(float(s["alpha"][0, 0]), gc.CASES[case]["rates"][1], float(s["epsilon"][0, 0])))
        assert "SCHED=1" in a.grid_learn_kernel_name(K) and "SCHED" not in b.grid_learn_kernel_name(K)
        for launch in range(2):
            _assert_same_outputs(a.rollout_grid_learn(K), b.rollout_grid_learn(K), (rng, launch))
        _assert_same_q(a, b, rng)
        _assert_same_handles(a, b, rng)
        a.close(); b.close()


# ---- the summary form and the log form against the full-output run
@pytest.mark.parametrize("case,rng", [("g55_noop_next_every3", "numpy"), ("g17_noise", "philox"), ("g55_sparse_limit_i32", "philox"),
                                      ("g88_disabled_pnoise", "numpy"), ("g34_noise_next_i32", "numpy")])
def test_summary_and_log_forms_against_the_full_output_run(case, rng):
    """with the case's schedule, and the log without a schedule"""
    for sched in ("case", None):
        _summary_and_log_forms_against_the_full_output_run(case, rng, sched)


def _summary_and_log_forms_against_the_full_output_run(case, rng, sched):
    autoreset = gc.CASES[case]["kw"]["autoreset"]
    a, b, f = _mk(case, rng), _mk(case, rng), _mk(case, rng)         # log form, summary form, full output
    for env in (a, b, f):
        _set(env, case, "sarsa", sched=sched)
    assert a.grid_learn_kernel_name(K, summary=True) == gsc.expected_name(case, rng, summary=True, sched=sched is not None)
    sa, sb, lg = a.episode_summary(), b.episode_summary(), _new_log(a)
    want5, pending = lref.new_state5(N), None
    want_log = lref.new_log(N, M_LOG, SENT_RET, SENT_LEN)
    counters = lref.new_counters()
    for launch in range(3):
        assert a.rollout_grid_learn(K, summary=sa, log=lg) is sa
        b.rollout_grid_learn(K, summary=sb)
        obs, rew, term, trunc, act = f.rollout_grid_learn(K)
        rc, pending = eref.reset_calls(_np(term), _np(trunc), autoreset, pending)
        want_log, want5 = lref.run(_np(rew), _np(term), _np(trunc), rc, want5, want_log, counters)
        _assert_same5(sa, want5, (case, rng, launch, "log form"))
        _assert_same5(sb, want5, (case, rng, launch, "summary form"))
        _assert_same_log(lg, want_log, (case, rng, launch))
        if launch == 0:                        # pop(): the three sums are zeroed, the log is not disturbed
            sa.pop(); sb.pop()
            want5 = lref.pop5(want5)
    assert counters["ended_terminated"] + counters["ended_truncated"] > 0 and counters["over_M"] + counters["under_M"] > 0
    assert (want_log["ret"] == SENT_RET).any() == (counters["under_M"] > 0)      # unwritten entries kept the sentinel
    for env in (a, b):
        _assert_same_q(env, f, (case, rng))
        _assert_same_handles(env, f, rng)
        if sched is not None:
            assert np.array_equal(_np(env.grid_learner_episodes()), _np(f.grid_learner_episodes()))
    with pytest.raises(ValueError):
        a.rollout_grid_learn(K, log=lg)                               # log goes with summary
    with pytest.raises(ValueError):
        a.rollout_grid_learn(K, out=a.alloc_rollout_grid(K), summary=sa, log=lg)
    with pytest.raises(TypeError):
        a.rollout_grid_eval(K, summary=sa, log=lg)                    # no log for the evaluation launches
    a.close(); b.close(); f.close()


# ---- small and ragged sizes, launches of one step (scheduled, log form)
def test_small_and_ragged_sizes_and_launches_of_one_step():
    for n in (1, 63, 257):
        _small_and_ragged_size(n)


def _small_and_ragged_size(n):
    case, algo = "g34_noise_next_i32", "sarsa"
    c = gc.CASES[case]
    for rng in ("numpy", "philox"):
        a = _mk(case, rng, n=n)
        _set(a, case, algo, q0=None)
        s, lg = a.episode_summary(), _new_log(a)
        state, Q, ep, t0 = None, None, None, 0
        want5, want_log = lref.new_state5(n), lref.new_log(n, M_LOG, SENT_RET, SENT_LEN)
        for k in (1, 7, 1, 7, 7):
            info, Q, ep, traj = gsr.closed_loop(c["cfg"], c["kw"], algo, *c["rates"], n, Q, gsc.ref_schedule(case, n), seed=SEED, K=k, launches=1,
                                                noop=c["noop"], philox_seed=gc.PHILOX_SEED, off=gc.ENV_ID_OFFSET,
                                                streams=_streams(a) if rng == "numpy" else None, tick0=t0, state=state, ep=ep)
            state, t0 = traj["state_out"], t0 + k
            want_log, want5 = lref.run(traj["reward"], traj["terminated"], traj["truncated"], traj["reset_call"], want5, want_log)
            a.rollout_grid_learn(k, summary=s, log=lg)
            _assert_same5(s, want5, (n, rng, k))
            _assert_same_log(lg, want_log, (n, rng, k))
            assert np.array_equal(_np(a.grid_learner_episodes()), ep), (n, rng, k)
        assert want_log["count"].any()
        _assert_same_q(a, gref.as_grid(Q, c["cfg"]["grid_shape"]), (n, rng))
        assert not a.status().any()
        a.close()


# ---- the counters through set_grid_learner_episodes
def test_counters_set_to_the_clamps_edge_and_far_past_it():
    for start in ("M-2", 1000):
        _counters_set_to(start)


def _counters_set_to(start):
    case, algo, rng = "g55_sparse_limit_i32", "sarsa", "philox"
    c = gc.CASES[case]
    M = gsc.shape(case)[1]
    ep0 = np.full(N, M - 2 if start == "M-2" else 1000, np.int64)
    a = _mk(case, rng)
    _set(a, case, algo)
    a.set_grid_learner_episodes(torch.as_tensor(ep0))
    assert np.array_equal(_np(a.grid_learner_episodes()), ep0)
    info, Q, ep, traj = gsr.closed_loop(c["cfg"], c["kw"], algo, *c["rates"], N, gc.initial_tables(case), gsc.ref_schedule(case), seed=SEED, K=K,
                                        launches=2, noop=c["noop"], philox_seed=gc.PHILOX_SEED, off=gc.ENV_ID_OFFSET, ep=ep0)
    if start == "M-2":
        assert info["E_changes"] > 0 and info["sel_before_env"].any() and info["sel_last_env"].any()
    else:
        assert info["E_changes"] == 0 and not info["sel_before_env"].any()
    for launch in range(2):
        _assert_launch_is_restated(a.rollout_grid_learn(K), traj, slice(launch * K, (launch + 1) * K), (start, launch))
    _assert_same_q(a, gref.as_grid(Q, c["cfg"]["grid_shape"]), start)
    assert np.array_equal(_np(a.grid_learner_episodes()), ep) and (ep > ep0).any()
    a.set_grid_learner_episodes()                 # None: zeros
    assert not _np(a.grid_learner_episodes()).any()
    for bad in (np.zeros(N - 1, np.int64), np.full(N, -1), np.zeros(N, np.float32)):
        with pytest.raises(ValueError):
            a.set_grid_learner_episodes(bad)
    a.close()


def test_cleared_schedule_equals_a_handle_that_never_had_one():
    case, algo = "g55_sparse_limit_i32", "sarsa"
    for rng in ("numpy", "philox"):
        a, b = _mk(case, rng), _mk(case, rng)
        _set(a, case, algo)
        _set(b, case, algo, sched=None)
        a.clear_grid_learner_schedule()
        assert a.grid_learner_schedule() is None and b.grid_learner_schedule() is None
        assert a.grid_learn_kernel_name(K) == gc.expected_name(case, rng) == b.grid_learn_kernel_name(K)
        for launch in range(2):
            _assert_same_outputs(a.rollout_grid_learn(K), b.rollout_grid_learn(K), (rng, launch))
        _assert_same_q(a, b, rng)
        _assert_same_handles(a, b, rng)
        # set_grid_learner drops a schedule too
        a.set_grid_learner_schedule(**gsc.schedule(case))
        _set(a, case, algo, sched=None)
        assert a.grid_learner_schedule() is None and "SCHED" not in a.grid_learn_kernel_name(K)
        a.close(); b.close()


def test_tables_replaced_between_launches_without_touching_q():
    case, algo, rng = "g34_noise_next_i32", "sarsa", "philox"
    c = gc.CASES[case]
    a = _mk(case, rng)
    _set(a, case, algo)
    first = gsc.ref_schedule(case)
    # the second schedule: epsilon only, other values, another M, the rows the other way round
    eps2 = np.array([[0.2, 0.1], [0.9, 0.6], [0.5, 0.3]], np.float32)
    row2 = ((np.arange(N) + 1) % 3).astype(np.int32)
    info, Q, ep, traj = gsr.closed_loop(c["cfg"], c["kw"], algo, *c["rates"], N, gc.initial_tables(case), first, seed=SEED, K=K, launches=1,
                                        noop=c["noop"], philox_seed=gc.PHILOX_SEED, off=gc.ENV_ID_OFFSET)
    _assert_launch_is_restated(a.rollout_grid_learn(K), traj, slice(0, K), "first")
    assert ep.any()
    q_before = _np(a.get_grid_q())
    a.set_grid_learner_schedule(epsilon=eps2, row=row2)
    _assert_same_q(_np(a.get_grid_q()), q_before, "the tables stay")
    assert not _np(a.grid_learner_episodes()).any()               # a new schedule starts at zero
    info2, Q2, ep2, traj2 = gsr.closed_loop(c["cfg"], c["kw"], algo, *c["rates"], N, Q, sref.Schedule(N, epsilon=eps2, row=row2), seed=SEED, K=K,
                                            launches=1, noop=c["noop"], philox_seed=gc.PHILOX_SEED, off=gc.ENV_ID_OFFSET, tick0=K,
                                            state=traj["state_out"])
    assert info2["E_changes"] > 0 and info2["alpha_changes"] == 0
    _assert_launch_is_restated(a.rollout_grid_learn(K), traj2, slice(0, K), "second")
    _assert_same_q(a, gref.as_grid(Q2, c["cfg"]["grid_shape"]), "second")
    assert np.array_equal(_np(a.grid_learner_episodes()), ep2)
    a.close()


def test_tables_in_lds_equal_tables_in_global_memory_under_a_schedule():
    for case in ("g55_sparse_limit_i32", "g17_noise"):
        _tables_in_lds_equal_tables_in_global_memory(case)


def _tables_in_lds_equal_tables_in_global_memory(case):
    for rng in ("numpy", "philox"):
        a, b = _mk(case, rng), _mk(case, rng)
        b.set_kernel_options("NO_GRID_QLDS")
        for env in (a, b):
            _set(env, case, "sarsa")
        assert a.grid_learn_kernel_name(K) == gsc.expected_name(case, rng, qlds=1)
        assert b.grid_learn_kernel_name(K) == gsc.expected_name(case, rng, qlds=0)
        sa, sb, la, lb = a.episode_summary(), b.episode_summary(), _new_log(a), _new_log(b)
        _assert_same_outputs(a.rollout_grid_learn(K), b.rollout_grid_learn(K), (case, rng, "full"))
        a.rollout_grid_learn(K, summary=sa); b.rollout_grid_learn(K, summary=sb)
        a.rollout_grid_learn(K, summary=sa, log=la); b.rollout_grid_learn(K, summary=sb, log=lb)
        _assert_same5(sa, _state5(sb), (case, rng))
        _assert_same_log(la, {k: _np(t) for k, t in zip(("count", "ret", "len"), lb.tensors())}, (case, rng))
        _assert_same_q(a, b, (case, rng))
        assert np.array_equal(_np(a.grid_learner_episodes()), _np(b.grid_learner_episodes()))
        _assert_same_handles(a, b, rng)
        a.close(); b.close()


def test_evaluation_between_two_scheduled_launches_moves_no_counter():
    case, algo, rng = "g55_sparse_limit_i32", "q_learning", "numpy"
    a, b = _mk(case, rng), _mk(case, rng)
    for env in (a, b):
        _set(env, case, algo)
    _assert_same_outputs(a.rollout_grid_learn(K), b.rollout_grid_learn(K), "first")
    ep = _np(a.grid_learner_episodes())
    assert ep.any()
    q = _np(a.get_grid_q())
    out = a.rollout_grid_eval(K)
    s = a.episode_summary()
    a.rollout_grid_eval(K, summary=s)
    assert _np(s.episodes).any()                                    # episodes ended under evaluation ...
    assert np.array_equal(_np(a.grid_learner_episodes()), ep)       # ... and no counter moved
    _assert_same_q(_np(a.get_grid_q()), q, "evaluation left the tables alone")
    # b steps the evaluation's actions open-loop: the following scheduled launches are equal
    b.rollout(out[4])
    sb = b.episode_summary()
    b.rollout_grid_eval(K, summary=sb)
    _assert_same_outputs(a.rollout_grid_learn(K), b.rollout_grid_learn(K), "second")
    assert np.array_equal(_np(a.grid_learner_episodes()), _np(b.grid_learner_episodes()))
    _assert_same_q(a, b, "after evaluation")
    a.close(); b.close()


# ---- HIP graphs
def test_scheduled_log_launch_replayed_from_a_hip_graph():
    case, algo, rng = "g34_noise_next_i32", "sarsa", "philox"
    a, b = _mk(case, rng), _mk(case, rng)
    for env in (a, b):
        _set(env, case, algo)
    sa, sb, la, lb = a.episode_summary(), b.episode_summary(), _new_log(a, 9), _new_log(b, 9)
    a.rollout_grid_learn(K, summary=sa, log=la)  # the eager launch of the same form before the capture
    b.rollout_grid_learn(K, summary=sb, log=lb)
    call = gru.capture(a, lambda: a.rollout_grid_learn(K, summary=sa, log=la), K)
    counts, eps = [_np(la.count)], [_np(a.grid_learner_episodes())]
    for replay in range(3):
        acts = torch.as_tensor(gref.action_vector(np.random.default_rng(replay).integers(0, 4, size=((3, 2, 2)[replay], N))), device=a.device)
        _assert_same_outputs(a.rollout(acts), b.rollout(acts), ("between", replay))
        call.replay()
        b.rollout_grid_learn(K, summary=sb, log=lb)
        torch.cuda.synchronize()
        _assert_same5(sa, _state5(sb), ("replay", replay))
        _assert_same_log(la, {k: _np(t) for k, t in zip(("count", "ret", "len"), lb.tensors())}, ("replay", replay))
        counts.append(_np(la.count)); eps.append(_np(a.grid_learner_episodes()))
        assert np.array_equal(eps[-1], _np(b.grid_learner_episodes()))
        assert (counts[-1] >= counts[-2]).all() and (counts[-1] > counts[-2]).any()      # the log goes on from replay to replay
        assert (eps[-1] > eps[-2]).any() and np.array_equal(eps[-1] - eps[0], counts[-1] - counts[0])
    _assert_same_q(a, b, "graph")
    _assert_same_handles(a, b, rng)
    a.close(); b.close()


# ---- refusals: each leaves Q, counters and schedule unchanged
_DISCRETE = dict(state_space_type="discrete", action_space_type="discrete", state_space_size=8, action_space_size=8, delay=0,
                 sequence_length=1, seed=0)


def test_refusals_change_nothing():
    from mdp_playground_amd import RLToyVectorEnv, _capi as capi
    case, algo, rng = "g34_dense", "q_learning", "philox"
    a, b = _mk(case, rng), _mk(case, rng)
    sched = gsc.schedule(case)
    s, lg = a.episode_summary(), _new_log(a)
    # no learner
    for call in (lambda: a.set_grid_learner_schedule(**sched), a.clear_grid_learner_schedule, a.grid_learner_episodes, a.set_grid_learner_episodes,
                 lambda: a.rollout_grid_learn(4, summary=s, log=lg)):
        with pytest.raises(capi.MdppError, match="no learner"):
            call()
    for env in (a, b):
        _set(env, case, algo, sched=None)
    # no schedule
    for call in (a.grid_learner_episodes, a.set_grid_learner_episodes):
        with pytest.raises(capi.MdppError, match="no schedule"):
            call()
    assert a.grid_learner_schedule() is None
    for env in (a, b):
        env.set_grid_learner_schedule(**sched)
        env.rollout_grid_learn(K)
    # a scheduled parameter through set_grid_learner_rates (epsilon is scheduled here; alpha and gamma are not)
    with pytest.raises(capi.MdppError, match="mdpp_clear_grid_learner_schedule"):
        a.set_grid_learner_rates(epsilon=0.5)
    with pytest.raises(capi.MdppError, match="mdpp_clear_grid_learner_schedule"):
        a.set_grid_learner_rates(gamma=0.5, epsilon=0.5)              # (nothing of the call is applied: not the gamma either)
    # ... shown before anything overwrites it: a launch of the refused handle equals one of the handle that made no such call
    _assert_same_outputs(a.rollout_grid_learn(K), b.rollout_grid_learn(K), "after the refused rates")
    _assert_same_q(a, b, "after the refused rates")
    for env in (a, b):
        env.set_grid_learner_rates(alpha=0.25, gamma=0.8)             # accepted
    # bad tables and rows: the binding's checks, then the library's own
    for bad in (dict(), dict(epsilon=[0.5, 1.5]), dict(epsilon=[0.5, float("nan")]), dict(alpha=[0.0, 0.5]), dict(epsilon=[[0.5], [0.25]]),
                dict(epsilon=[[0.5], [0.25]], row=np.full(N, 2)), dict(epsilon=[[0.5], [0.25]], row=np.zeros(N - 1, np.int64)),
                dict(epsilon=[0.5, 0.25], alpha=[0.5]), dict(epsilon=np.zeros((0,), np.float32))):
        with pytest.raises(ValueError):
            a.set_grid_learner_schedule(**bad)
    lib, stream = a._lib, a._stream()
    good, row = np.array([0.5, 0.25], np.float32), np.zeros(N, np.int32)
    bad_row = row.copy(); bad_row[N - 1] = 2
    for args in ((None, None, 1, 2, None), (np.array([0.5, 1.5], np.float32), None, 1, 2, None), (None, np.array([0.0, 0.5], np.float32), 1, 2, None),
                 (np.array([0.5, np.nan], np.float32), good, 1, 2, None), (good, None, 2, 1, None), (good, None, 2, 1, bad_row), (good, None, 1, 2, row),
                 (good, None, 0, 2, None), (good, None, 1, 0, None), (good, None, 1 << 12, 1 << 11, row)):
        e, al, R, M, r = args
        assert lib.mdpp_set_grid_learner_schedule(a._h, capi.nptr(e), capi.nptr(al), R, M, capi.nptr(r), stream) == EINVAL, args[2:4]
        assert b"mdpp_set_grid_learner_schedule" in lib.mdpp_last_error(a._h)
    # a null or oversized log
    ptrs = [C.c_void_p(t.data_ptr()) for t in s.tensors() + lg.tensors()]
    for hole in (5, 6, 7):
        p = list(ptrs); p[hole] = None
        assert lib.mdpp_step_n_grid_learn_log(a._h, 4, *p, M_LOG, stream) == EINVAL and b"null log buffer" in lib.mdpp_last_error(a._h)
    for m, why in ((0, b"M < 1"), (-3, b"M < 1"), ((2 ** 31 - 1) // N + 1, b"2^31 - 1")):
        assert lib.mdpp_step_n_grid_learn_log(a._h, 4, *ptrs, m, stream) == EINVAL and why in lib.mdpp_last_error(a._h)
    assert not _np(s.episodes).any() and not _np(lg.count).any() and (_np(lg.ret) == SENT_RET).all()
    # nothing changed: schedule, counters, tables, and the next launch
    assert np.array_equal(a.grid_learner_schedule()["epsilon"], b.grid_learner_schedule()["epsilon"])
    assert np.array_equal(_np(a.grid_learner_episodes()), _np(b.grid_learner_episodes()))
    _assert_same_q(a, b, "before")
    assert a.grid_learn_kernel_name(K) == gsc.expected_name(case, rng)
    _assert_same_outputs(a.rollout_grid_learn(K), b.rollout_grid_learn(K), "after the refusals")
    _assert_same_q(a, b, "after")
    assert np.array_equal(_np(a.grid_learner_episodes()), _np(b.grid_learner_episodes()))
    a.close(); b.close()
    # a handle that is not a grid; the discrete methods keep refusing a grid handle
    d = RLToyVectorEnv(num_envs=64, **_DISCRETE)
    for call in (lambda: d.set_grid_learner_schedule(epsilon=[0.5, 0.25]), d.clear_grid_learner_schedule, d.grid_learner_episodes,
                 d.set_grid_learner_episodes):
        with pytest.raises(NotImplementedError, match="serve grid envs only"):
            call()
    assert d._lib.mdpp_set_grid_learner_schedule(d._h, capi.nptr(good), None, 1, 2, None, d._stream()) == capi.EUNSUPPORTED
    assert b"grid learners serve grid envs only" in d._lib.mdpp_last_error(d._h)
    d.close()
    g = _mk(case, rng)
    _set(g, case, algo)
    for call in (lambda: g.set_learner_schedule(epsilon=[0.5, 0.25]), g.learner_episodes, g.set_learner_episodes):
        with pytest.raises((NotImplementedError, capi.MdppError)):
            call()
    g.close()
