"""Eligibility traces on the GPU beyond the full-output launch (RLToyVectorEnv.set_learner_traces; k_discrete_trace_summary and
its _log kernel, the SCHED forms): the summary= and summary= + log= launches against the full-output twin
and the rules of DESIGN.md 3.13 and 3.24 (tests/eval_summary_ref.py, tests/episode_log_ref.py), a per-episode schedule with
traces against the restatement -- alpha changing at an episode end while Z is non-zero --, and one launch captured in the
library's capture mode and replayed three times on a Philox handle with a delay, Z crossing the replays.  N = 320, K = 37;
every comparison is bit for bit."""
import numpy as np
import pytest
import torch

import episode_log_ref as lref
import eval_summary_ref as sumref
import graph_replay_util as gr
import learner_schedule_cases as scases
import learner_sweep_ref as ref
import learner_trace_cases as cases
import learner_trace_ref as tref
from test_gpu_learn_rollout import _assert_same_handles, _assert_same_outputs, _mk, _np, _tick
from test_gpu_learn_traces import K, N, OFF, Restated, _check_launch, _name, _traced

pytestmark = pytest.mark.gpu

LOG_M = 6
SENTINEL_RET, SENTINEL_LEN = -12345.5, -7


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int64) if x.dtype == np.float64 else x.view(np.int32) if x.dtype == np.float32 else x


def _same_tables(a, b, what):
    assert torch.equal(a.get_q().view(torch.int32), b.get_q().view(torch.int32)), (what, "Q")
    assert torch.equal(a.get_traces().view(torch.int32), b.get_traces().view(torch.int32)), (what, "Z")


@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("handle,algo,kind,rng,form", [
    ("s8_max5", "q_learning", tref.ACCUMULATING, "numpy", "uniform"), ("cfg2", "sarsa", tref.REPLACING, "philox", "pe"),
    ("s8_next_max5", "sarsa", tref.ACCUMULATING, "philox", "uniform"), ("cfg2_disabled_max5", "q_learning", tref.REPLACING, "numpy", "pe"),
    ("s8_noise", "q_learning", tref.REPLACING, "philox", "pe")])
def test_summary_and_log_launches_equal_the_full_output_launch(handle, algo, kind, rng, form, log):
    cfg, kw = cases.HANDLES[handle]
    full, summ = _traced(handle, rng, algo, kind, form), _traced(handle, rng, algo, kind, form)
    assert summ.learn_kernel_name(K) == _name(cfg, rng, form)
    s = summ.episode_summary()
    lg = summ.episode_log(LOG_M) if log else None
    want_log = None
    if log:
        lg.ret.fill_(SENTINEL_RET); lg.len.fill_(SENTINEL_LEN)
        want_log = lref.new_log(N, LOG_M, SENTINEL_RET, SENTINEL_LEN)
    st5, pending = lref.new_state5(N), None
    for launch in range(cases.LAUNCHES):
        what = (handle, algo, kind, rng, form, log, launch)
        out = full.rollout_learn(K)
        assert summ.rollout_learn(K, summary=s, log=lg) is s
        rew, term, trunc = _np(out[1]), _np(out[2]), _np(out[3])
        reset_call, pending = sumref.reset_calls(term, trunc, kw.get("autoreset", ref.SAME_STEP), pending)
        if log:
            want_log, st5 = lref.run(rew, term, trunc, reset_call, st5, want_log)
            for name, t in zip(("count", "ret", "len"), lg.tensors()):
                assert np.array_equal(_bits(_np(t)), _bits(want_log[name])), (what, "log." + name)
        else:
            st5 = sumref.summary(rew, term, trunc, reset_call, st5)
        for (name, _), t in zip(sumref.FIELDS, s.tensors()):
            assert np.array_equal(_bits(_np(t)), _bits(st5[name])), (what, name)
        _same_tables(summ, full, what)
        assert _np(s.episodes).any()
    _assert_same_handles(full, summ, rng)
    if handle not in cases.Z_BOUNDARY_EXEMPT:
        assert _np(summ.get_traces()).any()
    full.close(); summ.close()


@pytest.mark.parametrize("opt", ["NO_LEARN_LDS", "LEARN_SHORT_PIECES"])
def test_summary_launch_in_the_global_memory_form_and_in_pieces(opt):
    handle, algo, kind, rng = "s8_max5", "sarsa", tref.ACCUMULATING, "numpy"
    cfg = cases.HANDLES[handle][0]
    one, other = _traced(handle, rng, algo, kind), _traced(handle, rng, algo, kind, opts=(opt,))
    assert other.learn_kernel_name(K) == _name(cfg, rng, qlds=opt != "NO_LEARN_LDS")
    s1, s2 = one.episode_summary(), other.episode_summary()
    for launch in range(2):
        one.rollout_learn(K, summary=s1); other.rollout_learn(K, summary=s2)
        for g, w in zip(s2.tensors(), s1.tensors()):
            assert torch.equal(g, w), (opt, launch)
        _same_tables(other, one, (opt, launch))
    assert _np(one.get_traces()).any()
    _assert_same_handles(one, other, rng)
    one.close(); other.close()


# ---- a per-episode schedule with traces
@pytest.mark.parametrize("rng", cases.RNGS)
@pytest.mark.parametrize("algo,kind,skind", [("q_learning", tref.ACCUMULATING, "both"), ("sarsa", tref.REPLACING, "alpha"), ("sarsa", tref.ACCUMULATING, "eps")])
def test_schedule_with_traces_against_the_restatement(algo, kind, skind, rng):
    """tests/learner_schedule_cases.py's tables on s8_max5 (M = 24, four rows by i % 4): E and alpha are looked up again at
    every episode end, where Z -- non-zero after the sweep -- is zeroed"""
    handle = "s8_max5"
    cfg, kw = cases.HANDLES[handle]
    m = scases.HANDLES[handle][2]
    a = _traced(handle, rng, algo, kind)
    eps, al = scases.tables(skind, m)
    a.set_learner_schedule(epsilon=eps, alpha=al, row=scases.rows(N))
    assert a.learn_kernel_name(K) == _name(cfg, rng, sched=True), a.learn_kernel_name(K)
    r = Restated(a, algo, kind, sched=scases.schedule(skind, m, N))
    b = _mk(cfg, rng, env_id_offset=OFF, **kw)
    for launch in range(cases.LAUNCHES):
        out = _check_launch(a, r, K, (algo, kind, skind, rng, launch))
        _assert_same_outputs(out[:4], b.rollout(out[4]), (algo, launch))
        assert np.array_equal(_np(a.learner_episodes()), r.agent.ep)
    info = r.agent.info
    assert info["ends"] > 0 and (r.agent.ep > 0).all()
    if skind in ("alpha", "both"):
        assert info["alpha_changes"] > 0 and info["alpha_change_with_z"] > 0, info
    if skind in ("eps", "both"):
        assert info["E_changes"] > 0, info
    # ... and its summary form equals it
    c = _traced(handle, rng, algo, kind)
    c.set_learner_schedule(epsilon=eps, alpha=al, row=scases.rows(N))
    assert c.learn_kernel_name(K) == a.learn_kernel_name(K)
    s = c.episode_summary()
    for launch in range(cases.LAUNCHES):
        c.rollout_learn(K, summary=s)
    _same_tables(c, a, "summary form")
    assert torch.equal(c.learner_episodes(), a.learner_episodes())
    _assert_same_handles(a, c, rng)
    _assert_same_handles(a, b, rng)
    a.close(); b.close(); c.close()


# ---- graph replay: Z is read from the handle's buffer at replay and crosses the replays
@pytest.mark.parametrize("summary", [False, True])
def test_captured_trace_launch_replayed_three_times(summary):
    handle, algo, kind, rng = "cfg2", "sarsa", tref.ACCUMULATING, "philox"          # Philox streams and delay = 4
    a, b = _traced(handle, rng, algo, kind, "pe"), _traced(handle, rng, algo, kind, "pe")
    sa, sb = (a.episode_summary(), b.episode_summary()) if summary else (None, None)
    out_a = None if summary else a._alloc_rollout_closed(K)

    def call(e, s, out=None):
        return e.rollout_learn(K, summary=s) if summary else e.rollout_learn(K, out)

    call(a, sa, out_a); call(b, sb)                         # the eager launch before the capture (fills, LDS attribute)
    g = gr.capture(a, lambda: call(a, sa, out_a), K)
    for replay in range(3):
        z0 = a.get_traces()
        assert _np(z0).any(), replay                        # Z is non-zero going into the replay
        g.replay()
        out_b = call(b, sb)
        if summary:
            for x, y in zip(sa.tensors(), sb.tensors()):
                assert torch.equal(x, y), replay
        else:
            for name, x, y in zip(("obs", "reward", "terminated", "truncated", "actions"), out_a, out_b):
                assert torch.equal(x.view(torch.uint8) if x.dtype == torch.bool else x, y.view(torch.uint8) if y.dtype == torch.bool else y), (replay, name)
        _same_tables(a, b, replay)
        assert not torch.equal(a.get_traces(), z0), replay
    assert _tick(a) == _tick(b) == 4 * K
    _assert_same_handles(a, b, rng)
    a.close(); b.close()
