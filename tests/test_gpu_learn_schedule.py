"""Per-episode epsilon / alpha schedules of the in-kernel learners on the GPU (RLToyVectorEnv.set_learner_schedule; the SCHED
forms of k_discrete_learn_rollout / k_discrete_learn_summary; include/mdpp.h "Schedules").

As in tests/test_gpu_learn_sweep.py every launch is held to two yardsticks: the open-loop twin (an identically built handle
fed with the actions the launch returned: outputs, state record, env and space streams, tick) and the numpy restatement
tests/learner_schedule_ref.py fed with the launch's own outputs -- actions, get_q() and learner_episodes(), bit for bit.
N = 320 envs (one full workgroup and a partial one), K = 37 steps (no multiple of 4), two launches in a row,
env_id_offset = 1000.  What the passes must have exercised is stated in tests/learner_schedule_cases.py and shown reachable
on the CPU by tests/test_learner_schedule_host.py.  There is no tolerance anywhere: every comparison is bit for bit."""
import numpy as np
import pytest
import torch

import eval_summary_ref as sumref
import graph_replay_util as gr
import learner_schedule_cases as cases
import learner_schedule_ref as sref
import learner_sweep_cases as sweep
import learner_sweep_ref as ref
from test_gpu_learn_rollout import _CONT, _assert_same_handles, _assert_same_outputs, _bits, _mk, _np, _obs_now, _tick

pytestmark = pytest.mark.gpu

N, K = 320, cases.K
OFF = 1000
SEED, ALPHA, GAMMA, EPS = cases.SEED, cases.ALPHA, cases.GAMMA, cases.EPS


def _scheduled(handle, rng, algo, kind, n=N, off=OFF, lo=0, opts=(), **learner):
    """a handle of the case with its learner and its schedule set; env i follows row (lo + i) % 4"""
    cfg, kw, m = cases.HANDLES[handle]
    e = _mk(cfg, rng, n=n, env_id_offset=off, **kw)
    if opts:
        e.set_kernel_options(*opts)
    e.set_learner(algo, **dict(dict(alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=SEED), **learner))
    eps, al = cases.tables(kind, m)
    e.set_learner_schedule(epsilon=eps, alpha=al, row=cases.rows(n, lo))
    return e


class Restated:
    """the restatement, carried from launch to launch beside a handle"""

    def __init__(self, env, handle, algo, kind, off=OFF, lo=0, alpha=ALPHA, eps=EPS, sched="case"):
        cfg, kw, m = cases.HANDLES[handle]
        mdp = env.mdps[0]
        n = env.num_envs
        self.P, self.off = np.asarray(mdp.P), off
        shape = (n, 2, mdp.S, mdp.A) if algo == "double_q" else (n, mdp.S, mdp.A)
        self.sched = cases.schedule(kind, m, n, lo) if sched == "case" else sched
        self.agent = sref.Agent(algo, n, alpha, GAMMA, eps, self.sched, np.zeros(shape, np.float32), kw.get("autoreset", ref.SAME_STEP))

    def launch(self, tick0, obs_before, out):
        obs, rew, term, trunc = (_np(x) for x in out[:4])
        k, n = obs.shape
        w = [ref.tick_words(SEED, self.off, tick0, k + 1, n, st) for st in (ref.EXPLORE_STREAM, ref.ACTION_STREAM, ref.UPDATE_STREAM)]
        return sref.run(self.agent, obs_before, obs, rew, term, trunc, self.P, *w)


def _check_launch(a, r, k, what):
    """one learning launch of handle a against the restatement r (actions, tables, counters); returns its outputs"""
    before, tick0 = _obs_now(a), _tick(a)
    out = a.rollout_learn(k)
    assert out[4].dtype == torch.int32 and tuple(out[4].shape) == (k, a.num_envs)
    want = r.launch(tick0, before, out)
    got = _np(out[4])
    assert np.array_equal(got, want), (what, "actions", np.argwhere(got != want)[:5])
    q = _np(a.get_q())
    assert q.dtype == np.float32 and q.shape == r.agent.Q.shape
    assert np.array_equal(_bits(q), _bits(r.agent.Q)), (what, "Q", np.argwhere(_bits(q) != _bits(r.agent.Q))[:5])
    ep = a.learner_episodes()
    assert ep.dtype == torch.int32 and tuple(ep.shape) == (a.num_envs,) and ep.device == a.device
    assert np.array_equal(_np(ep), r.agent.ep), (what, "episodes", np.argwhere(_np(ep) != r.agent.ep)[:5])
    return out


def _name(handle, rng, algo, summary=False, qlds=None, sched=True):
    cfg = cases.HANDLES[handle][0]
    qlds = handle not in cases.GLOBAL_FORM if qlds is None else qlds
    return "%s<PHILOX=%d,NOISE=%d,UNIT=%d,QLDS=%d,PE=1%s%s>" % (
        "k_discrete_learn_summary" if summary else "k_discrete_learn_rollout", rng == "philox", "transition_noise" in cfg,
        "reward_dist" not in cfg, qlds, ",DOUBLE=1" if algo == "double_q" else "", ",SCHED=1" if sched else "")


def _equal_launches(a, b, launches, what, k=K):
    for launch in range(launches):
        for name, g, w in zip(("obs", "reward", "terminated", "truncated", "actions"), a.rollout_learn(k), b.rollout_learn(k)):
            assert torch.equal(g, w), (what, launch, name)
    assert torch.equal(a.get_q().view(torch.int32), b.get_q().view(torch.int32)), what


# ---- twin and restatement
@pytest.mark.parametrize("rng", cases.RNGS)
@pytest.mark.parametrize("algo", cases.ALGOS)
@pytest.mark.parametrize("handle", list(cases.HANDLES))
def test_scheduled_launch_twin_and_restatement(handle, algo, rng):
    cfg, kw, m = cases.HANDLES[handle]
    kind = cases.kind_of(handle, algo, rng)
    a, b = _scheduled(handle, rng, algo, kind), _mk(cfg, rng, env_id_offset=OFF, **kw)
    assert a.learn_kernel_name(K) == _name(handle, rng, algo), a.learn_kernel_name(K)
    got = a.learner_schedule()
    eps, al = cases.tables(kind, m)
    for key, t in (("epsilon", eps), ("alpha", al)):
        assert (got[key] is None) == (t is None) and (t is None or np.array_equal(got[key], t.astype(np.float32)))
    assert np.array_equal(got["row"], cases.rows(N)) and not _np(a.learner_episodes()).any()
    r = Restated(a, handle, algo, kind)
    for launch in range(cases.LAUNCHES):
        assert _tick(a) == launch * K
        out = _check_launch(a, r, K, (handle, algo, rng, launch))
        _assert_same_outputs(out[:4], b.rollout(out[4]), (handle, algo, rng, launch))
    _assert_same_handles(a, b, rng)
    info = r.agent.info
    print(handle, algo, rng, kind, "ep", r.agent.ep.min(), r.agent.ep.max(), {k: v for k, v in info.items() if not isinstance(v, np.ndarray)})
    cases.honest(handle, algo, kind, m, info, r.agent.ep, r.sched.row)
    a.close(); b.close()


# ---- equivalences
@pytest.mark.parametrize("algo", cases.ALGOS)
def test_tables_constant_at_the_handles_rates_give_the_unscheduled_pe_handle(algo):
    cfg, kw, m = cases.HANDLES["cfg2"]
    pe, sc = _mk(cfg, "numpy", env_id_offset=OFF), _mk(cfg, "numpy", env_id_offset=OFF)
    pe.set_learner(algo, alpha=np.full(N, ALPHA), gamma=GAMMA, epsilon=np.full(N, EPS), seed=SEED)
    sc.set_learner(algo, alpha=0.7, gamma=GAMMA, epsilon=0.9, seed=SEED)            # (both overridden by the tables)
    sc.set_learner_schedule(epsilon=np.full(3, EPS), alpha=np.full(3, ALPHA))
    assert pe.learn_kernel_name(K) == _name("cfg2", "numpy", algo, sched=False) and sc.learn_kernel_name(K) == _name("cfg2", "numpy", algo)
    assert sc.learner_schedule()["row"] is None
    _equal_launches(sc, pe, 2, algo)
    assert _np(sc.learner_episodes()).max() > 3                                       # (the counter ran past the table all the same)
    # one table only: the other parameter is the handle's own
    one = _mk(cfg, "numpy", env_id_offset=OFF)
    one.set_learner(algo, alpha=ALPHA, gamma=GAMMA, epsilon=0.9, seed=SEED)
    one.set_learner_schedule(epsilon=np.full((1, 2), EPS))
    pe2 = _mk(cfg, "numpy", env_id_offset=OFF)
    pe2.set_learner(algo, alpha=np.full(N, ALPHA), gamma=GAMMA, epsilon=np.full(N, EPS), seed=SEED)
    _equal_launches(one, pe2, 2, (algo, "epsilon only"))
    for e in (pe, sc, one, pe2):
        assert not e.status().any()
        e.close()


@pytest.mark.parametrize("rng", cases.RNGS)
@pytest.mark.parametrize("handle,algo", [("cfg2", "sarsa"), ("cfg2_next_step", "double_q"), ("cfg2_disabled_max5", "q_learning"), ("s20", "sarsa")])
def test_summary_launch_equals_the_full_output_launch(handle, algo, rng):
    kw = cases.HANDLES[handle][1]
    full, summ = _scheduled(handle, rng, algo, "both"), _scheduled(handle, rng, algo, "both")
    assert summ.learn_kernel_name(K) == _name(handle, rng, algo)
    s = summ.episode_summary()
    st5, pending = sumref.new_state5(N), None
    for launch in range(cases.LAUNCHES):
        ep0, epi0 = _np(summ.learner_episodes()), _np(s.episodes)
        out = full.rollout_learn(K)
        assert summ.rollout_learn(K, summary=s) is s
        reset_call, pending = sumref.reset_calls(_np(out[2]), _np(out[3]), kw.get("autoreset", ref.SAME_STEP), pending)
        st5 = sumref.summary(_np(out[1]), _np(out[2]), _np(out[3]), reset_call, st5)
        for (name, _), t in zip(sumref.FIELDS, s.tensors()):
            g, w = _np(t), st5[name]
            assert np.array_equal(g.view(np.int64) if g.dtype == np.float64 else g, w.view(np.int64) if w.dtype == np.float64 else w), (handle, launch, name)
        assert torch.equal(summ.get_q().view(torch.int32), full.get_q().view(torch.int32)), (handle, launch)
        assert torch.equal(summ.learner_episodes(), full.learner_episodes()), (handle, launch)
        # the counter moves as the summary's episodes do
        assert np.array_equal(_np(summ.learner_episodes()) - ep0, _np(s.episodes) - epi0) and (_np(s.episodes) - epi0).any()
    _assert_same_handles(full, summ, rng)
    full.close(); summ.close()


@pytest.mark.parametrize("opt", ["LEARN_SHORT_PIECES", "NO_LEARN_LDS"])
@pytest.mark.parametrize("algo", cases.ALGOS)
def test_pieces_and_the_global_memory_form_equal_one_lds_launch(algo, opt):
    one, other = _scheduled("cfg2_disabled_max5", "numpy", algo, "both"), _scheduled("cfg2_disabled_max5", "numpy", algo, "both", opts=(opt,))
    assert other.learn_kernel_name(K) == _name("cfg2_disabled_max5", "numpy", algo, qlds=opt != "NO_LEARN_LDS")
    _equal_launches(other, one, 2, (algo, opt))
    assert torch.equal(one.learner_episodes(), other.learner_episodes())
    _assert_same_handles(one, other, "numpy")
    # ... and keeping summaries in pieces
    s1, s2 = one.episode_summary(), other.episode_summary()
    one.rollout_learn(K, summary=s1); other.rollout_learn(K, summary=s2)
    for g, w in zip(s2.tensors(), s1.tensors()):
        assert torch.equal(g, w)
    assert torch.equal(one.learner_episodes(), other.learner_episodes())
    assert torch.equal(one.get_q().view(torch.int32), other.get_q().view(torch.int32))
    one.close(); other.close()


@pytest.mark.parametrize("algo", ["sarsa", "double_q"])
def test_counters_beyond_the_table_hold_the_last_entries_and_zeroed_counters_restart(algo):
    handle = "s8_max5"
    cfg, kw, m = cases.HANDLES[handle]
    a = _scheduled(handle, "philox", algo, "both")
    a.set_learner_episodes(np.full(N, m + 3))
    assert (_np(a.learner_episodes()) == m + 3).all()
    eps, al = cases.tables("both", m)
    row = cases.rows(N)
    last = _mk(cfg, "philox", env_id_offset=OFF, **kw)
    last.set_learner(algo, alpha=al[row, -1], gamma=GAMMA, epsilon=eps[row, -1], seed=SEED)
    _equal_launches(a, last, 2, (algo, "held at the last entries"))
    assert (_np(a.learner_episodes()) > m + 3).all()
    # a torch tensor on the device, then zeros: the restatement follows from ep = 0 with the tables the handle has by now
    a.set_learner_episodes(torch.full((N,), 2, dtype=torch.int64, device=a.device))
    assert (_np(a.learner_episodes()) == 2).all()
    a.set_learner_episodes()
    assert not _np(a.learner_episodes()).any()
    r = Restated(a, handle, algo, "both")
    r.agent.Q = _np(a.get_q())
    _check_launch(a, r, K, (algo, "restarted"))
    assert r.agent.info["E_changes"] > 0 and (r.agent.ep < m - 1).any()
    for bad in (np.full(N - 1, 1), np.full(N, -1), np.full(N, 0.5), np.full((N, 1), 1)):
        with pytest.raises(ValueError):
            a.set_learner_episodes(bad)
    a.close(); last.close()


@pytest.mark.parametrize("algo", ["q_learning", "double_q"])
def test_evaluation_reads_no_table_and_moves_no_counter(algo):
    handle = "cfg2"
    cfg, kw, m = cases.HANDLES[handle]
    a, b = _scheduled(handle, "numpy", algo, "both"), _mk(cfg, "numpy", env_id_offset=OFF, **kw)
    out = a.rollout_learn(K)
    b.rollout(out[4])
    b.set_learner(algo, alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=SEED, q=a.get_q())      # an unscheduled handle with the same tables
    ep, q, sched = a.learner_episodes(), a.get_q(), a.learner_schedule()
    assert _np(ep).any()
    for name, g, w in zip(("obs", "reward", "terminated", "truncated", "actions"), a.rollout_eval(K), b.rollout_eval(K)):
        assert torch.equal(g, w), (algo, name)
    sa, sb = a.episode_summary(), b.episode_summary()
    a.rollout_eval(K, summary=sa); b.rollout_eval(K, summary=sb)
    for g, w in zip(sa.tensors(), sb.tensors()):
        assert torch.equal(g, w)
    assert _np(sa.episodes).any()
    assert torch.equal(a.learner_episodes(), ep) and torch.equal(a.get_q().view(torch.int32), q.view(torch.int32))
    now = a.learner_schedule()
    assert all(np.array_equal(now[k], sched[k]) for k in sched)
    assert a.eval_kernel_name(K) == b.eval_kernel_name(K) and "SCHED" not in a.eval_kernel_name(K)
    assert a.learn_kernel_name(K) == _name(handle, "numpy", algo)
    _assert_same_handles(a, b, "numpy")
    a.close(); b.close()


@pytest.mark.parametrize("rng", cases.RNGS)
@pytest.mark.parametrize("algo", ["sarsa", "double_q"])
def test_two_shards_with_their_rows_equal_the_whole(algo, rng):
    handle = "s8_max5"
    whole = _scheduled(handle, rng, algo, "both", off=0)
    outs = [whole.rollout_learn(K) for _ in range(2)]
    q, ep = whole.get_q(), whole.learner_episodes()
    for lo in (0, N // 2):
        sl = slice(lo, lo + N // 2)
        sh = _scheduled(handle, rng, algo, "both", n=N // 2, off=lo, lo=lo)
        assert np.array_equal(sh.learner_schedule()["row"], cases.rows(N)[sl])
        for launch in range(2):
            for g, w in zip(sh.rollout_learn(K), outs[launch]):
                assert torch.equal(g, w[:, sl]), (algo, rng, lo, launch)
        assert torch.equal(sh.get_q().view(torch.int32), q[sl].view(torch.int32)) and torch.equal(sh.learner_episodes(), ep[sl])
        sh.close()
    whole.close()


# ---- graph replay
@pytest.mark.parametrize("summary", [False, True])
def test_captured_scheduled_launch_continues_the_schedule_at_every_replay(summary):
    handle, algo, rng = "s8_max5", "sarsa", "philox"
    a, b = _scheduled(handle, rng, algo, "both"), _scheduled(handle, rng, algo, "both")
    sa, sb = (a.episode_summary(), b.episode_summary()) if summary else (None, None)
    out_a = None if summary else a._alloc_rollout_closed(K)

    def call(e, s, out=None):
        return e.rollout_learn(K, summary=s) if summary else e.rollout_learn(K, out)

    call(a, sa, out_a); call(b, sb)                         # the eager launch before the capture (fills, LDS attribute)
    g = gr.capture(a, lambda: call(a, sa, out_a), K)
    for replay in range(3):
        ep0 = _np(a.learner_episodes())
        g.replay()
        out_b = call(b, sb)
        if summary:
            for x, y in zip(sa.tensors(), sb.tensors()):
                assert torch.equal(x, y), replay
        else:
            for name, x, y in zip(("obs", "reward", "terminated", "truncated", "actions"), out_a, out_b):
                assert torch.equal(x.view(torch.uint8) if x.dtype == torch.bool else x, y.view(torch.uint8) if y.dtype == torch.bool else y), (replay, name)
        assert torch.equal(a.get_q().view(torch.int32), b.get_q().view(torch.int32)), replay
        assert torch.equal(a.learner_episodes(), b.learner_episodes()), replay
        assert (_np(a.learner_episodes()) > ep0).all(), replay                 # (max_episode_steps = 5: every env ends episodes in 37 steps)
        # the counter moves between the replays too: five eager steps on both handles
        for x, y in zip(a.rollout_learn(5), b.rollout_learn(5)):
            assert torch.equal(x, y), replay
    assert _tick(a) == _tick(b) == 4 * K + 15
    _assert_same_handles(a, b, rng)
    m = cases.HANDLES[handle][2]
    ep = _np(a.learner_episodes())
    assert (ep >= m).any() and ep.min() > 8
    a.close(); b.close()


# ---- refusals: each leaves what is in force
def test_a_handle_with_noise_levels_is_refused_and_levels_are_refused_under_a_schedule():
    cfg = dict(sweep._S8, reward_noise=0.5)
    a = _mk(cfg, "numpy", n=64)
    a.set_learner("q_learning", alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=SEED)
    lv = np.linspace(0.0, 2.0, 64)
    a.set_noise_levels(reward_noise=lv)
    with pytest.raises(NotImplementedError, match="an epsilon/alpha schedule with per-env noise levels / one MDP per env: not built"):
        a.set_learner_schedule(epsilon=[0.5, 0.1])
    assert a.learner_schedule() is None and np.array_equal(a.noise_levels()[1], lv)
    assert a.learn_kernel_name(K).endswith(",PE=1,NLEV=1>")
    a.clear_noise_levels()
    a.set_learner_schedule(epsilon=[0.5, 0.1])
    assert a.learn_kernel_name(K).endswith(",PE=1,SCHED=1>")
    with pytest.raises(NotImplementedError, match="an epsilon/alpha schedule with per-env noise levels / one MDP per env: not built"):
        a.set_noise_levels(reward_noise=lv)
    assert a.learn_kernel_name(K).endswith(",PE=1,SCHED=1>") and np.array_equal(a.learner_schedule()["epsilon"], np.array([[0.5, 0.1]], np.float32))
    assert np.array_equal(a.noise_levels()[1], np.full(64, 0.5))
    a.rollout_learn(5)
    assert not a.status().any()
    a.clear_learner_schedule()
    assert a.learner_schedule() is None and a.learn_kernel_name(K).endswith("QLDS=1>")
    a.set_noise_levels(reward_noise=lv)
    assert a.learn_kernel_name(K).endswith(",PE=1,NLEV=1>")
    a.close()


def test_a_per_env_mdp_learner_a_missing_learner_and_a_continuous_env_are_refused():
    from mdp_playground_amd import RLToyVectorEnv, _capi as capi
    cfg = dict(sweep._S8)
    cfg.pop("seed")
    pm = RLToyVectorEnv(seeds=list(range(1, 65)), **cfg)
    pm.set_learner("q_learning", alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=SEED, per_env_mdp=True)
    name = pm.learn_kernel_name(K)
    with pytest.raises(NotImplementedError, match="an epsilon/alpha schedule with per-env noise levels / one MDP per env: not built"):
        pm.set_learner_schedule(alpha=[0.5, 0.1])
    assert pm.learner_schedule() is None and pm.learn_kernel_name(K) == name and ",PM=" in name
    pm.rollout_learn(5)
    pm.close()
    a = _mk(cases.HANDLES["cfg2"][0], "numpy", n=64)
    with pytest.raises(capi.MdppError, match="no learner"):
        a.set_learner_schedule(epsilon=[0.5, 0.1])
    with pytest.raises(capi.MdppError, match="no learner"):
        a.learner_episodes()
    a.set_learner("q_learning", alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=SEED)
    with pytest.raises(capi.MdppError, match="no schedule"):
        a.learner_episodes()
    with pytest.raises(capi.MdppError, match="no schedule"):
        a.set_learner_episodes()
    for bad in (dict(), dict(epsilon=np.zeros((2, 3))), dict(epsilon=[1.5]), dict(alpha=[0.0]), dict(epsilon=np.zeros((2, 3)), row=np.zeros(63, int)),
                dict(epsilon=np.zeros((2, 3)), row=np.full(64, 2))):
        with pytest.raises(ValueError):
            a.set_learner_schedule(**bad)
    assert a.learner_schedule() is None and "SCHED" not in a.learn_kernel_name(K)
    a.set_learner_schedule(epsilon=[0.5, 0.1])
    a.set_learner("sarsa", alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=SEED)          # a new learner drops the schedule
    assert a.learner_schedule() is None and "SCHED" not in a.learn_kernel_name(K)
    a.set_learner_schedule(epsilon=[0.5, 0.1])
    a.rollout_learn(K)
    assert _np(a.learner_episodes()).any()
    a.set_learner_schedule(epsilon=[0.5, 0.1])                                        # setting it again zeroes the counters
    assert not _np(a.learner_episodes()).any()
    a.set_learner(None)
    assert a.learner_schedule() is None
    a.close()
    c = RLToyVectorEnv(num_envs=64, **_CONT)
    with pytest.raises(NotImplementedError, match="discrete"):
        c.set_learner_schedule(epsilon=[0.5, 0.1])
    c.close()


@pytest.mark.parametrize("algo", ["q_learning", "double_q"])
def test_the_scheduled_parameter_is_refused_by_set_learner_rates_and_the_free_one_is_set(algo):
    from mdp_playground_amd import _capi as capi
    handle = "s8_max5"
    a = _scheduled(handle, "numpy", algo, "eps")
    r = Restated(a, handle, algo, "eps")
    _check_launch(a, r, K, "scheduled")
    for bad in (dict(epsilon=0.5), dict(epsilon=np.full(N, 0.5)), dict(alpha=0.5, epsilon=0.5)):
        with pytest.raises(capi.MdppError, match="clear_learner_schedule"):
            a.set_learner_rates(**bad)
    # the library's own refusals: MDPP_ESTATE, the reason names the way out
    eps_host = np.full(N, 0.5, np.float32)
    assert a._lib.mdpp_set_learner_rates(a._h, 0.5, 0.5) == capi.ESTATE
    assert b"mdpp_clear_learner_schedule" in a._lib.mdpp_last_error(a._h)
    assert a._lib.mdpp_set_learner_params(a._h, None, None, capi.nptr(eps_host), None) == capi.ESTATE
    assert b"mdpp_clear_learner_schedule" in a._lib.mdpp_last_error(a._h)
    _check_launch(a, r, 9, "after the refused calls: unchanged")
    a.set_learner_rates(alpha=0.5)                              # alpha is free under an epsilon schedule
    r.agent.al0[:] = np.float32(0.5)
    _check_launch(a, r, 9, "alpha set under the epsilon schedule")
    a.set_learner_rates(gamma=0.5)
    r.agent.ga[:] = np.float32(0.5)
    _check_launch(a, r, 9, "gamma set under the schedule")
    assert a.learn_kernel_name(K) == _name(handle, "numpy", algo)
    # an alpha schedule owns alpha, and epsilon is free
    b = _scheduled(handle, "numpy", algo, "alpha")
    with pytest.raises(capi.MdppError, match="clear_learner_schedule"):
        b.set_learner_rates(alpha=0.5)
    assert b._lib.mdpp_set_learner_params(b._h, capi.nptr(eps_host), None, None, None) == capi.ESTATE
    rb = Restated(b, handle, algo, "alpha", eps=0.75)
    b.set_learner_rates(epsilon=0.75)
    _check_launch(b, rb, K, "epsilon set under the alpha schedule")
    assert not a.status().any() and not b.status().any()
    a.close(); b.close()
