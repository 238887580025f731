"""The episode log on the GPU (log= on rollout_learn with summary=; mdpp_step_n_learn_log; the k_discrete_learn_summary_log
kernels of every learner form; include/mdpp.h "Episode summaries").  rollout_eval keeps no log.

A launch with a log is held, bit for bit (float64 as int64), to a twin handle that makes the full-output call: the twin's
reward / terminated / truncated fed through the restatement tests/episode_log_ref.py give the three log arrays and the five
summary arrays; tables, state record, streams, tick -- and learner_episodes() under a schedule -- are the twin's.  The log's
ret / len are filled with a sentinel before the first launch and compared whole: entries at or beyond min(count, M) still hold
it.  N = 320, K = 37, two launches, env_id_offset = 1000; the cases, their M and what a pass must have exercised are in
tests/episode_log_cases.py, shown reachable on the CPU by tests/test_episode_log_host.py.  There is no tolerance anywhere
but on curve()'s mean return, a float64 sum in torch's order.  Without the feature every test fails: log= is a TypeError."""
import ctypes as C

import numpy as np
import pytest
import torch

import episode_log_cases as cases
import episode_log_ref as lref
import eval_summary_cases as esc
import eval_summary_ref as sref
import graph_replay_util as gr
import test_gpu_schedule_sweep as sweep
from test_gpu_learn_rollout import _assert_same_handles, _mk, _np, _tick

pytestmark = pytest.mark.gpu

N, K, OFF = cases.N, cases.K, cases.OFF
SEED, ALPHA, GAMMA, EPS = cases.SEED, cases.ALPHA, cases.GAMMA, cases.EPS
EINVAL = -1                       # MDPP_EINVAL


# ---- handles
def _make(case, algo, rng, n=N, lo=0, options=()):
    """a handle of the case with its learner, its levels and its schedule; envs lo ... lo + n - 1 of the case's N"""
    form, name, kind = cases.CASES[case]
    learner = algo
    q0 = cases.learner_tables(case, algo, lo + n)
    if form == "plain":
        cfg, kw = esc.SUMMARY_CASES[name]
        env = _mk(cfg, rng, n=n, env_id_offset=OFF + lo, **kw)
        if options:
            env.set_kernel_options(*options)
        env.set_learner(learner, alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=SEED, q=torch.as_tensor(q0[lo:], device=env.device))
        return env
    env = sweep._handle(form, name, rng, learner, n, lo, options)
    if kind is not None:
        sweep._schedule(env, form, name, kind, lo)
    if q0 is not None:
        env.set_q(torch.as_tensor(q0[lo:], device=env.device))
    return env


def _launch(env, algo, k, **kw):
    return env.rollout_learn(k, **kw)


def _new_log(env, M):
    """the handle's log with the sentinel in every ret / len entry, and the restatement's twin of it"""
    lg = env.episode_log(M)
    assert all(not t.any() for t in lg.tensors()) and lg.max_episodes == M
    lg.ret.fill_(cases.SENTINEL_RET)
    lg.len.fill_(cases.SENTINEL_LEN)
    return lg, lref.new_log(env.num_envs, M, cases.SENTINEL_RET, cases.SENTINEL_LEN)


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int64) if x.dtype == np.float64 else x.view(np.int32) if x.dtype == np.float32 else x


def _assert_log(lg, want, what):
    for name, t in zip(("count", "ret", "len"), lg.tensors()):
        g, w = _np(t), want[name]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        assert np.array_equal(_bits(g), _bits(w)), (what, "log." + name, np.argwhere(_bits(g) != _bits(w))[:5])


def _assert_summary(summ, st, what):
    for (name, dt), t in zip(lref.FIELDS5, summ.tensors()):
        g, w = _np(t), st[name]
        assert g.dtype == dt and g.shape == w.shape, (what, name)
        assert np.array_equal(_bits(g), _bits(w)), (what, name, np.argwhere(_bits(g) != _bits(w))[:5])


def _qbits(env):
    return env.get_q().view(torch.int32).clone()


def _same_learner(s, t, case, what):
    assert torch.equal(_qbits(s), _qbits(t)), (what, "Q")
    if cases.CASES[case][2] is not None:
        assert torch.equal(s.learner_episodes(), t.learner_episodes()), (what, "learner_episodes")


class Twin:
    """the full-output twin of a handle and the restatement fed with its outputs, carried from launch to launch"""

    def __init__(self, case, algo, rng, M, n=N, lo=0, options=()):
        self.case, self.algo = case, algo
        self.env = _make(case, algo, rng, n, lo, options)
        self.autoreset = cases.autoreset_of(case)
        self.st, self.log = lref.new_state5(n), lref.new_log(n, M, cases.SENTINEL_RET, cases.SENTINEL_LEN)
        self.pending, self.counters = None, lref.new_counters()

    def launch(self, k):
        out = _launch(self.env, self.algo, k)
        _, rew, term, trunc = (_np(x) for x in out[:4])
        rc, self.pending = sref.reset_calls(term, trunc, self.autoreset, self.pending)
        self.log, self.st = lref.run(rew, term, trunc, rc, self.st, self.log, self.counters)
        return out

    def pop(self):
        self.st = lref.pop5(self.st)


# ---- every form against the full-output twin and the restatement
@pytest.mark.parametrize("case,algo,rng", cases.RUNS)
def test_log_launch_equals_the_rule_on_the_full_output_twin(case, algo, rng):
    M = cases.LOG_M[case]
    s, t = _make(case, algo, rng), Twin(case, algo, rng, M)
    name = (s.eval_kernel_name(K), s.learn_kernel_name(K))
    summ = s.episode_summary()
    lg, _ = _new_log(s, M)
    for launch in range(cases.LAUNCHES):
        what = (case, algo, rng, launch)
        out = t.launch(K)
        assert _launch(s, algo, K, summary=summ, log=lg) is summ
        _assert_log(lg, t.log, what)
        _assert_summary(summ, t.st, what)
        _same_learner(s, t.env, case, what)
        assert _tick(s) == _tick(t.env) == (launch + 1) * K
    assert (s.eval_kernel_name(K), s.learn_kernel_name(K)) == name
    # the two consequences, on the device's own numbers: no pop() happened
    count, ret, ln = (_np(x) for x in lg.tensors())
    assert np.array_equal(count, _np(summ.episodes))
    whole = np.flatnonzero(count <= M)
    assert np.array_equal(np.where(np.arange(M)[:, None] < count[None, :], ln, 0).sum(axis=0)[whole], _np(summ.length_sum)[whole])
    rs = _np(summ.return_sum)
    for i in whole:
        acc = np.float64(0.0)
        for m in range(count[i]):
            acc = acc + ret[m, i]
        assert _bits(acc) == _bits(rs[i]), (case, algo, rng, "left-to-right sum", i)
    assert torch.equal(lg.filled(), lg.count.clamp(max=M))
    r0, l0 = lg.episodes_of(int(whole[0]))
    assert np.array_equal(r0, ret[:count[whole[0]], whole[0]]) and np.array_equal(l0, ln[:count[whole[0]], whole[0]])
    # the observation every env shows, the state record, the streams
    none = torch.zeros(N, dtype=torch.bool, device=s.device)
    assert torch.equal(s.reset(mask=none)[0], t.env.reset(mask=none)[0]) and torch.equal(t.env.reset(mask=none)[0], out[0][K - 1])
    _assert_same_handles(s, t.env, rng)
    print(case, algo, rng, M, t.counters)
    cases.honest(case, algo, t.counters)
    s.close(); t.env.close()


@pytest.mark.parametrize("m_of", ["one", "larger_than_any_count"])
def test_capacity_one_and_a_capacity_no_env_reaches(m_of):
    case, algo, rng = "s8_noise", "sarsa", "numpy"
    M = 1 if m_of == "one" else 2 * K + 1                 # (an env ends at most one episode per step)
    s, t = _make(case, algo, rng), Twin(case, algo, rng, M)
    summ = s.episode_summary()
    lg, _ = _new_log(s, M)
    for launch in range(cases.LAUNCHES):
        t.launch(K)
        _launch(s, algo, K, summary=summ, log=lg)
        _assert_log(lg, t.log, (m_of, launch))
        _assert_summary(summ, t.st, (m_of, launch))
    c = t.counters
    assert (c["over_M"] > 0 and c["under_M"] == c["zero"]) if M == 1 else (c["over_M"] == 0 and c["under_M"] == N), c
    if M > 1:
        n, mean_ret, mean_len = (_np(x) for x in lg.curve())
        count = t.log["count"]
        assert np.array_equal(n, (np.arange(M)[:, None] < count[None, :]).sum(axis=1)) and n[0] > 0 and n[-1] == 0
        assert np.isnan(mean_ret[-1]) and np.isnan(mean_len[-1])
        m0 = count > 0
        # (a float64 sum of at most N terms in another order: within N ulp of the sum of the magnitudes)
        r0 = t.log["ret"][0, m0]
        assert abs(mean_ret[0] - r0.mean()) <= N * 2.0 ** -52 * np.abs(r0).sum() / m0.sum() and mean_len[0] == t.log["len"][0, m0].mean()
    _assert_same_handles(s, t.env, rng)
    s.close(); t.env.close()


# ---- with a log == without one, on everything but the log
@pytest.mark.parametrize("algo", cases.ALGOS)
@pytest.mark.parametrize("case", ["cfg2", "pm_nlev_sched"])
def test_a_launch_with_a_log_equals_the_summary_launch_without_one_on_everything_else(case, algo):
    rng = "numpy"
    a, b = _make(case, algo, rng), _make(case, algo, rng)
    sa, sb = a.episode_summary(), b.episode_summary()
    lg, _ = _new_log(a, cases.LOG_M[case])
    names = (a.learn_kernel_name(K), a.eval_kernel_name(K))
    for launch in range(cases.LAUNCHES):
        _launch(a, algo, K, summary=sa, log=lg)
        _launch(b, algo, K, summary=sb)
        for name, x, y in zip(("ret", "len", "episodes", "return_sum", "length_sum"), sa.tensors(), sb.tensors()):
            assert torch.equal(x, y), (case, algo, launch, name)
        _same_learner(a, b, case, (case, algo, launch))
    assert torch.equal(lg.count, sb.episodes) and lg.count.any()
    assert (a.learn_kernel_name(K), a.eval_kernel_name(K)) == names == (b.learn_kernel_name(K), b.eval_kernel_name(K))
    _assert_same_handles(a, b, rng)
    a.close(); b.close()


@pytest.mark.parametrize("algo", cases.ALGOS)
def test_a_log_call_sent_out_in_pieces_equals_one_launch(algo):
    """LEARN_SHORT_PIECES: launches of at most 5 steps; count crosses the pieces through the caller's array, as ret and len do"""
    case, rng = "cfg2", "numpy"
    M = cases.LOG_M[case]
    one, many, t = _make(case, algo, rng), _make(case, algo, rng, options=("LEARN_SHORT_PIECES",)), Twin(case, algo, rng, M)
    s1, sm = one.episode_summary(), many.episode_summary()
    (l1, _), (lm, _) = _new_log(one, M), _new_log(many, M)
    for launch in range(2):
        _launch(one, algo, K, summary=s1, log=l1)
        _launch(many, algo, K, summary=sm, log=lm)
        t.launch(K)
        for lg, summ in ((l1, s1), (lm, sm)):
            _assert_log(lg, t.log, (algo, launch))
            _assert_summary(summ, t.st, (algo, launch))
    assert t.counters["spanning_logged"] > 0 and t.counters["over_M"] > 0, t.counters
    _assert_same_handles(one, many, rng)
    _assert_same_handles(one, t.env, rng)
    for e in (one, many, t.env):
        e.close()


# ---- sizes and shards
@pytest.mark.parametrize("n", [1, 63, 257])
@pytest.mark.parametrize("case", ["cfg2_disabled_max5", "pm_nlev_trunc"])
def test_sizes_with_launches_of_one_step(case, n):
    """max_episode_steps = 5: every env ends episodes within a few launches of one step, and M = 2 is passed"""
    algo, rng, M = "sarsa", "numpy", 2
    s, t = _make(case, algo, rng, n=n), Twin(case, algo, rng, M, n=n)
    summ = s.episode_summary()
    lg, _ = _new_log(s, M)
    for launch in range(24):                              # (next-step autoreset: an episode and its reset call take six steps at the most)
        t.launch(1)
        _launch(s, algo, 1, summary=summ, log=lg)
        _assert_log(lg, t.log, (case, n, launch))
        _assert_summary(summ, t.st, (case, n, launch))
    assert t.counters["over_M"] > 0 and t.counters["spanning_logged"] > 0, t.counters
    _same_learner(s, t.env, case, (case, n))
    _assert_same_handles(s, t.env, rng)
    s.close(); t.env.close()


@pytest.mark.parametrize("algo", ["sarsa", "double_q"])
@pytest.mark.parametrize("case", ["s8_noise", "pm_nlev_sched"])
def test_two_unequal_shards_equal_the_columns_of_the_whole(case, algo):
    rng, M = "philox", cases.LOG_M[case]
    whole = _make(case, algo, rng)
    summ = whole.episode_summary()
    lg, _ = _new_log(whole, M)
    for launch in range(2):
        _launch(whole, algo, K, summary=summ, log=lg)
    assert (lg.count > M).any() and (lg.count < M).any()
    for lo, n in ((0, 97), (97, 223)):
        sh = _make(case, algo, rng, n=n, lo=lo)
        ss = sh.episode_summary()
        ls, _ = _new_log(sh, M)
        for launch in range(2):
            _launch(sh, algo, K, summary=ss, log=ls)
        assert torch.equal(ls.count, lg.count[lo:lo + n]), (case, algo, lo)
        assert torch.equal(ls.ret.view(torch.int64), lg.ret[:, lo:lo + n].contiguous().view(torch.int64)), (case, algo, lo)
        assert torch.equal(ls.len, lg.len[:, lo:lo + n]), (case, algo, lo)
        for x, y in zip(ss.tensors(), summ.tensors()):
            assert torch.equal(x, y[lo:lo + n]), (case, algo, lo)
        assert not sh.status().any()
        sh.close()
    whole.close()


# ---- graph replay
@pytest.mark.parametrize("case,algo", [("pm_nlev_trunc", "sarsa"), ("cfg2_disabled_max5", "q_learning")])
def test_a_captured_log_launch_accumulates_across_replays(case, algo):
    rng, M = "philox", 2 * cases.LOG_M[case]
    a, b = _make(case, algo, rng), _make(case, algo, rng)
    sa, sb = a.episode_summary(), b.episode_summary()
    (la, _), (lb, _) = _new_log(a, M), _new_log(b, M)

    def call(e, s, lg):
        return _launch(e, algo, K, summary=s, log=lg)

    call(a, sa, la); call(b, sb, lb)                        # the eager launch before the capture (fills, LDS attribute)
    g = gr.capture(a, lambda: call(a, sa, la), K)
    for replay in range(3):
        before = la.count.clone()
        g.replay()
        call(b, sb, lb)
        for name, x, y in zip(("count", "ret", "len"), la.tensors(), lb.tensors()):
            assert torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x, y.view(torch.int64) if y.dtype == torch.float64 else y), (replay, name)
        for x, y in zip(sa.tensors(), sb.tensors()):
            assert torch.equal(x, y), replay
        assert (la.count > before).all(), replay             # (max_episode_steps = 5: every env ends episodes in 37 steps)
        _same_learner(a, b, case, replay)
        # eager launches of five steps in between, with the same log
        _launch(a, algo, 5, summary=sa, log=la); _launch(b, algo, 5, summary=sb, log=lb)
        assert torch.equal(la.count, lb.count), replay
    assert _tick(a) == _tick(b) == 4 * K + 15
    assert (la.count > M).any() and torch.equal(la.count, sa.episodes)
    assert not (la.len[:, (la.count >= M)] == cases.SENTINEL_LEN).any()
    _assert_same_handles(a, b, rng)
    a.close(); b.close()


# ---- pop()
@pytest.mark.parametrize("algo", ["q_learning", "double_q"])
def test_a_pop_between_launches_does_not_move_the_log(algo):
    case, rng = "cfg2_next_step", "numpy"
    M = cases.LOG_M[case]
    s, t = _make(case, algo, rng), Twin(case, algo, rng, M)
    summ = s.episode_summary()
    lg, _ = _new_log(s, M)
    popped = np.zeros(N, np.int64)
    for launch in range(3):
        t.launch(K)
        _launch(s, algo, K, summary=summ, log=lg)
        _assert_log(lg, t.log, (algo, launch))
        _assert_summary(summ, t.st, (algo, launch))
        kept = [x.clone() for x in lg.tensors()]
        popped += _np(summ.pop()[0])
        t.pop()
        assert all(torch.equal(x, y) for x, y in zip(kept, lg.tensors()))
        _assert_summary(summ, t.st, (algo, launch, "after pop"))
    assert np.array_equal(_np(lg.count), popped) and popped.any() and not _np(summ.episodes).any()
    _assert_same_handles(s, t.env, rng)
    s.close(); t.env.close()


# ---- refusals
def test_the_value_error_table_and_the_c_refusals_come_before_any_device_work():
    from mdp_playground_amd import _capi as capi
    from mdp_playground_amd.summary import EpisodeLog
    case, rng = "cfg2", "numpy"
    env, other = _make(case, "q_learning", rng), _make(case, "q_learning", rng, n=N - 1)
    q_before, state_before = _qbits(env), env.get_augmented_state()
    summ = env.episode_summary()
    wrong_dtype = env.episode_log(4)
    wrong_dtype.ret = wrong_dtype.ret.to(torch.float32)
    wrong_int = env.episode_log(4)
    wrong_int.count = wrong_int.count.to(torch.int64)
    strided = env.episode_log(4)
    strided.len = torch.zeros((4, 2 * N), dtype=torch.int32, device=env.device)[:, ::2]
    env_major = env.episode_log(4)
    env_major.ret = torch.zeros((N, 4), dtype=torch.float64, device=env.device).t()
    short = env.episode_log(4)
    short.len = short.len[:3]
    bad = (other.episode_log(4), EpisodeLog(N, 4, "cpu"), wrong_dtype, wrong_int, strided, env_major, short, "log", (1, 2, 3))
    with pytest.raises(TypeError):                       # rollout_eval keeps no log
        env.rollout_eval(K, summary=summ, log=env.episode_log(4))
    assert not hasattr(env._lib, "mdpp_step_n_eval_log")
    for call in (env.rollout_learn,):
        for lg in bad:
            with pytest.raises(ValueError):
                call(K, summary=summ, log=lg)
        with pytest.raises(ValueError):
            call(K, log=env.episode_log(4))
        with pytest.raises(ValueError):
            call(K, out=env.alloc_rollout_learn(K), log=env.episode_log(4))
        with pytest.raises(ValueError):
            call(K, out=env.alloc_rollout_learn(K), summary=summ, log=env.episode_log(4))
    with pytest.raises(ValueError):
        env.episode_log(0)
    # the library's own refusals: MDPP_EINVAL with a message
    lg = env.episode_log(4)
    five = [C.c_void_p(x.data_ptr()) for x in summ.tensors()]
    three = [C.c_void_p(x.data_ptr()) for x in lg.tensors()]
    for fn, what in ((env._lib.mdpp_step_n_learn_log, b"mdpp_step_n_learn_log"),):
        for j in range(3):
            args = list(three)
            args[j] = None
            assert fn(env._h, K, *five, *args, 4, None) == EINVAL
            assert what + b": null log buffer" in env._lib.mdpp_last_error(env._h)
        for m, msg in ((0, b"M < 1"), (-3, b"M < 1"), ((2 ** 31 - 1) // N + 1, b"M * num_envs > 2^31 - 1")):
            assert fn(env._h, K, *five, *three, m, None) == EINVAL
            assert what + b": " + msg in env._lib.mdpp_last_error(env._h)
        assert fn(env._h, 0, *five, *three, 4, None) == EINVAL and b"K < 1" in env._lib.mdpp_last_error(env._h)
    assert _tick(env) == 0 and torch.equal(_qbits(env), q_before)
    after = env.get_augmented_state()
    assert all(np.array_equal(after[k], state_before[k]) for k in after)
    assert all(not x.any() for x in summ.tensors() + lg.tensors())
    # a handle without a learner, and one the closed-loop launches do not serve: the _summary calls' refusals, word for word
    plain = _mk(esc.SUMMARY_CASES["cfg2"][0], rng)
    for call in (plain.rollout_learn,):
        with pytest.raises(capi.MdppError, match="no learner"):
            call(4, summary=plain.episode_summary(), log=plain.episode_log(2))
    plain.close()
    env.rollout_learn(K, summary=summ, log=lg)
    assert _tick(env) == K and not env.status().any() and lg.count.any()
    env.close(); other.close()
