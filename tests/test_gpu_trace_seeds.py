"""Eligibility traces on ONE MDP PER ENV on the GPU: RLToyVectorEnv(seeds=[...]) with set_learner(..., per_env_mdp=True) and
set_learner_traces(..., per_env_mdp=True); the PM = 1 / PM = 2 forms of k_discrete_trace_rollout / _summary / _summary_log, with
and without SCHED (include/mdpp.h "Traces on one MDP per env").

Every launch is held, bit for bit, to the yardsticks of tests/test_gpu_per_env_mdp.py and tests/test_gpu_learn_traces.py:
  twin         an identical seeds= handle fed the returned actions through rollout(): outputs (reward by bits), state record,
               env and space streams, status and step counter all equal;
  restatement  tests/learner_trace_ref.py fed the launch's own outputs with P[i] per env (per_env_mdp_cpu.PerEnvP): actions,
               get_q() and get_traces();
  CPU loop     (Philox handles) tests/trace_seed_cases.closed_loop: one oracle env per seed driven by the restatement --
               actions, outputs, Q and Z.
The set-up is per_env_mdp_cpu's: N = 320 (one full workgroup and 64 lanes of a second), seeds 100 ... 419, env_id_offset 1000,
K = 37, two launches and a third after reset(mask=).  What the passes must have exercised is learner_trace_cases.honest(),
shown reachable on the CPU by tests/test_trace_seed_cases_host.py.  No tolerance anywhere.

Placements, asserted by kernel name: at S = A = 8 Q and Z take 128 KiB of a workgroup's 160 KiB and the envs' MDP slots
40 - 52 KiB, so Q and Z go to LDS and the MDPs are read in global memory (QLDS=1, PM=1); S = A = 20 has neither in LDS
(QLDS=0, PM=1); S = A = 5 and 7 have both (QLDS=1, PM=2) and run again in the three placements the options force."""
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
import per_env_mdp_cpu as pm
import test_gpu_per_env_mdp as pe
import trace_seed_cases as tsc
from test_gpu_per_env_mdp import ODD, _assert_same_handles, _assert_same_outputs, _bits, _np, _obs_now, _tick

pytestmark = pytest.mark.gpu

N, K, OFF, SEED = tsc.N, tsc.K, tsc.OFF, tsc.SEED
ALPHA, GAMMA, EPS, LAMBDA = cases.ALPHA, cases.GAMMA, cases.EPS, cases.LAMBDA
PLACEMENTS = [(), ("NO_PM_LDS",), ("NO_LEARN_LDS",), ("NO_PM_LDS", "NO_LEARN_LDS")]


def _mk(cfg, rng, seeds=pm.SEEDS, off=OFF, **kw):
    from mdp_playground_amd import RLToyVectorEnv
    extra = dict(rng="philox", philox_seed=pm.PHILOX_SEED) if rng == "philox" else {}
    return RLToyVectorEnv(seeds=list(seeds), env_id_offset=off, **extra, **kw, **cfg)


def _traced(handle, rng, algo, kind, form="uniform", seeds=pm.SEEDS, off=OFF, lo=0, opts=(), lam=None, cfg=None, traces=True):
    """a seeds= handle of the case with its per_env_mdp learner and (traces) its traces; env i takes entry lo + i of the per-env cycles"""
    c, kw = tsc.HANDLES[handle] if cfg is None else (cfg, {})
    e = _mk(c, rng, seeds, off, **kw)
    if opts:
        e.set_kernel_options(*opts)
    al, ga, ep, lm = cases.params(form, len(seeds), lo)
    e.set_learner(algo, alpha=al, gamma=ga, epsilon=ep, seed=SEED, per_env_mdp=True)
    assert e.learner_traces is None
    if traces:
        e.set_learner_traces(lm if lam is None else lam, kind, per_env_mdp=True)
        assert e.learner_traces == kind
    return e


class Restated:
    """the restatement on one MDP per env, carried from launch to launch beside a handle"""

    def __init__(self, cfg, algo, kind, form="uniform", seeds=pm.SEEDS, off=OFF, lo=0, autoreset=ref.SAME_STEP, lam=None, sched=None):
        mdps = pm.build_mdps(cfg, seeds)
        m, n = mdps[0], len(mdps)
        self.P, self.off = pm.PerEnvP(mdps), off
        al, ga, ep, lm = cases.params(form, n, lo)
        self.agent = tref.TraceAgent(algo, n, al, ga, ep, lm if lam is None else lam, kind, np.zeros((n, m.S, m.A), np.float32),
                                     autoreset, sched=sched)

    def launch(self, tick0, obs_before, out):
        obs, rew, term, trunc = (_np(x) for x in out[:4])
        k, n = obs.shape
        w = [ref.tick_words(SEED, self.off, tick0, k + 1, n, st) for st in (ref.EXPLORE_STREAM, ref.ACTION_STREAM)]
        return tref.run(self.agent, obs_before, obs, rew, term, trunc, self.P, *w)


def _same_bits(got, want, what):
    assert got.dtype == np.float32 and got.shape == want.shape, what
    assert np.array_equal(_bits(got), _bits(want)), (what, np.argwhere(_bits(got) != _bits(want))[:5])


def _check_tables(a, r, what):
    _same_bits(_np(a.get_q()), r.agent.Q, (what, "Q"))
    z = a.get_traces()
    assert z.dtype == torch.float32 and z.device == a.device and tuple(z.shape) == r.agent.Z.shape
    _same_bits(_np(z), r.agent.Z, (what, "Z"))


def _check_launch(a, r, k, what):
    """one learning launch of handle a against the restatement r (actions, Q, Z); returns its outputs"""
    before, tick0 = _obs_now(a), _tick(a)
    out = a.rollout_learn(k)
    assert out[4].dtype == torch.int32 and tuple(out[4].shape) == (k, a.num_envs)
    want = r.launch(tick0, before, out)
    got = _np(out[4])
    assert np.array_equal(got, want), (what, "actions", np.argwhere(got != want)[:5])
    _check_tables(a, r, what)
    return out


def _placement(cfg, *options):
    """(QLDS, PM) by the rule of include/mdpp.h: test_gpu_per_env_mdp._placement with Q and Z counted together -- two tables,
    what it counts for double_q"""
    return pe._placement(cfg, "double_q", *options)


def _name(cfg, rng, placement, summary=False, sched=False):
    qlds, pmv = placement
    return "%s<PHILOX=%d,NOISE=%d,UNIT=%d,QLDS=%d,PE=1,PM=%d%s>" % (
        "k_discrete_trace_summary" if summary else "k_discrete_trace_rollout", rng == "philox", "transition_noise" in cfg,
        "reward_dist" not in cfg, qlds, pmv, ",SCHED=1" if sched else "")


def _same_tables(a, b, what):
    assert torch.equal(a.get_q().view(torch.int32), b.get_q().view(torch.int32)), (what, "Q")
    assert torch.equal(a.get_traces().view(torch.int32), b.get_traces().view(torch.int32)), (what, "Z")


def _equal_launches(a, b, launches, what, k=K, traces=True):
    for launch in range(launches):
        for name, g, w in zip(("obs", "reward", "terminated", "truncated", "actions"), a.rollout_learn(k), b.rollout_learn(k)):
            assert torch.equal(g, w), (what, launch, name)
    assert torch.equal(a.get_q().view(torch.int32), b.get_q().view(torch.int32)), what
    if traces:
        assert torch.equal(a.get_traces().view(torch.int32), b.get_traces().view(torch.int32)), what


def _assert_cpu_loop(agent, traj, a, stacked, what):
    obs, rew, term, trunc, act = stacked
    for name, g, w in (("actions", act, traj["actions"]), ("obs", obs, traj["obs"]), ("terminated", term.astype(bool), traj["terminated"]),
                       ("truncated", trunc.astype(bool), traj["truncated"]), ("reward", _bits(rew), _bits(traj["reward"]))):
        assert np.array_equal(g, w), (what, "CPU loop", name, np.argwhere(g != w)[:5])
    _same_bits(_np(a.get_q()), agent.Q, (what, "CPU loop", "Q"))
    _same_bits(_np(a.get_traces()), agent.Z, (what, "CPU loop", "Z"))


# ---- twin, restatement, CPU loop, get_traces and the name.  (Before this form existed the handle was refused: the library's
#      "eligibility traces with one MDP per env: not built", NotImplementedError -- and set_learner_traces took no per_env_mdp.)
@pytest.mark.parametrize("handle,algo,kind,rng,form", tsc.all_cases())
def test_trace_seed_launch_twin_restatement_and_cpu_loop(handle, algo, kind, rng, form):
    cfg, kw = tsc.HANDLES[handle]
    a, b = _traced(handle, rng, algo, kind, form), _mk(cfg, rng, **kw)
    placement = _placement(cfg)
    assert placement == {"s20": (0, 1)}.get(handle, (1, 1))      # (the arithmetic of this file's docstring)
    assert a.learn_kernel_name(K) == _name(cfg, rng, placement), a.learn_kernel_name(K)
    assert not _np(a.get_traces()).any()
    assert np.array_equal(_obs_now(a), _obs_now(b))
    r = Restated(cfg, algo, kind, form, autoreset=kw.get("autoreset", ref.SAME_STEP))
    what = (handle, algo, kind, rng, form)
    outs = []
    for launch in range(tsc.LAUNCHES):
        assert _tick(a) == launch * K
        out = _check_launch(a, r, K, what + (launch,))
        _assert_same_outputs(out[:4], b.rollout(out[4]), what + (launch,))
        outs.append([_np(x) for x in out])
    _assert_same_handles(a, b, rng)
    cases.honest(handle, algo, kind, r.agent.info, tsc.LAUNCHES)
    nz = pm.nonzero_envs(r.agent.Q)
    assert nz[:256].any() and nz[256:].any()
    if rng == "philox":
        al, ga, ep, lam = cases.params(form, N)
        agent, traj = tsc.closed_loop(cfg, kw, algo, kind, al, ga, ep, lam)
        _assert_cpu_loop(agent, traj, a, [np.concatenate([o[j] for o in outs]) for j in range(5)], what)
    # a third launch after reset(mask=): the masked envs start an episode, their Q and Z stay
    mask = torch.as_tensor(np.random.default_rng(5).random(N) < 0.4, device=a.device)
    oa, _ = a.reset(mask=mask)
    ob, _ = b.reset(mask=mask)
    assert torch.equal(oa, ob)
    r.agent.pending[_np(mask)] = False              # (a reset env's next call is a step)
    _check_tables(a, r, what + ("after reset",))
    out = _check_launch(a, r, K, what + ("third",))
    _assert_same_outputs(out[:4], b.rollout(out[4]), what + ("third",))
    _assert_same_handles(a, b, rng)
    print(handle, algo, kind, rng, form, {k: v for k, v in r.agent.info.items() if not isinstance(v, np.ndarray)})
    a.close(); b.close()


# ---- no size a multiple of 4 (the slots pack bytes into dwords): Q, Z and the MDPs in LDS, then every forced placement
@pytest.mark.parametrize("rng", ["numpy", "philox"])
@pytest.mark.parametrize("shape,algo,kind", [("odd_unit", "q_learning", tref.ACCUMULATING), ("odd_rdist", "sarsa", tref.REPLACING)])
def test_odd_shapes_in_every_placement(shape, algo, kind, rng):
    cfg = ODD[shape]
    assert _placement(cfg) == (1, 2)
    want = {(): (1, 2), ("NO_PM_LDS",): (1, 1), ("NO_LEARN_LDS",): (0, 2), ("NO_PM_LDS", "NO_LEARN_LDS"): (0, 1)}
    hs = []
    for options in PLACEMENTS:
        e = _traced(None, rng, algo, kind, "pe", opts=options, cfg=cfg)
        assert _placement(cfg, *options) == want[options]
        assert e.learn_kernel_name(K) == _name(cfg, rng, want[options]), (options, e.learn_kernel_name(K))
        hs.append(e)
    a, b = hs[0], _mk(cfg, rng)
    r = Restated(cfg, algo, kind, "pe")
    for launch in range(tsc.LAUNCHES):
        out = _check_launch(a, r, K, (shape, rng, launch))
        _assert_same_outputs(out[:4], b.rollout(out[4]), (shape, rng, launch))
        for options, e in zip(PLACEMENTS[1:], hs[1:]):
            for name, g, w in zip(("obs", "reward", "terminated", "truncated", "actions"), e.rollout_learn(K), out):
                assert torch.equal(g, w), (shape, rng, options, launch, name)
            _same_tables(e, a, (shape, rng, options, launch))
    assert (r.agent.Z != 0).any() and r.agent.info["ends"] > 0
    if rng == "philox":
        al, ga, ep, lam = cases.params("pe", N)
        agent, _ = tsc.closed_loop(cfg, {}, algo, kind, al, ga, ep, lam)
        _same_bits(_np(a.get_q()), agent.Q, (shape, "CPU loop", "Q"))
        _same_bits(_np(a.get_traces()), agent.Z, (shape, "CPU loop", "Z"))
    for e in hs:
        _assert_same_handles(e, b, rng)
        e.close()
    b.close()


# ---- sizes: one lane, a wave less one, a workgroup and one (tail lanes of a PM = 2 workgroup stage the last env's tables)
@pytest.mark.parametrize("k", [1, 7])
@pytest.mark.parametrize("n", [1, 63, 257])
def test_small_and_odd_sizes(n, k):
    cfg = ODD["odd_unit"]
    algo, kind, rng = ("q_learning", "sarsa")[n % 2], cases.KINDS[k % 2], ("numpy", "philox")[(n + k) % 2]
    form, seeds = ("pe" if n > 1 else "uniform"), pm.SEEDS[:n]
    a, b = _traced(None, rng, algo, kind, form, seeds=seeds, cfg=cfg), _mk(cfg, rng, seeds=seeds)
    # (one env: its one MDP is a shared MDP, the flags change nothing -- the shared-MDP kernel, uniform parameters)
    name = a.learn_kernel_name(k)
    assert name == (_name(cfg, rng, (1, 2)) if n > 1 else "k_discrete_trace_rollout<PHILOX=%d,NOISE=0,UNIT=1,QLDS=1>" % (rng == "philox")), name
    r = Restated(cfg, algo, kind, form, seeds=seeds)
    for launch in range(3):
        out = _check_launch(a, r, k, (n, k, launch))
        _assert_same_outputs(out[:4], b.rollout(out[4]), (n, k, launch))
    assert (r.agent.Z != 0).any() or k == 1
    _assert_same_handles(a, b, rng)
    a.close(); b.close()


# ---- a call sent out in pieces: Z and sarsa's action cross them
@pytest.mark.parametrize("rng", ["numpy", "philox"])
def test_a_call_sent_out_in_pieces_equals_one_launch(rng):
    handle, algo, kind = "cfg2", "sarsa", tref.ACCUMULATING
    one, many = _traced(handle, rng, algo, kind, "pe"), _traced(handle, rng, algo, kind, "pe", opts=("LEARN_SHORT_PIECES",))
    assert one.learn_kernel_name(K) == many.learn_kernel_name(K)
    _equal_launches(many, one, 2, (rng, "pieces"))
    assert _np(one.get_traces()).any()
    s1, s2 = one.episode_summary(), many.episode_summary()          # ... and the summary form's pieces
    one.rollout_learn(K, summary=s1); many.rollout_learn(K, summary=s2)
    for g, w in zip(s2.tensors(), s1.tensors()):
        assert torch.equal(g, w), rng
    _same_tables(many, one, (rng, "summary pieces"))
    _assert_same_handles(one, many, rng)
    one.close(); many.close()


# ---- summary= and log= against the full-output launch and the rules of DESIGN.md 3.13 / 3.24
LOG_M = 6
SENTINEL_RET, SENTINEL_LEN = -12345.5, -7


def _bits5(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int64) if x.dtype == np.float64 else x.view(np.int32) if x.dtype == np.float32 else x


@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("handle,algo,kind,rng,form", [
    ("s8_max5", "q_learning", tref.ACCUMULATING, "numpy", "uniform"), ("cfg2", "sarsa", tref.REPLACING, "philox", "pe"),
    ("s8_next_max5", "sarsa", tref.ACCUMULATING, "philox", "uniform"), ("s8_noise", "q_learning", tref.REPLACING, "numpy", "pe"),
    ("s20", "q_learning", tref.REPLACING, "philox", "uniform")])
def test_summary_and_log_launches_equal_the_full_output_launch(handle, algo, kind, rng, form, log):
    cfg, kw = tsc.HANDLES[handle]
    full, summ = _traced(handle, rng, algo, kind, form), _traced(handle, rng, algo, kind, form)
    assert summ.learn_kernel_name(K) == _name(cfg, rng, _placement(cfg))
    s = summ.episode_summary()
    lg = summ.episode_log(LOG_M) if log else None
    want_log = None
    if log:
        lg.ret.fill_(SENTINEL_RET); lg.len.fill_(SENTINEL_LEN)
        want_log = lref.new_log(N, LOG_M, SENTINEL_RET, SENTINEL_LEN)
    st5, pending = lref.new_state5(N), None
    for launch in range(tsc.LAUNCHES):
        what = (handle, algo, kind, rng, form, log, launch)
        out = full.rollout_learn(K)
        assert summ.rollout_learn(K, summary=s, log=lg) is s
        rew, term, trunc = _np(out[1]), _np(out[2]), _np(out[3])
        reset_call, pending = sumref.reset_calls(term, trunc, kw.get("autoreset", ref.SAME_STEP), pending)
        if log:
            want_log, st5 = lref.run(rew, term, trunc, reset_call, st5, want_log)
            for name, t in zip(("count", "ret", "len"), lg.tensors()):
                assert np.array_equal(_bits5(_np(t)), _bits5(want_log[name])), (what, "log." + name)
        else:
            st5 = sumref.summary(rew, term, trunc, reset_call, st5)
        for (name, _), t in zip(sumref.FIELDS, s.tensors()):
            assert np.array_equal(_bits5(_np(t)), _bits5(st5[name])), (what, name)
        _same_tables(summ, full, what)
        assert _np(s.episodes).any()
    _assert_same_handles(full, summ, rng)
    assert _np(summ.get_traces()).any()
    full.close(); summ.close()


@pytest.mark.parametrize("rng", ["numpy", "philox"])
def test_evaluation_between_two_learning_launches_leaves_q_and_z(rng):
    handle, algo, kind = "s8", "sarsa", tref.ACCUMULATING
    cfg, kw = tsc.HANDLES[handle]
    a, b = _traced(handle, rng, algo, kind), _mk(cfg, rng, **kw)
    r = Restated(cfg, algo, kind)
    out = _check_launch(a, r, K, (rng, "first"))
    b.rollout(out[4])
    zb, qb = a.get_traces(), a.get_q()
    assert _np(zb).any()
    e_out = a.rollout_eval(K)
    a.rollout_eval(K, summary=a.episode_summary())
    assert torch.equal(a.get_traces().view(torch.int32), zb.view(torch.int32)) and torch.equal(a.get_q().view(torch.int32), qb.view(torch.int32))
    assert "trace" not in a.eval_kernel_name(K) and ",PM=" in a.eval_kernel_name(K)
    _assert_same_outputs(e_out[:4], b.rollout(e_out[4]), (rng, "eval"))
    # the learner goes on where it was: a second learning launch on the tables and traces of the first.  (The restatement is
    # fed outputs, so it follows the env from wherever the evaluations left it; pending flags come from the evaluation.)
    r.agent.pending[:] = False                              # (same-step autoreset: no reset call is ever pending)
    a.reset(mask=torch.zeros(N, dtype=torch.bool, device=a.device))     # (the observation every env shows: a summary launch wrote none)
    a2 =_traced(handle, rng, algo, kind)                   # ... and against a handle that made the same calls with summary=
    s = a2.episode_summary()
    a2.rollout_learn(K, summary=s); a2.rollout_eval(K, summary=s); a2.rollout_eval(K, summary=s)
    _same_tables(a2, a, (rng, "the same calls as summaries"))
    out = _check_launch(a, r, K, (rng, "learn after eval"))
    a2.rollout_learn(K, summary=s)
    _same_tables(a2, a, (rng, "second learning launch"))
    a.close(); b.close(); a2.close()


# ---- the sweep schedule with traces, in both setting orders
@pytest.mark.parametrize("rng", cases.RNGS)
@pytest.mark.parametrize("algo,kind", [("q_learning", tref.ACCUMULATING), ("sarsa", tref.REPLACING)])
def test_sweep_schedule_with_traces_in_both_orders(algo, kind, rng):
    handle, m = tsc.SCHED_HANDLE, tsc.SCHED_M
    cfg, kw = tsc.HANDLES[handle]
    eps, al = scases.tables(tsc.SCHED_KIND, m)
    a = _traced(handle, rng, algo, kind)                                     # traces, then the schedule
    a.set_learner_schedule(epsilon=eps, alpha=al, row=scases.rows(N), sweep=True)
    c = _traced(handle, rng, algo, kind, traces=False)                       # the schedule, then traces
    c.set_learner_schedule(epsilon=eps, alpha=al, row=scases.rows(N), sweep=True)
    c.set_learner_traces(LAMBDA, kind, per_env_mdp=True)
    name = a.learn_kernel_name(K)
    assert name == c.learn_kernel_name(K) == _name(cfg, rng, (1, 1), sched=True) and name.endswith(",PM=1,SCHED=1>"), name
    r = Restated(cfg, algo, kind, sched=scases.schedule(tsc.SCHED_KIND, m, N))
    b = _mk(cfg, rng, **kw)
    s = c.episode_summary()
    lg = c.episode_log(LOG_M)
    for launch in range(tsc.LAUNCHES):
        out = _check_launch(a, r, K, (algo, kind, rng, launch))
        _assert_same_outputs(out[:4], b.rollout(out[4]), (algo, launch))
        assert np.array_equal(_np(a.learner_episodes()), r.agent.ep)
        # the other order, as the summary form (launch 0) and its log form (launch 1)
        c.rollout_learn(K, summary=s, log=lg if launch else None)
        _same_tables(c, a, ("other order", launch))
        assert torch.equal(c.learner_episodes(), a.learner_episodes())
    info = r.agent.info
    assert info["ends"] > 0 and info["alpha_changes"] > 0 and info["alpha_change_with_z"] > 0 and info["E_changes"] > 0, info
    assert (r.agent.ep >= m).any() and (r.agent.ep < m - 1).any()
    assert _np(lg.count).any()
    _assert_same_handles(a, c, rng)
    _assert_same_handles(a, b, rng)
    # clear_learner_schedule ends the sweep opt-in and leaves the traces
    a.clear_learner_schedule()
    assert a.learn_kernel_name(K) == _name(cfg, rng, (1, 1)) and a.learner_traces == kind
    a.close(); b.close(); c.close()


# ---- two unequal shards of one seeds list equal the whole
@pytest.mark.parametrize("rng", ["numpy", "philox"])
def test_two_unequal_shards_equal_the_whole(rng):
    handle, algo, kind, cut = "s8", "q_learning", tref.REPLACING, 100
    whole = _traced(handle, rng, algo, kind, "pe")
    lo = _traced(handle, rng, algo, kind, "pe", seeds=pm.SEEDS[:cut])
    hi = _traced(handle, rng, algo, kind, "pe", seeds=pm.SEEDS[cut:], off=OFF + cut, lo=cut)
    for launch in range(tsc.LAUNCHES):
        w, x, y = whole.rollout_learn(K), lo.rollout_learn(K), hi.rollout_learn(K)
        for name, g, p, q in zip(("obs", "reward", "terminated", "truncated", "actions"), w, x, y):
            assert torch.equal(g, torch.cat([p, q], dim=1)), (rng, launch, name)
    for get in ("get_q", "get_traces"):
        g = getattr(whole, get)()
        assert torch.equal(g.view(torch.int32), torch.cat([getattr(lo, get)(), getattr(hi, get)()]).view(torch.int32)), (rng, get)
    assert _np(whole.get_traces()).any()
    whole.close(); lo.close(); hi.close()


# ---- graph replay: every env's tables, Q and Z are read from the handle's buffers at replay; Z and the counter cross the replays
@pytest.mark.parametrize("summary", [False, True])
def test_captured_launch_replayed_three_times(summary):
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
    del g
    a.close(); b.close()


# ---- lambda = 0 is the traceless per-env-MDP learner
@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("algo", cases.ALGOS)
def test_lambda_0_equals_the_traceless_learner(algo, kind):
    """q + u 1 = q + u and Q[e] + u 0 = Q[e] while Q holds no -0 (it starts from +0 and rewards here are never negative)"""
    handle, rng = "cfg2", "philox"
    a = _traced(handle, rng, algo, kind, lam=0.0)
    b = _traced(handle, rng, algo, kind, traces=False)
    assert a.learn_kernel_name(K).startswith("k_discrete_trace_rollout<") and b.learn_kernel_name(K).startswith("k_discrete_learn_rollout<")
    assert a.learn_kernel_name(K).endswith(",PE=1,PM=1>") and b.learn_kernel_name(K).endswith(",PE=1,PM=2>")
    _equal_launches(a, b, 2, (algo, kind), traces=False)
    q = _np(a.get_q())
    assert (q != 0).any() and not np.signbit(q[q == 0]).any()
    assert not _np(a.get_traces()).any()                        # c = 0: nothing survives a sweep
    _assert_same_handles(a, b, rng)
    a.close(); b.close()


# ---- refusals and state
def _small(rng="numpy", algo="q_learning", cfg=None):
    e = _mk(tsc.HANDLES["s8"][0] if cfg is None else cfg, rng, seeds=pm.SEEDS[:64])
    e.set_learner(algo, alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=SEED, per_env_mdp=True)
    return e


def test_double_q_is_refused_with_the_opt_in():
    a = _small(algo="double_q")
    name = a.learn_kernel_name(K)
    with pytest.raises(NotImplementedError, match="eligibility traces with double_q: not built"):
        a.set_learner_traces(LAMBDA, per_env_mdp=True)
    assert a.learner_traces is None and a.learn_kernel_name(K) == name and "DOUBLE=1" in name
    # (the refused call left no opt-in behind: the plain call meets the refusal it met before)
    a.set_learner("sarsa", alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=SEED, per_env_mdp=True)
    with pytest.raises(NotImplementedError, match="eligibility traces with one MDP per env: not built"):
        a.set_learner_traces(LAMBDA)
    # the other order: set_learner("double_q") on a handle with traces starts a new learner, which drops them
    a.set_learner_traces(LAMBDA, per_env_mdp=True)
    a.set_learner("double_q", alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=SEED, per_env_mdp=True)
    assert a.learner_traces is None and a.learn_kernel_name(K) == name
    a.rollout_learn(5)
    assert not a.status().any()
    a.close()


def test_noise_levels_are_refused_with_the_opt_in_in_both_orders():
    cfg = dict(tsc.HANDLES["s8"][0], reward_noise=0.5)
    lv = np.linspace(0.0, 2.0, 64)
    a = _small(cfg=cfg)
    a.set_noise_levels(reward_noise=lv, per_env_mdp=True)
    with pytest.raises(NotImplementedError, match="eligibility traces with per-env noise levels: not built"):
        a.set_learner_traces(LAMBDA, per_env_mdp=True)
    assert a.learner_traces is None and np.array_equal(a.noise_levels()[1], lv) and ",NLEV=1,PM=" in a.learn_kernel_name(K)
    a.clear_noise_levels()
    a.set_learner_traces(LAMBDA, per_env_mdp=True)
    name = a.learn_kernel_name(K)
    assert name.startswith("k_discrete_trace_rollout<") and ",PM=" in name
    with pytest.raises(NotImplementedError, match="eligibility traces with per-env noise levels: not built"):
        a.set_noise_levels(reward_noise=lv, per_env_mdp=True)
    assert a.learner_traces == tref.REPLACING and a.learn_kernel_name(K) == name and np.array_equal(a.noise_levels()[1], np.full(64, 0.5))
    a.rollout_learn(5)
    assert not a.status().any()
    a.close()


def test_the_opt_in_its_refusals_and_what_ends_it():
    from mdp_playground_amd import RLToyVectorEnv
    cfg = tsc.HANDLES["s8"][0]
    # a shared MDP: ValueError; the C call is accepted and changes nothing; the sweep schedule with traces stays refused there
    shared = RLToyVectorEnv(num_envs=64, seed=0, **cfg)
    shared.set_learner("q_learning", alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=SEED)
    with pytest.raises(ValueError, match="per_env_mdp"):
        shared.set_learner_traces(LAMBDA, per_env_mdp=True)
    assert shared.learner_traces is None
    assert shared._lib.mdpp_learner_traces_per_env_mdp(shared._h, 1) == 0
    shared.set_learner_traces(LAMBDA)
    assert shared.learn_kernel_name(K) == "k_discrete_trace_rollout<PHILOX=0,NOISE=0,UNIT=1,QLDS=1>"
    with pytest.raises(NotImplementedError, match="eligibility traces with the schedule of mdpp_learner_schedule_sweep: not built"):
        shared.set_learner_schedule(epsilon=[0.5, 0.1], sweep=True)
    shared.close()
    # one MDP per env without the per_env_mdp learner: the learner's own refusal
    bare = _mk(cfg, "numpy", seeds=pm.SEEDS[:64])
    with pytest.raises(NotImplementedError, match="one shared MDP"):
        bare.set_learner_traces(LAMBDA, per_env_mdp=True)
    bare.close()
    # without the opt-in: refused as ever
    a = _small()
    plain = a.learn_kernel_name(K)
    with pytest.raises(NotImplementedError, match="eligibility traces with one MDP per env: not built"):
        a.set_learner_traces(LAMBDA)
    assert a.learner_traces is None and a.learn_kernel_name(K) == plain and plain.startswith("k_discrete_learn_rollout<")
    # with it: in force; a call without it is refused and traces, Z and the kernel's name stay
    a.set_learner_traces(LAMBDA, tref.ACCUMULATING, per_env_mdp=True)
    a.rollout_learn(K)
    z, name = a.get_traces().clone(), a.learn_kernel_name(K)
    assert _np(z).any() and name.startswith("k_discrete_trace_rollout<") and name.endswith(",PE=1,PM=1>")
    with pytest.raises(NotImplementedError, match="eligibility traces with one MDP per env: not built"):
        a.set_learner_traces(0.5)
    assert a.learner_traces == tref.ACCUMULATING and torch.equal(a.get_traces(), z) and a.learn_kernel_name(K) == name
    # set_traces / get_traces and a per-env lambda serve the handle
    a.set_traces(z * 0.5)
    assert torch.equal(a.get_traces(), z * 0.5)
    a.set_learner_traces(np.linspace(0.0, 1.0, 64).astype(np.float32), tref.REPLACING, per_env_mdp=True)
    assert a.learner_traces == tref.REPLACING and not _np(a.get_traces()).any() and a.learn_kernel_name(K) == name
    a.rollout_learn(5)
    # clear_learner_traces: the traceless PM kernel again, and the opt-in is over
    a.clear_learner_traces()
    assert a.learner_traces is None and a.learn_kernel_name(K) == plain
    with pytest.raises(NotImplementedError, match="eligibility traces with one MDP per env: not built"):
        a.set_learner_traces(LAMBDA)
    # set_learner drops the traces and the opt-in
    a.set_learner_traces(LAMBDA, per_env_mdp=True)
    a.set_learner("sarsa", alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=SEED, per_env_mdp=True)
    assert a.learner_traces is None and a.learn_kernel_name(K) == plain
    with pytest.raises(NotImplementedError, match="eligibility traces with one MDP per env: not built"):
        a.set_learner_traces(LAMBDA)
    # the C flag: off drops the traces; the learner's flag off drops learner and traces
    a.set_learner_traces(LAMBDA, per_env_mdp=True)
    assert a._lib.mdpp_learner_traces(a._h) == 2
    assert a._lib.mdpp_learner_traces_per_env_mdp(a._h, 0) == 0 and a._lib.mdpp_learner_traces(a._h) == 0
    assert a._lib.mdpp_learner_traces_per_env_mdp(a._h, 1) == 0 and a._lib.mdpp_set_learner_traces(a._h, 2, 0.5, None) == 0
    assert a._lib.mdpp_learner_per_env_mdp(a._h, 1) == 0 and a._lib.mdpp_learner_traces(a._h) == 2      # (on again while on: nothing changes)
    assert a._lib.mdpp_learner_per_env_mdp(a._h, 0) == 0 and a._lib.mdpp_learner_traces(a._h) == 0
    assert not a.status().any()
    a.close()
