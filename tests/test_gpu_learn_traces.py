"""Eligibility traces of the in-kernel learners on the GPU: SARSA(lambda) and Watkins's Q(lambda) (RLToyVectorEnv.set_learner_traces;
k_discrete_trace_rollout; include/mdpp.h "Eligibility traces").

Every launch is held to four things: the open-loop twin (an identically built handle fed with the actions the launch
returned: the four outputs, state record, streams, tick), the numpy restatement tests/learner_trace_ref.py fed with the
launch's own outputs (every action, Q and Z bit for bit), get_traces() and the kernel's name.  N = 320 envs (five waves, one
full workgroup and a partial one, resets diverging inside the waves), K = 37 (no multiple of 4), two launches and a third
after reset(mask=), env_id_offset = 1000.  What the passes must have exercised is stated in tests/learner_trace_cases.py and
shown reachable on the CPU by tests/test_learner_trace_cases_host.py.  No tolerance anywhere: every comparison is bit for bit.

A long call cut into pieces: the handle's real piece size is (2^32 - 1) / (8 N) steps -- 1.6 million at N = 320 -- and cannot
be reached in a test; the pieces' hand-over is run with MDPP_OPT_LEARN_SHORT_PIECES (pieces of 5 steps), as the other
learners' tests do."""
import numpy as np
import pytest
import torch

import learner_sweep_ref as ref
import learner_trace_cases as cases
import learner_trace_ref as tref
from test_gpu_learn_rollout import _assert_same_handles, _assert_same_outputs, _bits, _mk, _np, _obs_now, _tick

pytestmark = pytest.mark.gpu

N, K = 320, cases.K
OFF = 1000
SEED, ALPHA, GAMMA, EPS, LAMBDA = cases.SEED, cases.ALPHA, cases.GAMMA, cases.EPS, cases.LAMBDA


def _traced(handle, rng, algo, kind, form="uniform", n=N, off=OFF, opts=(), lam=None, cfg=None):
    """a handle of the case with its learner and its traces set"""
    c, kw = cases.HANDLES[handle] if cfg is None else (cfg, {})
    e = _mk(c, rng, n=n, env_id_offset=off, **kw)
    if opts:
        e.set_kernel_options(*opts)
    al, ga, ep, lm = cases.params(form, n)
    e.set_learner(algo, alpha=al, gamma=ga, epsilon=ep, seed=SEED)
    assert e.learner_traces is None
    e.set_learner_traces(lm if lam is None else lam, kind)
    assert e.learner_traces == kind
    return e


class Restated:
    """the restatement, carried from launch to launch beside a handle"""

    def __init__(self, env, algo, kind, form="uniform", off=OFF, autoreset=ref.SAME_STEP, lam=None, sched=None):
        mdp = env.mdps[0]
        n = env.num_envs
        self.P, self.off = np.asarray(mdp.P), off
        al, ga, ep, lm = cases.params(form, n)
        self.agent = tref.TraceAgent(algo, n, al, ga, ep, lm if lam is None else lam, kind, np.zeros((n, mdp.S, mdp.A), np.float32),
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


def _name(cfg, rng, form="uniform", summary=False, qlds=True, sched=False):
    return "%s<PHILOX=%d,NOISE=%d,UNIT=%d,QLDS=%d%s%s>" % (
        "k_discrete_trace_summary" if summary else "k_discrete_trace_rollout", rng == "philox", "transition_noise" in cfg,
        "reward_dist" not in cfg and not cfg.get("use_custom_mdp", False), qlds, ",PE=1" if form == "pe" or sched else "", ",SCHED=1" if sched else "")


def _equal_launches(a, b, launches, what, k=K, traces=True):
    for launch in range(launches):
        for name, g, w in zip(("obs", "reward", "terminated", "truncated", "actions"), a.rollout_learn(k), b.rollout_learn(k)):
            assert torch.equal(g, w), (what, launch, name)
    assert torch.equal(a.get_q().view(torch.int32), b.get_q().view(torch.int32)), what
    if traces:
        assert torch.equal(a.get_traces().view(torch.int32), b.get_traces().view(torch.int32)), what


# ---- twin, restatement, get_traces and the name
@pytest.mark.parametrize("handle,algo,kind,rng,form", cases.all_cases())
def test_trace_launch_twin_and_restatement(handle, algo, kind, rng, form):
    cfg, kw = cases.HANDLES[handle]
    a, b = _traced(handle, rng, algo, kind, form), _mk(cfg, rng, env_id_offset=OFF, **kw)
    assert a.learn_kernel_name(K) == _name(cfg, rng, form), a.learn_kernel_name(K)
    assert not _np(a.get_traces()).any()
    r = Restated(a, algo, kind, form, autoreset=kw.get("autoreset", ref.SAME_STEP))
    what = (handle, algo, kind, rng, form)
    for launch in range(cases.LAUNCHES):
        assert _tick(a) == launch * K
        out = _check_launch(a, r, K, what + (launch,))
        _assert_same_outputs(out[:4], b.rollout(out[4]), what + (launch,))
    cases.honest(handle, algo, kind, r.agent.info, cases.LAUNCHES)
    # a third launch after reset(mask=): the masked envs start an episode, their Q and Z stay (Z is the learner's, not the env's)
    mask = torch.as_tensor(np.random.default_rng(5).random(N) < 0.4, device=a.device)
    oa, _ = a.reset(mask=mask)
    ob, _ = b.reset(mask=mask)
    assert torch.equal(oa, ob)
    r.agent.pending[_np(mask)] = False              # (a reset env's next call is a step)
    _check_tables(a, r, what + ("after reset",))
    out = _check_launch(a, r, K, what + ("third",))
    _assert_same_outputs(out[:4], b.rollout(out[4]), what + ("third",))
    _assert_same_handles(a, b, rng)
    info = r.agent.info
    print(handle, algo, kind, rng, form, {k: v for k, v in info.items() if not isinstance(v, np.ndarray)})
    a.close(); b.close()


# ---- sizes: one lane, a wave less one, a workgroup and one; one step and seven
@pytest.mark.parametrize("k", [1, 7])
@pytest.mark.parametrize("n", [1, 63, 257])
def test_small_and_odd_sizes(n, k):
    handle, algo, kind, rng = "s8_max5", ("q_learning", "sarsa")[n % 2], cases.KINDS[k % 2], ("numpy", "philox")[(n + k) % 2]
    cfg, kw = cases.HANDLES[handle]
    form = "pe" if n > 1 else "uniform"
    a, b = _traced(handle, rng, algo, kind, form, n=n), _mk(cfg, rng, n=n, env_id_offset=OFF, **kw)
    r = Restated(a, algo, kind, form)
    for launch in range(3):
        out = _check_launch(a, r, k, (n, k, launch))
        _assert_same_outputs(out[:4], b.rollout(out[4]), (n, k, launch))
    assert (r.agent.Z != 0).any() or k == 1
    _assert_same_handles(a, b, rng)
    a.close(); b.close()


@pytest.mark.parametrize("algo", cases.ALGOS)
def test_one_action(algo):
    """A = 1: every selection is action 0, explored or not; Q(lambda) still cuts on the explore branch"""
    cfg = cases._custom(6, 1, (5,), 61)
    a, b = _traced(None, "philox", algo, tref.ACCUMULATING, cfg=cfg), _mk(cfg, "philox", env_id_offset=OFF)
    r = Restated(a, algo, tref.ACCUMULATING)
    for launch in range(2):
        out = _check_launch(a, r, K, (algo, launch))
        assert not _np(out[4]).any()
        _assert_same_outputs(out[:4], b.rollout(out[4]), (algo, launch))
    if algo == "q_learning":
        assert r.agent.info["cuts"] > 0 and r.agent.info["cut_greedy_action"] == r.agent.info["cuts"]
    a.close(); b.close()


# ---- the global-memory form: two tables that do not fit LDS, and the option that keeps Q out of it
@pytest.mark.parametrize("algo,kind", [("q_learning", tref.REPLACING), ("sarsa", tref.ACCUMULATING)])
def test_two_tables_beyond_lds_take_the_global_memory_form(algo, kind):
    """S = 64, A = 8: 256 lanes x 2 tables x 512 entries x 4 B = 1 MiB per workgroup"""
    cfg = cases._custom(64, 8, (3, 7), 648)
    a, b = _traced(None, "numpy", algo, kind, "pe", cfg=cfg), _mk(cfg, "numpy", env_id_offset=OFF)
    assert (a.mdps[0].S, a.mdps[0].A) == (64, 8)
    assert a.learn_kernel_name(K) == _name(cfg, "numpy", "pe", qlds=False), a.learn_kernel_name(K)
    r = Restated(a, algo, kind, "pe")
    for launch in range(2):
        out = _check_launch(a, r, K, (algo, launch))
        _assert_same_outputs(out[:4], b.rollout(out[4]), (algo, launch))
    assert (r.agent.Z != 0).any()
    _assert_same_handles(a, b, "numpy")
    a.close(); b.close()


@pytest.mark.parametrize("opt", ["NO_LEARN_LDS", "LEARN_SHORT_PIECES"])
@pytest.mark.parametrize("algo", cases.ALGOS)
def test_the_global_memory_form_and_pieces_equal_one_lds_launch(algo, opt):
    handle, kind = "cfg2", tref.ACCUMULATING
    cfg = cases.HANDLES[handle][0]
    one, other = _traced(handle, "numpy", algo, kind, "pe"), _traced(handle, "numpy", algo, kind, "pe", opts=(opt,))
    assert one.learn_kernel_name(K) == _name(cfg, "numpy", "pe")
    assert other.learn_kernel_name(K) == _name(cfg, "numpy", "pe", qlds=opt != "NO_LEARN_LDS")
    _equal_launches(other, one, 2, (algo, opt))                 # (pieces of 5 steps: Z and sarsa's action cross them)
    assert _np(one.get_traces()).any()
    _assert_same_handles(one, other, "numpy")
    one.close(); other.close()


# ---- lambda = 0 and lambda = 1
@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("algo", cases.ALGOS)
def test_lambda_0_equals_the_traceless_learner(algo, kind):
    """q + u 1 = q + u and Q[e] + u 0 = Q[e] while Q holds no -0 (it starts from +0 and rewards here are never negative)"""
    handle, rng = "cfg2", "philox"
    cfg, kw = cases.HANDLES[handle]
    a = _traced(handle, rng, algo, kind, lam=0.0)
    b = _mk(cfg, rng, env_id_offset=OFF, **kw)
    b.set_learner(algo, alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=SEED)
    assert a.learn_kernel_name(K).startswith("k_discrete_trace_rollout<") and b.learn_kernel_name(K).startswith("k_discrete_learn_rollout<")
    _equal_launches(a, b, 2, (algo, kind), traces=False)
    q = _np(a.get_q())
    assert (q != 0).any() and not np.signbit(q[q == 0]).any()
    assert not _np(a.get_traces()).any()                        # c = 0: nothing survives a sweep
    _assert_same_handles(a, b, rng)
    a.close(); b.close()


@pytest.mark.parametrize("algo,kind", [("q_learning", tref.ACCUMULATING), ("sarsa", tref.REPLACING)])
def test_lambda_1(algo, kind):
    handle, rng = "s8_max5", "numpy"
    a = _traced(handle, rng, algo, kind, lam=1.0)
    r = Restated(a, algo, kind, lam=1.0)
    for launch in range(2):
        _check_launch(a, r, K, (algo, kind, launch))
    assert (r.agent.Z != 0).any()
    a.close()


# ---- the buffer: round trip, set_learner, set_q, evaluation
def test_traces_round_trip_set_q_leaves_them_and_set_learner_drops_them():
    from mdp_playground_amd import _capi as capi
    handle, algo, kind, rng = "s8", "sarsa", tref.ACCUMULATING, "philox"
    a = _traced(handle, rng, algo, kind)
    r = Restated(a, algo, kind)
    _check_launch(a, r, K, "first")
    z = torch.as_tensor(np.random.default_rng(3).random((N, 8, 8)).astype(np.float32), device=a.device)
    a.set_traces(z)
    assert torch.equal(a.get_traces(), z)
    r.agent.Z = _np(z)
    q = torch.as_tensor(np.random.default_rng(4).normal(size=(N, 8, 8)).astype(np.float32), device=a.device)
    a.set_q(q)                                                  # leaves Z alone
    assert torch.equal(a.get_traces(), z) and torch.equal(a.get_q(), q)
    r.agent.Q = _np(q)
    _check_launch(a, r, K, "from given Q and Z")
    for bad in (z[:-1], z.double(), z.cpu(), _np(z)):
        with pytest.raises(ValueError):
            a.set_traces(bad)
    # evaluation neither reads nor writes Z
    zb, qb = a.get_traces(), a.get_q()
    a.rollout_eval(K)
    a.rollout_eval(K, summary=a.episode_summary())
    assert torch.equal(a.get_traces().view(torch.int32), zb.view(torch.int32)) and torch.equal(a.get_q().view(torch.int32), qb.view(torch.int32))
    assert "trace" not in a.eval_kernel_name(K)
    # clear_learner_traces: the one-step learner again
    a.clear_learner_traces()
    assert a.learner_traces is None and a.learn_kernel_name(K).startswith("k_discrete_learn_rollout<")
    with pytest.raises(capi.MdppError, match="no traces"):
        a.get_traces()
    a.set_learner_traces(LAMBDA, kind)
    assert not _np(a.get_traces()).any()                        # (zeros when traces are set)
    a.rollout_learn(K)
    assert _np(a.get_traces()).any()
    # set_learner drops the traces; the next traces start from zeros
    a.set_learner(algo, alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=SEED)
    assert a.learner_traces is None and a.learn_kernel_name(K).startswith("k_discrete_learn_rollout<")
    with pytest.raises(capi.MdppError, match="no traces"):
        a.set_traces(z)
    a.set_learner_traces(LAMBDA, tref.REPLACING)
    assert a.learner_traces == tref.REPLACING and not _np(a.get_traces()).any()
    a.set_learner(None)
    assert a.learner_traces is None
    with pytest.raises(capi.MdppError, match="no learner"):
        a.set_learner_traces(LAMBDA)
    assert not a.status().any()
    a.close()


def test_rates_and_lambda_between_launches():
    """set_learner_rates (scalars and arrays) and a new lambda serve the handle as it stands; Z is zeroed by set_learner_traces only"""
    handle, algo, kind, rng = "s8_max5", "q_learning", tref.REPLACING, "numpy"
    cfg = cases.HANDLES[handle][0]
    a = _traced(handle, rng, algo, kind)
    r = Restated(a, algo, kind)
    _check_launch(a, r, K, "uniform")
    a.set_learner_rates(alpha=0.5, epsilon=0.5)
    r.agent.al0[:] = np.float32(0.5)
    r.agent.E0[:] = ref.epsilon_threshold(0.5)
    _check_launch(a, r, 9, "new uniform rates")
    assert a.learn_kernel_name(K) == _name(cfg, rng)
    ga = np.linspace(0.0, 1.0, N).astype(np.float32)
    a.set_learner_rates(gamma=ga)
    r.agent.ga[:] = ga
    _check_launch(a, r, 9, "per-env gamma: the PE form with the uniform lambda as an array")
    assert a.learn_kernel_name(K) == _name(cfg, rng, "pe")
    lam = np.linspace(1.0, 0.0, N).astype(np.float32)
    a.set_learner_traces(torch.as_tensor(lam), kind)            # (a torch tensor; Z starts again from zeros)
    r.agent.lam[:] = lam
    r.agent.Z[:] = 0
    _check_launch(a, r, 9, "per-env lambda")
    for bad in (np.full(N - 1, 0.5), np.full(N, 1.5), np.full(N, np.nan), -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            a.set_learner_traces(bad, kind)
    with pytest.raises(ValueError):
        a.set_learner_traces(0.5, "dutch")
    # the library's own checks: MDPP_EINVAL (-1), nothing changed
    from mdp_playground_amd import _capi as capi
    for bad in (np.full(N, np.nan, np.float32), np.full(N, 1.5, np.float32)):
        assert a._lib.mdpp_set_learner_lambda(a._h, capi.nptr(bad), None) == -1
        assert b"lambda" in a._lib.mdpp_last_error(a._h)
    assert a._lib.mdpp_set_learner_traces(a._h, 3, 0.5, None) == -1 and a._lib.mdpp_set_learner_traces(a._h, 1, float("nan"), None) == -1
    assert a.learner_traces == kind
    _check_launch(a, r, 9, "after the refused calls: unchanged")
    a.close()


# ---- refusals, in both orders: each leaves what is in force
def test_double_q_is_refused():
    a = _mk(cases.HANDLES["s8"][0], "numpy", n=64)
    a.set_learner("double_q", alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=SEED)
    name = a.learn_kernel_name(K)
    with pytest.raises(NotImplementedError, match="eligibility traces with double_q: not built"):
        a.set_learner_traces(LAMBDA)
    assert a.learner_traces is None and a.learn_kernel_name(K) == name and "DOUBLE=1" in name
    a.rollout_learn(5)
    # the other order: set_learner("double_q") on a handle with traces starts a new learner, which drops them
    a.set_learner("sarsa", alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=SEED)
    a.set_learner_traces(LAMBDA)
    a.set_learner("double_q", alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=SEED)
    assert a.learner_traces is None and a.learn_kernel_name(K) == name
    assert not a.status().any()
    a.close()


def test_noise_levels_are_refused_in_both_orders():
    cfg = dict(cases.HANDLES["s8"][0], reward_noise=0.5)
    lv = np.linspace(0.0, 2.0, 64)
    a = _mk(cfg, "numpy", n=64)
    a.set_learner("q_learning", alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=SEED)
    a.set_noise_levels(reward_noise=lv)
    with pytest.raises(NotImplementedError, match="eligibility traces with per-env noise levels: not built"):
        a.set_learner_traces(LAMBDA)
    assert a.learner_traces is None and np.array_equal(a.noise_levels()[1], lv) and a.learn_kernel_name(K).endswith(",PE=1,NLEV=1>")
    a.clear_noise_levels()
    a.set_learner_traces(LAMBDA)
    name = a.learn_kernel_name(K)
    assert name.startswith("k_discrete_trace_rollout<")
    with pytest.raises(NotImplementedError, match="eligibility traces with per-env noise levels: not built"):
        a.set_noise_levels(reward_noise=lv)
    assert a.learner_traces == tref.REPLACING and a.learn_kernel_name(K) == name and np.array_equal(a.noise_levels()[1], np.full(64, 0.5))
    a.rollout_learn(5)
    assert not a.status().any()
    a.close()


def test_one_mdp_per_env_is_refused():
    """(the other order does not exist: traces are only ever set on a shared-MDP handle, where per_env_mdp=True is a ValueError)"""
    from mdp_playground_amd import RLToyVectorEnv
    cfg = dict(cases.HANDLES["s8"][0])
    cfg.pop("seed")
    pm = RLToyVectorEnv(seeds=list(range(1, 65)), **cfg)
    pm.set_learner("q_learning", alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=SEED, per_env_mdp=True)
    name = pm.learn_kernel_name(K)
    with pytest.raises(NotImplementedError, match="eligibility traces with one MDP per env: not built"):
        pm.set_learner_traces(LAMBDA)
    assert pm.learner_traces is None and pm.learn_kernel_name(K) == name and ",PM=" in name
    pm.rollout_learn(5)
    pm.close()
    a = _traced("s8", "numpy", "q_learning", tref.REPLACING, n=64)
    with pytest.raises(ValueError):
        a.set_learner("q_learning", alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=SEED, per_env_mdp=True)
    assert a.learner_traces == tref.REPLACING
    a.close()


def test_the_sweep_schedule_is_refused_in_both_orders():
    a = _traced("s8", "numpy", "sarsa", tref.REPLACING, n=64)
    name = a.learn_kernel_name(K)
    with pytest.raises(NotImplementedError, match="eligibility traces with the schedule of mdpp_learner_schedule_sweep: not built"):
        a.set_learner_schedule(epsilon=[0.5, 0.1], sweep=True)
    assert a.learner_schedule() is None and a.learner_traces == tref.REPLACING and a.learn_kernel_name(K) == name
    a.set_learner_schedule(epsilon=[0.5, 0.1])                  # the plain schedule is served
    assert a.learn_kernel_name(K).endswith(",PE=1,SCHED=1>") and a.learn_kernel_name(K).startswith("k_discrete_trace_rollout<")
    a.rollout_learn(5)
    a.close()
    b = _mk(cases.HANDLES["s8"][0], "numpy", n=64)
    b.set_learner("sarsa", alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=SEED)
    b.set_learner_schedule(epsilon=[0.5, 0.1], sweep=True)
    name = b.learn_kernel_name(K)
    with pytest.raises(NotImplementedError, match="eligibility traces with the schedule of mdpp_learner_schedule_sweep: not built"):
        b.set_learner_traces(LAMBDA)
    assert b.learner_traces is None and b.learn_kernel_name(K) == name and b.learner_schedule() is not None
    b.clear_learner_schedule()
    b.set_learner_traces(LAMBDA)
    assert b.learner_traces == tref.REPLACING
    b.rollout_learn(5)
    assert not b.status().any()
    b.close()
