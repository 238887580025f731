"""Per-env noise levels on ONE MDP PER ENV on the GPU (RLToyVectorEnv(seeds=[...]).set_learner(..., per_env_mdp=True) then
set_noise_levels(..., per_env_mdp=True): a noise x seed sweep in one launch; the NLEV forms of the closed-loop kernels with
PM = 1 / 2).

The yardsticks:
  twin rule    for each of the seven (transition_noise, reward_noise) pairs, the mixed handle's envs at that pair equal, bit
               for bit, the same-index envs of a UNIFORM per-env-MDP handle created at the pair with the same seeds and learner
               -- outputs, Q-tables, state record, env and space streams, status and tick -- after each of two launches;
  restatement  tests/learner_sweep_ref.py fed the launch's own outputs with P[i] per env: actions and get_q() bit for bit;
  CPU loop     (Philox streams) noise_seed_cases.closed_loop: one oracle env per seed at its own level, driven by the
               restatement -- actions, outputs and Q bit for bit.
noise_seed_cases.honest and FLOORS are re-asserted on the device's result; tests/test_noise_seed_host.py shows on the CPU that
they can be met.  Without the feature every case fails at set_noise_levels(..., per_env_mdp=True)."""
import numpy as np
import pytest
import torch

import eval_summary_ref as eref
import graph_replay_util as gr
import learner_sweep_ref as ref
import noise_seed_cases as cases
import per_env_mdp_cpu as pm

pytestmark = pytest.mark.gpu

N, K, OFF, SEED, SEEDS = cases.N, cases.K, cases.OFF, cases.SEED, cases.SEEDS
ALPHA, GAMMA, EPS = cases.ALPHA, cases.GAMMA, cases.EPS
ONLY = "per-env noise levels: learner and evaluation launches only; clear_noise_levels\\(\\) first"
ALL = np.arange(N)


def _mk(cfg, rng, seeds=SEEDS, off=OFF, options=(), **kw):
    from mdp_playground_amd import RLToyVectorEnv
    extra = dict(rng="philox", philox_seed=cases.PHILOX_SEED) if rng == "philox" else {}
    env = RLToyVectorEnv(seeds=list(seeds), env_id_offset=off, **extra, **kw, **cfg)
    if options:
        env.set_kernel_options(*options)
    return env


def _learner(env, algo, q=None, **over):
    kw = dict(alpha=ALPHA, gamma=GAMMA, epsilon=EPS)
    kw.update(over)
    env.set_learner(algo, seed=SEED, per_env_mdp=True, q=None if q is None else torch.as_tensor(q, device=env.device), **kw)


def _mixed(cfg, rng, algo, kw, seeds=SEEDS, lo=0, off=OFF, q=None, options=(), **over):
    """a handle of envs lo ... lo + n - 1 of the level cycle on `seeds`, with the per-env-MDP learner and the levels set"""
    env = _mk(cases.mixed_cfg(cfg), rng, seeds, off + lo, options, **kw)
    _learner(env, algo, q, **over)
    tn, rn = cases.level_arrays(len(seeds), lo)
    env.set_noise_levels(transition_noise=tn, reward_noise=rn, per_env_mdp=True)
    return env, tn, rn


def _twins(cfg, rng, algo, kw, tn, rn, seeds=SEEDS, off=OFF, q=None, pairs=None, **over):
    """(p, sigma) -> (the uniform per-env-MDP handle created at that pair with the same seeds and learner, the envs of the
    mixed handle at it)"""
    out = {}
    for p, s in pairs or cases.pairs_present(tn, rn):
        env = _mk(cases.twin_cfg(cfg, p, s), rng, seeds, off, **kw)
        _learner(env, algo, q, **over)
        assert "NLEV" not in env.learn_kernel_name(K)
        out[(p, s)] = (env, np.flatnonzero((tn == p) & (rn == s)))
    return out


def _np(x):
    return x.cpu().numpy().copy()


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def _obs_now(env):
    return _np(env._obs) if env._obs_src is None else _np(env._obs_src)


def _same_at(got, want, at, what):
    """tuples of [K, n] tensors: equal, bit for bit, at the envs `at`"""
    at = torch.as_tensor(at, device=got[0].device)
    for j, (g, w) in enumerate(zip(got, want)):
        g, w = g[:, at], w[:, at]
        if g.dtype == torch.float32:
            g, w = g.view(torch.int32), w.view(torch.int32)
        if g.dtype == torch.float64:
            g, w = g.view(torch.int64), w.view(torch.int64)
        assert torch.equal(g, w), (what, j)


def _same_handles_at(a, b, at, rng, what):
    """tables, state record, streams, status and tick of handle a's envs `at` equal those of handle b"""
    from mdp_playground_amd import _capi as capi
    qa, qb = _bits(_np(a.get_q())), _bits(_np(b.get_q()))
    assert np.array_equal(qa[at], qb[at]), (what, "Q")
    sa, sb = a.get_augmented_state(), b.get_augmented_state()
    assert sa.keys() == sb.keys()
    for k in sa:
        assert np.array_equal(sa[k][at], sb[k][at]), (what, k)
    if rng == "numpy":
        for st in (capi.STREAM_ENV, capi.STREAM_SPACE):
            assert np.array_equal(a.get_rng_streams(st)[at], b.get_rng_streams(st)[at]), (what, "stream", st)
    assert gr.tick(a) == gr.tick(b)
    assert not a.status().any() and not b.status().any()


def _run_twin_rule(a, twins, rng, what, launches=cases.LAUNCHES, k=K, step=None):
    step = step or (lambda env: env.rollout_learn(k))
    outs = []
    for launch in range(launches):
        out = step(a)
        outs.append(out)
        for pair, (b, at) in twins.items():
            _same_at(out, step(b), at, what + (pair, launch))
            _same_handles_at(a, b, at, rng, what + (pair, launch))
    return outs


def _close(a, twins=None):
    a.close()
    for b, _ in (twins or {}).values():
        b.close()


class Restated:
    """the restatement on one MDP per env, carried from launch to launch beside a handle"""

    def __init__(self, cfg, algo, seeds=SEEDS, off=OFF, alpha=ALPHA, gamma=GAMMA, eps=EPS, autoreset=ref.SAME_STEP):
        mdps = pm.build_mdps(cfg, seeds)
        m, n = mdps[0], len(mdps)
        self.algo, self.alpha, self.gamma, self.eps, self.autoreset, self.off = algo, alpha, gamma, eps, autoreset, off
        self.P = pm.PerEnvP(mdps)
        self.Q = np.zeros((n, 2, m.S, m.A) if algo == "double_q" else (n, m.S, m.A), np.float32)
        self.pending = np.zeros(n, bool)
        self.info = {}

    def launch(self, tick0, obs_before, out):
        obs, rew, term, trunc = (_np(x) for x in out[:4])
        k, n = obs.shape
        w_e, w_a, w_u = (ref.tick_words(SEED, self.off, tick0, k + 1, n, st) for st in (ref.EXPLORE_STREAM, ref.ACTION_STREAM, ref.UPDATE_STREAM))
        act, self.Q, self.pending, info = ref.run(self.algo, self.alpha, self.gamma, self.eps, self.Q, obs_before, obs, rew, term, trunc,
                                                  self.P, self.autoreset, w_e, w_a, w_u, self.pending)
        ref.merge_info(self.info, info)
        return act


def _restated_step(a, r, k, what):
    """step(env) for _run_twin_rule: the mixed handle's launch is also held to the restatement (actions and Q)"""
    def step(env):
        if env is not a:
            return env.rollout_learn(k)
        before, tick0 = _obs_now(env), gr.tick(env)
        out = env.rollout_learn(k)
        want = r.launch(tick0, before, out)
        assert np.array_equal(_np(out[4]), want), (what, "actions against the restatement", np.argwhere(_np(out[4]) != want)[:5])
        assert np.array_equal(_bits(_np(env.get_q())), _bits(r.Q)), (what, "Q against the restatement")
        step.before.append(before)
        return out
    step.before = []
    return step


def _assert_cpu_loop(cfg, kw, algo, a, tn, rn, outs, what, k=K, **learner):
    _, Q, traj = cases.closed_loop(cfg, kw, algo, tn, rn, learner.get("alpha", ALPHA), learner.get("gamma", GAMMA), learner.get("epsilon", EPS), K=k)
    obs, rew, term, trunc, act = (np.concatenate([_np(o[j]) for o in outs]) for j in range(5))
    for name, g, w in (("actions", act, traj["actions"]), ("obs", obs, traj["obs"]), ("terminated", term.astype(bool), traj["terminated"]),
                       ("truncated", trunc.astype(bool), traj["truncated"]), ("reward", _bits(rew), _bits(traj["reward"]))):
        assert np.array_equal(g, w), (what, "CPU loop", name, np.argwhere(g != w)[:5])
    assert np.array_equal(_bits(_np(a.get_q())), _bits(Q)), (what, "CPU loop", "Q")


def _assert_names(a, cfg, algo, rng, *options):
    qlds, pmv, _, _ = cases.placement(cfg, algo, rng, *options)
    assert a.learn_kernel_name(K) == cases.kernel_name("learn", cfg, algo, rng, qlds, pmv), (a.learn_kernel_name(K), qlds, pmv)
    assert a.eval_kernel_name(K) == cases.kernel_name("eval", cfg, algo, rng, qlds, pmv), (a.eval_kernel_name(K), qlds, pmv)


# ---- the twin rule
@pytest.mark.parametrize("case,algo,rng", cases.TWIN_PARAMS)
def test_twin_rule_restatement_and_cpu_loop(case, algo, rng):
    cfg, kw, _, k = cases.CASES[case]
    a, tn, rn = _mixed(cfg, rng, algo, kw)
    _assert_names(a, cfg, algo, rng)
    got_tn, got_rn = a.noise_levels()
    assert got_tn.dtype == np.float64 and np.array_equal(got_tn, tn) and np.array_equal(got_rn, rn)
    twins = _twins(cfg, rng, algo, kw, tn, rn)
    assert len(twins) == 7
    autoreset = kw.get("autoreset", ref.SAME_STEP)
    r = Restated(cfg, algo, autoreset=autoreset)
    what = (case, algo, rng)
    step = _restated_step(a, r, k, what)
    outs = _run_twin_rule(a, twins, rng, what, k=k, step=step)
    if rng == "philox":
        _assert_cpu_loop(cfg, kw, algo, a, tn, rn, outs, what, k=k)
    # what keeps the pass honest, on the device's outputs
    obs, rew, term, trunc, act = (np.concatenate([_np(o[j]) for o in outs]) for j in range(5))
    term, trunc = term.astype(bool), trunc.astype(bool)
    state = np.concatenate([np.concatenate([b[None], _np(o[0])[:-1]]) for b, o in zip(step.before, outs)])
    ended = term | trunc
    reset_call = np.zeros_like(ended)
    if autoreset == ref.NEXT_STEP:
        pend = np.zeros(N, bool)
        for t in range(ended.shape[0]):                  # a reset call follows every ending step and ends nothing itself
            reset_call[t] = pend
            pend = ended[t] & ~reset_call[t]
    live = ~reset_call
    true_next = live & ~(ended & (autoreset == ref.SAME_STEP))     # (after a same-step reset obs is the next episode's first state)
    P, values = cases.tables(cfg)
    nxt = np.where(true_next, obs, P[ALL[None, :], state, act])    # (where obs is not the true next state: counted as not noisy)
    cases.honest(tn, rn, state, act, nxt, rew, term, r.info["explored_env"], P, values, live)
    counts = cases.check_floors(case, _np(a.get_q()), term, what)
    print(case, algo, rng, "non-zero Q: all, lanes 0-255, lanes 256-319; envs that terminated:", counts)
    _close(a, twins)


# ---- every reachable placement by option on the tabular shape
OPTION_SETS = [(), ("NO_PM_NLEV_LDS",), ("NO_PM_LDS",), ("NO_PM_LDS", "NO_PM_NLEV_LDS"), ("NO_LEARN_LDS",), ("NO_LEARN_LDS", "NO_PM_NLEV_LDS"),
               ("NO_LEARN_LDS", "NO_PM_LDS"), ("NO_LEARN_LDS", "NO_PM_LDS", "NO_PM_NLEV_LDS")]


@pytest.mark.parametrize("algo,rng", [("q_learning", "numpy"), ("double_q", "numpy"), ("sarsa", "philox")])
def test_every_placement_by_option_computes_what_the_default_placement_computes(algo, rng):
    cfg = cases.TABULAR
    handles = []
    for options in OPTION_SETS:
        e, _, _ = _mixed(cfg, rng, algo, {}, options=options)
        _assert_names(e, cfg, algo, rng, *options)
        handles.append(e)
    placements = {cases.placement(cfg, algo, rng, *o)[:3] for o in OPTION_SETS}
    assert len(placements) == (8 if (algo, rng) == ("q_learning", "numpy") else 4 if rng == "philox" else 6), placements
    for launch in range(2):
        want = handles[0].rollout_learn(K)
        for e, options in zip(handles[1:], OPTION_SETS[1:]):
            _same_at(e.rollout_learn(K), want, ALL, (algo, rng, options, launch))
            _same_handles_at(e, handles[0], ALL, rng, (algo, rng, options, launch))
    want = handles[0].rollout_eval(K)                    # evaluation takes the same placements
    for e, options in zip(handles[1:], OPTION_SETS[1:]):
        _same_at(e.rollout_eval(K), want, ALL, (algo, rng, options, "eval"))
    for e in handles:
        e.close()


def test_the_worked_placements_by_name():
    for cfg, algo, want in ((cases.TABULAR, "q_learning", "QLDS=1,PE=1,NLEV=1,PM=2>"), (cases.TABULAR, "double_q", "QLDS=1,PE=1,DOUBLE=1,NLEV=1,PM=1>"),
                            (cases.S20, "q_learning", "QLDS=0,PE=1,NLEV=1,PM=1>")):
        a, _, _ = _mixed(cfg, "numpy", algo, {}, seeds=SEEDS[:14])
        assert a.learn_kernel_name(K).endswith(want), (algo, a.learn_kernel_name(K))
        assert a.eval_kernel_name(K).endswith(",NLEV=1,PM=%s>" % want[-2]) and ("QLDS=%s," % want[5]) in a.eval_kernel_name(K)
        s = a.episode_summary()
        a.rollout_learn(3, summary=s)
        a.close()


# ---- sizes with a launch of one step; pieces; where the tables come from
@pytest.mark.parametrize("rng", ["numpy", "philox"])
@pytest.mark.parametrize("n", [1, 63, 257])
def test_sizes_with_a_launch_of_one_step(n, rng):
    lo = 3 if n == 1 else 0                      # (one env: the env of levels (0.10, 10))
    seeds = SEEDS[lo:lo + n]
    a, tn, rn = _mixed(cases.TABULAR, rng, "q_learning", {}, seeds=seeds, lo=lo)
    # (one env: its one MDP is a shared MDP, the opt-in changes nothing and the shared-MDP kernel serves it)
    assert (",NLEV=1,PM=" in a.learn_kernel_name(1)) == (n > 1) and ",NLEV=1" in a.learn_kernel_name(1), a.learn_kernel_name(1)
    twins = _twins(cases.TABULAR, rng, "q_learning", {}, tn, rn, seeds=seeds, off=OFF + lo)
    assert len(twins) == min(n, 7)
    for k in (1, K):
        _run_twin_rule(a, twins, rng, (n, rng, k), launches=1, k=k)
    _close(a, twins)


@pytest.mark.parametrize("rng", ["numpy", "philox"])
def test_a_sarsa_call_sent_out_in_pieces_equals_one_launch(rng):
    one, tn, rn = _mixed(cases.TABULAR, rng, "sarsa", {})
    many, _, _ = _mixed(cases.TABULAR, rng, "sarsa", {}, options=("LEARN_SHORT_PIECES",))
    r = Restated(cases.TABULAR, "sarsa")
    step = _restated_step(many, r, K, (rng, "pieces"))
    for launch in range(2):
        _same_at(step(many), one.rollout_learn(K), ALL, (rng, launch))
        _same_handles_at(many, one, ALL, rng, (rng, launch))
    assert r.info["carried_differs"] > 0
    one.close(); many.close()


@pytest.mark.parametrize("path", ["device", "mdps"])
def test_device_built_and_caller_given_tables(path):
    cfg = cases.CFG2
    kw = dict(mdps=pm.build_mdps(cases.mixed_cfg(cfg))) if path == "mdps" else {}
    a, tn, rn = _mixed(cfg, "philox", "q_learning", kw)
    assert a.tables_built_on == ("device" if path == "device" else "host")
    outs = [a.rollout_learn(K) for _ in range(2)]
    _assert_cpu_loop(cfg, {}, "q_learning", a, tn, rn, outs, (path,))
    a.close()


# ---- levels with per-env alpha / epsilon / gamma
@pytest.mark.parametrize("algo,rng", [("q_learning", "numpy"), ("double_q", "philox")])
def test_levels_with_per_env_learner_parameters(algo, rng):
    rs = np.random.default_rng(12)
    over = dict(alpha=rs.uniform(0.05, 1.0, N).astype(np.float32), gamma=rs.uniform(0.0, 1.0, N).astype(np.float32),
                epsilon=rs.uniform(0.0, 1.0, N).astype(np.float32))
    a, tn, rn = _mixed(cases.TABULAR, rng, algo, {}, **over)
    twins = _twins(cases.TABULAR, rng, algo, {}, tn, rn, **over)
    r = Restated(cases.TABULAR, algo, alpha=over["alpha"], gamma=over["gamma"], eps=over["epsilon"])
    outs = _run_twin_rule(a, twins, rng, (algo, rng), step=_restated_step(a, r, K, (algo, rng)))
    if rng == "philox":
        _assert_cpu_loop(cases.TABULAR, {}, algo, a, tn, rn, outs, (algo, rng), **over)
    _close(a, twins)


# ---- all-equal arrays are the uniform per-env-MDP handle
@pytest.mark.parametrize("rng", ["numpy", "philox"])
@pytest.mark.parametrize("algo", ["sarsa", "double_q"])
def test_all_equal_arrays_reproduce_the_uniform_per_env_mdp_handle_on_every_env(algo, rng):
    uni = _mk(cases.twin_cfg(cases.CFG2, 0.1, 1.0), rng)
    same = _mk(cases.mixed_cfg(cases.CFG2), rng)
    scal = _mk(cases.mixed_cfg(cases.CFG2), rng)
    for e in (uni, same, scal):
        _learner(e, algo)
    same.set_noise_levels(np.full(N, 0.1), torch.full((N,), 1.0, device=same.device), per_env_mdp=True)
    scal.set_noise_levels(transition_noise=0.1, reward_noise=1, per_env_mdp=True)       # scalars are broadcast
    assert "NLEV" not in uni.learn_kernel_name(K) and ",NLEV=1,PM=" in same.learn_kernel_name(K) and ",NLEV=1,PM=" in scal.learn_kernel_name(K)
    for launch in range(2):
        want = uni.rollout_learn(K)
        for e in (same, scal):
            _same_at(e.rollout_learn(K), want, ALL, (algo, rng, launch))
            _same_handles_at(e, uni, ALL, rng, (algo, rng, launch))
    for e in (uni, same, scal):
        e.close()


# ---- greedy evaluation and both summary forms
@pytest.mark.parametrize("case,algo,rng", [("tabular", "q_learning", "numpy"), ("cfg2", "double_q", "philox"), ("s29", "double_q", "numpy"),
                                           ("cfg2_next_step", "sarsa", "philox")])
def test_evaluation_and_summaries_equal_the_twins_and_the_full_output_launch(case, algo, rng):
    cfg, kw, _, _ = cases.CASES[case]
    S, A = cfg["state_space_size"], cfg["action_space_size"]
    q0 = np.random.default_rng(9).normal(size=(N, 2, S, A) if algo == "double_q" else (N, S, A)).astype(np.float32)
    a, tn, rn = _mixed(cfg, rng, algo, kw, q=q0)
    _assert_names(a, cfg, algo, rng)
    twins = _twins(cfg, rng, algo, kw, tn, rn, q=q0)
    what = (case, algo, rng)
    words = [a._learn_rates[:], a._learn_algo]
    ev = _run_twin_rule(a, twins, rng, what + ("eval",), launches=1, step=lambda e: e.rollout_eval(K))[0]
    assert np.array_equal(_bits(_np(a.get_q())), _bits(q0))                             # evaluation writes no table
    assert [a._learn_rates[:], a._learn_algo] == words and np.array_equal(a.noise_levels()[0], tn)
    # the summary forms against the full-output launch of a second mixed handle brought to the same point
    full, _, _ = _mixed(cfg, rng, algo, kw, q=q0)
    full.rollout_eval(K)
    summ = a.episode_summary()
    autoreset = kw.get("autoreset", ref.SAME_STEP)
    st = eref.new_state5(N)
    _, pending = eref.reset_calls(_np(ev[2]).astype(bool), _np(ev[3]).astype(bool), autoreset)
    for form in ("learn", "eval", "learn"):
        assert getattr(a, "rollout_" + form)(K, summary=summ) is summ
        out = getattr(full, "rollout_" + form)(K)
        _same_handles_at(a, full, ALL, rng, what + (form, "summary against full output"))
        rc, pending = eref.reset_calls(_np(out[2]).astype(bool), _np(out[3]).astype(bool), autoreset, pending)
        st = eref.summary(_np(out[1]), _np(out[2]).astype(bool), _np(out[3]).astype(bool), rc, st)
        for (name, dt), t in zip(eref.FIELDS, summ.tensors()):
            g, w = _np(t), st[name]
            assert g.dtype == dt, (name, g.dtype)
            if dt == np.float64:
                g, w = g.view(np.int64), w.view(np.int64)
            assert np.array_equal(g, w), (what, form, name, np.argwhere(g != w)[:5])
    assert int(summ.tensors()[2].sum()) > 0                                             # episodes ended
    # ... and the summary launches under levels equal the twins' summary launches
    sums = {}

    def summary_step(form):
        def step(env):
            s = sums.setdefault((id(env), form), env.episode_summary())
            getattr(env, "rollout_" + form)(K, summary=s)
            return tuple(t[None] for t in s.tensors())                                  # ([1, N] each: compared like outputs)
        return step
    for b, _ in twins.values():                                                         # (the twins: to where a is)
        for form in ("learn", "eval", "learn"):
            getattr(b, "rollout_" + form)(K)
    for form in ("learn", "eval"):
        _run_twin_rule(a, twins, rng, what + (form, "summary"), launches=1, step=summary_step(form))
    full.close()
    _close(a, twins)


# ---- levels changed between launches, then cleared
@pytest.mark.parametrize("algo", ["q_learning", "double_q"])
def test_levels_set_changed_and_cleared_between_launches(algo):
    rng = "philox"                 # (the handle that continues is rebuilt from state record, tick and tables: Philox streams keep no other state)
    created = cases.twin_cfg(cases.CFG2, 0.1, 1.0)
    a = _mk(created, rng)
    _learner(a, algo)
    before = a.learn_kernel_name(K), a.eval_kernel_name(K), a.rollout_kernel_name(K)
    a.rollout_learn(K)
    tn, rn = cases.level_arrays(N)
    a.set_noise_levels(tn, rn, per_env_mdp=True)
    assert ",NLEV=1,PM=" in a.learn_kernel_name(K) and ",NLEV=1,PM=" in a.eval_kernel_name(K)
    a.rollout_learn(K)
    a.set_noise_levels(transition_noise=tn[::-1].copy(), per_env_mdp=True)      # other levels mid-training; the reward levels stay
    assert np.array_equal(a.noise_levels()[0], tn[::-1]) and np.array_equal(a.noise_levels()[1], rn)
    out_rev = a.rollout_learn(K)
    c = _mk(created, rng)                                                        # ... which is what both arrays given at once do
    _learner(c, algo)
    c.rollout_learn(K)
    c.set_noise_levels(tn, rn, per_env_mdp=True)
    c.rollout_learn(K)
    c.clear_noise_levels()
    c.set_noise_levels(tn[::-1].copy(), rn, per_env_mdp=True)
    _same_at(c.rollout_learn(K), out_rev, ALL, (algo, "changed"))
    a.clear_noise_levels()
    assert (a.learn_kernel_name(K), a.eval_kernel_name(K), a.rollout_kernel_name(K)) == before
    assert np.array_equal(a.noise_levels()[0], np.full(N, 0.1)) and np.array_equal(a.noise_levels()[1], np.full(N, 1.0))
    with pytest.raises(NotImplementedError, match="per-env noise levels on one MDP per env: not built"):
        a.set_noise_levels(reward_noise=rn)                                      # (clearing dropped the opt-in too)
    # a handle that never had levels, continuing from the same state
    b = _mk(created, rng)
    b.set_augmented_state(a.get_augmented_state())
    assert b._lib.mdpp_tick(b._h, gr.tick(a), None) == 0
    _learner(b, algo, q=_np(a.get_q()))
    assert (b.learn_kernel_name(K), b.eval_kernel_name(K), b.rollout_kernel_name(K)) == before
    for launch in range(2):
        _same_at(a.rollout_learn(K), b.rollout_learn(K), ALL, (algo, "cleared", launch))
        _same_handles_at(a, b, ALL, rng, (algo, "cleared", launch))
    act = torch.zeros((3, N), dtype=torch.int32, device=a.device)
    _same_at(a.rollout(act), b.rollout(act), ALL, (algo, "open loop after clear"))
    # set_learner(None) drops levels given with the opt-in, and the opt-in
    c.set_learner(None)
    assert c.learn_kernel_name(K) == ""
    c.rollout(act)
    _learner(c, algo)
    assert "NLEV" not in c.learn_kernel_name(K)
    for e in (a, b, c):
        e.close()


# ---- shards
@pytest.mark.parametrize("rng", ["numpy", "philox"])
@pytest.mark.parametrize("algo", ["sarsa", "double_q"])
def test_two_shards_with_their_seed_and_array_halves_equal_the_whole(algo, rng):
    whole, _, _ = _mixed(cases.CFG2, rng, algo, {}, off=0)
    outs = [whole.rollout_learn(K) for _ in range(2)]
    q = whole.get_q()
    for lo in (0, N // 2):
        sh, tn, _ = _mixed(cases.CFG2, rng, algo, {}, seeds=SEEDS[lo:lo + N // 2], lo=lo, off=0)
        assert len(np.unique(tn)) == 5
        sl = slice(lo, lo + N // 2)
        for launch in range(2):
            for g, w in zip(sh.rollout_learn(K), outs[launch]):
                assert torch.equal(g, w[:, sl]), (algo, rng, lo, launch)
        assert torch.equal(sh.get_q().view(torch.int32), q[sl].view(torch.int32))
        sh.close()
    whole.close()


# ---- a captured launch
@pytest.mark.parametrize("algo,rng", [("sarsa", "philox"), ("double_q", "numpy")])
def test_graph_replay(algo, rng):
    """rollout_learn captured in the library's capture mode, replayed three times with the step counter moved by 5 in between,
    against an eager twin"""
    k = 9
    g, _, _ = _mixed(cases.TABULAR, rng, algo, {})
    e, _, _ = _mixed(cases.TABULAR, rng, algo, {})
    out = g.alloc_rollout_learn(k)
    want = e.rollout_learn(k)
    got = g.rollout_learn(k, out=out)                    # the eager launch of the same form before the capture
    assert all(torch.equal(x, y) for x, y in zip(got, want))
    cap = gr.capture(g, lambda: g.rollout_learn(k, out=out), k)
    for replay in range(3):
        for h in (g, e):                                 # the counter moves by 5: a greedy launch serves a handle with levels
            h.rollout_eval(5)
        cap.replay()
        want = e.rollout_learn(k)
        for name, x, y in zip(("obs", "reward", "terminated", "truncated", "actions"), out, want):
            assert torch.equal(x.view(torch.uint8) if x.dtype == torch.bool else x, y.view(torch.uint8) if y.dtype == torch.bool else y), (algo, replay, name)
        assert torch.equal(g.get_q().view(torch.int32), e.get_q().view(torch.int32)), (algo, replay)
    g._obs_src = out[0][k - 1]
    _same_handles_at(g, e, ALL, rng, (algo, "after the replays"))
    del cap
    g.close(); e.close()


# ---- refusals
def test_refusals():
    from mdp_playground_amd import RLToyVectorEnv, _capi as capi
    cfg = cases.mixed_cfg(cases.TABULAR)
    a = _mk(cfg, "numpy", seeds=SEEDS[:64])
    rn = np.full(64, 0.25)
    with pytest.raises(NotImplementedError, match="one shared MDP"):            # no per_env_mdp learner: the learner's refusal
        a.set_noise_levels(reward_noise=rn, per_env_mdp=True)
    _learner(a, "q_learning")
    name = a.learn_kernel_name(K)
    with pytest.raises(NotImplementedError, match="per-env noise levels on one MDP per env: not built") as e:
        a.set_noise_levels(reward_noise=rn)                                      # without the opt-in: today's message
    assert str(e.value) == "mdpp_set_noise_levels: per-env noise levels on one MDP per env: not built"
    assert a.learn_kernel_name(K) == name
    # the C rule: flag off, mdpp_set_noise_levels returns what it returned; on, it proceeds
    assert a._lib.mdpp_set_noise_levels(a._h, None, capi.nptr(rn), None) == capi.EUNSUPPORTED
    a.set_noise_levels(reward_noise=rn, per_env_mdp=True)
    assert ",NLEV=1,PM=" in a.learn_kernel_name(K)
    act = torch.zeros((4, 64), dtype=torch.int32, device=a.device)
    for call in (lambda: a.step(act[0]), lambda: a.rollout(act), lambda: a.step_graph(act)):
        with pytest.raises(capi.MdppError, match=ONLY):
            call()
    with pytest.raises(NotImplementedError, match="policy rollouts"):           # (set_policy keeps refusing, the noise key first)
        a.set_policy(np.zeros(8, np.int64), seed=3)
    assert a.policy_kernel_name(4) == ""
    with pytest.raises(ValueError, match="transition_noise"):                   # bad arrays, as on a shared MDP
        a.set_noise_levels(transition_noise=np.arange(64) % 17 / 17.0, per_env_mdp=True)
    a.rollout_learn(4)
    assert not a.status().any()
    a.close()
    shared = RLToyVectorEnv(num_envs=64, seed=0, **cfg)
    shared.set_learner("q_learning", alpha=ALPHA, gamma=GAMMA, epsilon=EPS)
    with pytest.raises(ValueError, match="per_env_mdp"):
        shared.set_noise_levels(reward_noise=rn, per_env_mdp=True)
    assert shared._lib.mdpp_noise_levels_per_env_mdp(shared._h, 1) == 0         # the C call on a shared MDP: accepted, nothing changes
    shared.set_noise_levels(reward_noise=rn)
    assert shared.learn_kernel_name(K).endswith(",NLEV=1>")
    shared.close()
