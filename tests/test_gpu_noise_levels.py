"""Per-env noise levels on the GPU (RLToyVectorEnv.set_noise_levels; the NLEV form of the closed-loop step around the PE learner
and the greedy evaluation).

The yardstick is the twin rule: env i of a handle with mixed levels equals, bit for bit, env i of a UNIFORM handle created at
env i's (transition_noise, reward_noise) pair and run with the same learner -- outputs, tables, state record, env and space
streams, tick -- after each of two launches.  The uniform handles are held to the oracle and to the restatement by
tests/test_gpu_learn_rollout.py and tests/test_gpu_learn_sweep.py.  N = 320 envs (one full workgroup and a quarter), K = 37
steps, levels cycling by env index (tests/noise_levels_cases.py): every wave holds all 25 pairs, lanes that skip the
space-stream draw sit beside lanes that make it.  What the passes must have exercised is stated in noise_levels_cases.honest
and shown reachable on the CPU by tests/test_noise_levels_host.py."""
import numpy as np
import pytest
import torch

import learner_sweep_cases as sweep
import learner_sweep_ref as ref
import noise_levels_cases as cases
from test_gpu_learn_rollout import REFUSED, _bits, _mk, _np, _obs_now, _tick
from test_gpu_learn_sweep import Restated

pytestmark = pytest.mark.gpu

N, K = 320, cases.K
OFF = 1000
SEED, ALPHA, GAMMA, EPS = cases.SEED, cases.ALPHA, cases.GAMMA, cases.EPS
ONLY = "per-env noise levels: learner and evaluation launches only; clear_noise_levels\\(\\) first"


def _learner(env, algo, q=None, **over):
    kw = dict(alpha=ALPHA, gamma=GAMMA, epsilon=EPS)
    kw.update(over)
    env.set_learner(algo, seed=SEED, q=None if q is None else torch.as_tensor(q, device=env.device), **kw)


def _mixed(cfg, rng, algo, kw, n=N, lo=0, off=OFF, q=None, **over):
    """a handle of envs lo ... lo + n - 1 of the level cycles, with the learner set"""
    env = _mk(cases.mixed_cfg(cfg), rng, n=n, env_id_offset=off + lo, **kw)
    _learner(env, algo, q, **over)
    tn, rn = cases.level_arrays(n, lo)
    env.set_noise_levels(transition_noise=tn, reward_noise=rn)
    return env, tn, rn


def _twins(cfg, rng, algo, kw, tn, rn, n=N, off=OFF, q=None, pairs=None, **over):
    """(p, sigma) -> (the uniform handle created at that pair with the same learner, the envs of the mixed handle at it)"""
    out = {}
    for p, s in pairs or cases.pairs_present(tn, rn):
        env = _mk(cases.twin_cfg(cfg, p, s), rng, n=n, env_id_offset=off, **kw)
        _learner(env, algo, q, **over)
        assert "NLEV" not in env.learn_kernel_name(K)
        out[(p, s)] = (env, np.flatnonzero((tn == p) & (rn == s)))
    return out


def _same_at(got, want, at, what):
    """tuples of [K, N] tensors: equal, bit for bit, at the envs `at`"""
    at = torch.as_tensor(at, device=got[0].device)
    for j, (g, w) in enumerate(zip(got, want)):
        g, w = g[:, at], w[:, at]
        if g.dtype == torch.float32:
            g, w = g.view(torch.int32), w.view(torch.int32)
        assert torch.equal(g, w), (what, j)


def _same_handles_at(a, b, at, rng, what):
    """tables, state record, streams and tick of handle a's envs `at` equal those of handle b"""
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
    assert _tick(a) == _tick(b)
    assert not a.status().any() and not b.status().any()


def _run_twin_rule(a, twins, rng, what, launches=cases.LAUNCHES, k=K, step=None):
    """`launches` launches of the mixed handle and of every twin (step(env): the launch; default rollout_learn(k)), compared
    after each; returns the mixed handle's outputs"""
    step = step or (lambda env: env.rollout_learn(k))
    outs = []
    for launch in range(launches):
        out = step(a)
        outs.append(out)
        for pair, (b, at) in twins.items():
            _same_at(out, step(b), at, what + (pair, launch))
            _same_handles_at(a, b, at, rng, what + (pair, launch))
    return outs


def _close(a, twins):
    a.close()
    for b, _ in twins.values():
        b.close()


def _name(kind, cfg, rng, qlds, algo):
    dbl = algo == "double_q"
    if kind == "learn":
        return "k_discrete_learn_rollout<PHILOX=%d,NOISE=1,UNIT=%d,QLDS=%d,PE=1%s,NLEV=1>" % (rng == "philox", "reward_dist" not in cfg, qlds, ",DOUBLE=1" if dbl else "")
    return "k_discrete_eval_rollout<PHILOX=%d,NOISE=1,UNIT=%d,QLDS=%d,DOUBLE=%d,NLEV=1>" % (rng == "philox", "reward_dist" not in cfg, qlds, dbl)


# ---- the twin rule
@pytest.mark.parametrize("case,algo,rng", cases.TWIN_PARAMS)
def test_twin_rule(case, algo, rng):
    cfg, kw, _ = cases.CASES[case]
    a, tn, rn = _mixed(cfg, rng, algo, kw)
    assert a.learn_kernel_name(K) == _name("learn", cfg, rng, case not in cases.GLOBAL_Q, algo), a.learn_kernel_name(K)
    got_tn, got_rn = a.noise_levels()
    assert got_tn.dtype == np.float64 and np.array_equal(got_tn, tn) and np.array_equal(got_rn, rn)
    twins = _twins(cfg, rng, algo, kw, tn, rn)
    assert len(twins) == 25
    autoreset = kw.get("autoreset", ref.SAME_STEP)
    r = Restated(a, algo, off=OFF, autoreset=autoreset)

    def step(env):
        if env is not a:
            return env.rollout_learn(K)
        before, tick0 = _obs_now(env), _tick(env)
        out = env.rollout_learn(K)
        want = r.launch(tick0, before, out)              # (the restatement too: it also counts the exploring selections)
        assert np.array_equal(_np(out[4]), want), (case, algo, rng, "actions against the restatement")
        step.before.append(before)
        return out
    step.before = []
    outs = _run_twin_rule(a, twins, rng, (case, algo, rng), step=step)
    assert np.array_equal(_bits(_np(a.get_q())), _bits(r.Q))
    # the honesty counts of the host file, on the GPU's outputs
    obs, rew, term, trunc, act = (np.concatenate([_np(o[j]) for o in outs]) for j in range(5))
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
    P = np.asarray(a.mdps[0].P)
    nxt = np.where(true_next, obs, P[state, act])                   # (where obs is not the true next state: counted as not noisy)
    cases.honest(tn, rn, state, act, nxt, rew, term, r.info["explored_env"], P, live)
    _close(a, twins)


# ---- per-env levels together with per-env alpha / epsilon / gamma
@pytest.mark.parametrize("algo,rng", [("q_learning", "numpy"), ("double_q", "philox"), ("sarsa", "philox")])
def test_levels_with_per_env_learner_parameters(algo, rng):
    al, ga, ep = sweep.pe_arrays(N)
    over = dict(alpha=al, gamma=ga, epsilon=ep)
    a, tn, rn = _mixed(cases.TABULAR, rng, algo, {}, **over)
    assert a.learn_kernel_name(K).endswith(",NLEV=1>")
    twins = _twins(cases.TABULAR, rng, algo, {}, tn, rn, **over)
    _run_twin_rule(a, twins, rng, (algo, rng))
    # one parameter per env only, set after the levels: the other two travel as arrays of their uniform values
    b, _, _ = _mixed(cases.TABULAR, rng, algo, {})
    b.set_learner_rates(epsilon=ep)
    tw = _twins(cases.TABULAR, rng, algo, {}, tn, rn, pairs=cases.pairs_present(tn, rn)[::6], epsilon=ep)
    assert len(tw) == 5
    _run_twin_rule(b, tw, rng, (algo, rng, "epsilon"))
    _close(a, twins)
    _close(b, tw)


# ---- all-equal arrays are the uniform handle
@pytest.mark.parametrize("rng", ["numpy", "philox"])
@pytest.mark.parametrize("algo", ["sarsa", "double_q"])
def test_all_equal_arrays_reproduce_the_uniform_handle_on_every_env(algo, rng):
    uni = _mk(cases.twin_cfg(sweep.CFG2, 0.1, 1.0), rng)
    same = _mk(cases.mixed_cfg(sweep.CFG2), rng)
    scal = _mk(cases.mixed_cfg(sweep.CFG2), rng)
    for e in (uni, same, scal):
        _learner(e, algo)
    same.set_noise_levels(np.full(N, 0.1), torch.full((N,), 1.0, device=same.device))
    scal.set_noise_levels(transition_noise=0.1, reward_noise=1)                       # scalars are broadcast
    assert "NLEV" not in uni.learn_kernel_name(K) and ",NLEV=1>" in same.learn_kernel_name(K) and ",NLEV=1>" in scal.learn_kernel_name(K)
    for launch in range(2):
        want = uni.rollout_learn(K)
        for e in (same, scal):
            _same_at(e.rollout_learn(K), want, np.arange(N), (algo, rng, launch))
            _same_handles_at(e, uni, np.arange(N), rng, (algo, rng, launch))
    # one key only: the other stays at its creation value
    one, ref_one = _mk(cases.twin_cfg(sweep.CFG2, 0.1, 1.0), rng), _mk(cases.twin_cfg(sweep.CFG2, 0.1, 5.0), rng)
    for e in (one, ref_one):
        _learner(e, algo)
    one.set_noise_levels(reward_noise=np.full(N, 5.0))
    assert np.array_equal(one.noise_levels()[0], np.full(N, 0.1)) and np.array_equal(one.noise_levels()[1], np.full(N, 5.0))
    _same_at(one.rollout_learn(K), ref_one.rollout_learn(K), np.arange(N), (algo, rng, "reward key only"))
    _same_handles_at(one, ref_one, np.arange(N), rng, (algo, rng, "reward key only"))
    for e in (uni, same, scal, one, ref_one):
        e.close()


# ---- greedy evaluation and both summary forms
@pytest.mark.parametrize("case,algo,rng", [("tabular", "q_learning", "numpy"), ("cfg2", "double_q", "philox"), ("s29", "double_q", "numpy"),
                                           ("cfg2_next_step", "sarsa", "philox")])
def test_evaluation_and_summaries_under_levels_equal_the_twins(case, algo, rng):
    cfg, kw, _ = cases.CASES[case]
    q0 = sweep.random_q(9, N, cfg["state_space_size"], cfg["action_space_size"], algo == "double_q")
    a, tn, rn = _mixed(cfg, rng, algo, kw, q=q0)
    assert a.eval_kernel_name(K) == _name("eval", cfg, rng, case not in cases.GLOBAL_Q, algo), a.eval_kernel_name(K)
    assert a.learn_kernel_name(K) == _name("learn", cfg, rng, case not in cases.GLOBAL_Q, algo)
    twins = _twins(cfg, rng, algo, kw, tn, rn, q=q0)
    what = (case, algo, rng)
    _run_twin_rule(a, twins, rng, what + ("eval",), launches=1, step=lambda e: e.rollout_eval(K))
    assert np.array_equal(_bits(_np(a.get_q())), _bits(q0))                             # evaluation writes no table
    sums = {}

    def summary_step(form):
        def step(env):
            s = sums.setdefault((id(env), form), env.episode_summary())
            getattr(env, "rollout_" + form)(K, summary=s)
            return tuple(t[None] for t in s.tensors())                                  # ([1, N] each: compared like outputs)
        return step
    for form in ("learn", "eval", "learn"):
        outs = _run_twin_rule(a, twins, rng, what + (form, "summary"), launches=1, step=summary_step(form))
        assert int(outs[0][2].sum()) > 0                                                # episodes ended
    assert not np.array_equal(_bits(_np(a.get_q())), _bits(q0))
    _close(a, twins)


# ---- levels changed between launches, then cleared
@pytest.mark.parametrize("algo", ["q_learning", "double_q"])
def test_levels_set_changed_and_cleared_between_launches(algo):
    rng = "philox"                 # (the handle that continues is rebuilt from state record, tick and tables: Philox streams keep no other state)
    created = cases.twin_cfg(sweep.CFG2, 0.1, 1.0)
    a = _mk(created, rng, env_id_offset=OFF)
    _learner(a, algo)
    before = a.learn_kernel_name(K), a.eval_kernel_name(K), a.rollout_kernel_name(K)
    a.rollout_learn(K)
    tn, rn = cases.level_arrays(N)
    a.set_noise_levels(tn, rn)
    assert ",NLEV=1>" in a.learn_kernel_name(K) and ",NLEV=1>" in a.eval_kernel_name(K)
    a.rollout_learn(K)
    a.set_noise_levels(transition_noise=tn[::-1].copy())           # other levels mid-training; the reward levels stay
    assert np.array_equal(a.noise_levels()[0], tn[::-1]) and np.array_equal(a.noise_levels()[1], rn)
    out_rev = a.rollout_learn(K)
    # ... which is what a handle given both arrays at once does from the same state
    c = _mk(created, rng, env_id_offset=OFF)
    _learner(c, algo)
    c.rollout_learn(K)
    c.set_noise_levels(tn, rn)
    c.rollout_learn(K)
    c.clear_noise_levels()
    c.set_noise_levels(tn[::-1].copy(), rn)
    _same_at(c.rollout_learn(K), out_rev, np.arange(N), (algo, "changed"))
    a.clear_noise_levels()
    assert (a.learn_kernel_name(K), a.eval_kernel_name(K), a.rollout_kernel_name(K)) == before
    assert np.array_equal(a.noise_levels()[0], np.full(N, 0.1)) and np.array_equal(a.noise_levels()[1], np.full(N, 1.0))
    # a handle that never had levels, continuing from the same state
    b = _mk(created, rng, env_id_offset=OFF)
    b.set_augmented_state(a.get_augmented_state())
    assert b._lib.mdpp_tick(b._h, _tick(a), None) == 0
    _learner(b, algo, q=_np(a.get_q()))
    assert (b.learn_kernel_name(K), b.eval_kernel_name(K), b.rollout_kernel_name(K)) == before
    for launch in range(2):
        _same_at(a.rollout_learn(K), b.rollout_learn(K), np.arange(N), (algo, "cleared", launch))
        _same_handles_at(a, b, np.arange(N), rng, (algo, "cleared", launch))
    act = torch.zeros((3, N), dtype=torch.int32, device=a.device)
    _same_at(a.rollout(act), b.rollout(act), np.arange(N), (algo, "open loop after clear"))
    for e in (a, b, c):
        e.close()


# ---- shards, pieces, small handles
@pytest.mark.parametrize("rng", ["numpy", "philox"])
@pytest.mark.parametrize("algo", ["sarsa", "double_q"])
def test_two_shards_with_their_array_halves_equal_the_whole(algo, rng):
    whole, _, _ = _mixed(sweep.CFG2, rng, algo, {}, off=0)
    outs = [whole.rollout_learn(K) for _ in range(2)]
    q = whole.get_q()
    for lo in (0, N // 2):
        sh, tn, _ = _mixed(sweep.CFG2, rng, algo, {}, n=N // 2, lo=lo, off=0)
        assert len(np.unique(tn)) == 5
        sl = slice(lo, lo + N // 2)
        for launch in range(2):
            for g, w in zip(sh.rollout_learn(K), outs[launch]):
                assert torch.equal(g, w[:, sl]), (algo, rng, lo, launch)
        assert torch.equal(sh.get_q().view(torch.int32), q[sl].view(torch.int32))
        sh.close()
    whole.close()


@pytest.mark.parametrize("rng", ["numpy", "philox"])
@pytest.mark.parametrize("algo", ["sarsa", "double_q"])
def test_a_call_sent_out_in_pieces_equals_one_launch(algo, rng):
    one, _, _ = _mixed(sweep.CFG2, rng, algo, {})
    many, _, _ = _mixed(sweep.CFG2, rng, algo, {})
    many.set_kernel_options("LEARN_SHORT_PIECES")
    for launch in range(2):
        _same_at(many.rollout_learn(K), one.rollout_learn(K), np.arange(N), (algo, rng, launch))
        _same_handles_at(many, one, np.arange(N), rng, (algo, rng, launch))
    one.close(); many.close()


def test_cdfs_forced_out_of_lds_equal_the_staged_form():
    one, _, _ = _mixed(cases.TABULAR, "numpy", "q_learning", {})
    two, _, _ = _mixed(cases.TABULAR, "numpy", "q_learning", {})
    two.set_kernel_options("NO_NLEV_LDS")
    three, _, _ = _mixed(cases.TABULAR, "numpy", "q_learning", {})
    three.set_kernel_options("NO_NLEV_LDS", "NO_LEARN_LDS")
    assert "QLDS=1" in two.learn_kernel_name(K) and "QLDS=0" in three.learn_kernel_name(K)
    for launch in range(2):
        want = one.rollout_learn(K)
        for e in (two, three):
            _same_at(e.rollout_learn(K), want, np.arange(N), launch)
            _same_handles_at(e, one, np.arange(N), "numpy", launch)
    for e in (one, two, three):
        e.close()


@pytest.mark.parametrize("rng", ["numpy", "philox"])
@pytest.mark.parametrize("n", [1, 63])
def test_small_handles(n, rng):
    lo = 3 if n == 1 else 0                  # (N = 1: the env of levels (0.10, 0.0))
    a, tn, rn = _mixed(cases.TABULAR, rng, "q_learning", {}, n=n, lo=lo)
    twins = _twins(cases.TABULAR, rng, "q_learning", {}, tn, rn, n=n, off=OFF + lo)
    assert len(twins) == (1 if n == 1 else 25)
    _run_twin_rule(a, twins, rng, (n, rng))
    _close(a, twins)


# ---- refusals and names
def test_step_and_rollout_are_refused_while_levels_are_set_with_the_reason():
    from mdp_playground_amd import _capi as capi
    a, tn, rn = _mixed(cases.TABULAR, "numpy", "q_learning", {})
    act = torch.zeros((4, N), dtype=torch.int32, device=a.device)
    state, tick = a.get_augmented_state(), _tick(a)
    with pytest.raises(capi.MdppError, match=ONLY):
        a.step(act[0])
    with pytest.raises(capi.MdppError, match=ONLY):
        a.rollout(act)
    with pytest.raises(capi.MdppError, match=ONLY):
        a.step_graph(act)
    with pytest.raises(NotImplementedError, match="transition_noise"):
        a.set_policy(np.zeros(8, np.int64))              # (set_policy keeps refusing noise keys as it does)
    assert _tick(a) == tick and all(np.array_equal(state[k], v) for k, v in a.get_augmented_state().items())
    a.reset()                                            # reset() is unaffected
    a.rollout_learn(4)
    # levels are configuration, not state: the state getters and setters neither carry nor disturb them
    st = a.get_augmented_state()
    assert not any("noise" in k for k in st)
    a.set_augmented_state(st)
    assert np.array_equal(a.noise_levels()[0], tn) and np.array_equal(a.noise_levels()[1], rn) and ",NLEV=1>" in a.learn_kernel_name(K)
    a.clear_noise_levels()
    a.step(act[0]); a.rollout(act)
    assert not a.status().any()
    a.close()


def test_handles_without_the_key_and_bad_arrays_are_refused():
    from mdp_playground_amd import _capi as capi
    tn, rn = cases.level_arrays(N)
    for cfg, key, arg in ((cases.TABULAR, "transition_noise", dict(transition_noise=tn)), (cases.TABULAR, "reward_noise", dict(reward_noise=rn)),
                          (dict(cases.TABULAR, transition_noise=0.0, reward_noise=0.0), "transition_noise", dict(transition_noise=tn)),
                          (dict(cases.TABULAR, transition_noise=0.1), "reward_noise", dict(transition_noise=tn, reward_noise=rn))):
        e = _mk(cfg, "numpy")
        _learner(e, "q_learning")
        name = e.learn_kernel_name(K)
        with pytest.raises(ValueError, match=key):
            e.set_noise_levels(**arg)
        assert e.learn_kernel_name(K) == name
        # ... and by the library itself: MDPP_ESTATE with the reason
        arr = np.ascontiguousarray(arg[key])
        rc = e._lib.mdpp_set_noise_levels(e._h, capi.nptr(arr) if key == "transition_noise" else None, capi.nptr(arr) if key == "reward_noise" else None, None)
        assert rc == -4 and key in e._lib.mdpp_last_error(e._h).decode()
        e.close()
    # a key present at 0 serves reward levels
    e = _mk(dict(cases.TABULAR, reward_noise=0.0), "numpy")
    _learner(e, "q_learning")
    e.set_noise_levels(reward_noise=rn)
    assert ",NLEV=1>" in e.learn_kernel_name(K)
    e.rollout_learn(4)
    e.close()
    a = _mk(cases.mixed_cfg(cases.TABULAR), "numpy")
    _learner(a, "q_learning")
    name = a.learn_kernel_name(K)
    assert "NLEV" not in name
    for bad in (dict(transition_noise=tn[:-1]), dict(reward_noise=np.stack([rn, rn])), dict(transition_noise=np.full(N, np.nan)),
                dict(transition_noise=np.full(N, 1.5)), dict(reward_noise=np.full(N, -1.0)), dict(reward_noise=torch.full((N,), float("inf"))),
                dict(transition_noise=np.arange(N) % 17 / 17.0), dict(transition_noise=-0.1), dict(reward_noise=float("nan"))):
        with pytest.raises(ValueError, match=next(iter(bad))):
            a.set_noise_levels(**bad)
    a.set_noise_levels()                                 # (None, None: nothing changes)
    assert a.learn_kernel_name(K) == name
    # bad arrays through the C entry point
    def c_call(t, r):
        rc = a._lib.mdpp_set_noise_levels(a._h, capi.nptr(t), capi.nptr(r), None)
        return rc, a._lib.mdpp_last_error(a._h).decode()
    for t, r, text in ((np.full(N, 1.5), None, "transition_noise in \\[0, 1\\]"), (np.full(N, np.nan), None, "transition_noise in \\[0, 1\\]"),
                       (None, np.full(N, -1.0), "reward_noise finite"), (None, np.full(N, np.inf), "reward_noise finite"),
                       (np.arange(N) % 17 / 17.0, None, "17 distinct values")):
        rc, msg = c_call(t, r)
        assert rc == -1, (rc, msg)
        with pytest.raises(capi.MdppError, match=text):
            capi.check(a._lib, a._h, rc, "mdpp_set_noise_levels")
        assert a.learn_kernel_name(K) == name            # nothing changed
    assert np.array_equal(a.noise_levels()[0], np.full(N, cases.CREATED["transition_noise"]))
    assert np.array_equal(a.noise_levels()[1], np.full(N, cases.CREATED["reward_noise"]))
    a.close()


@pytest.mark.parametrize("case", ["seeds", "irrelevant_features", "continuous", "S300"])
def test_handles_set_learner_refuses_are_refused_with_the_reason(case):
    from mdp_playground_amd import RLToyVectorEnv
    cfg, kw, reason = REFUSED[case]
    cfg = dict(cfg, reward_noise=1.0)
    if case != "continuous":
        cfg["transition_noise"] = 0.1
    if "seeds" in kw:
        cfg.pop("seed")
    env = RLToyVectorEnv(**({} if "seeds" in kw else {"num_envs": 64}), **kw, **cfg)
    with pytest.raises(NotImplementedError, match=reason):
        env.set_noise_levels(reward_noise=np.full(env.num_envs, 2.0))
    env.close()


def test_kernel_names_with_and_without_levels():
    a = _mk(cases.mixed_cfg(cases.TABULAR), "numpy")
    _learner(a, "double_q")
    plain = a.learn_kernel_name(K), a.eval_kernel_name(K)
    assert plain == ("k_discrete_learn_rollout<PHILOX=0,NOISE=1,UNIT=1,QLDS=1,DOUBLE=1>", "k_discrete_eval_rollout<PHILOX=0,NOISE=1,UNIT=1,QLDS=1,DOUBLE=1>")
    a.set_noise_levels(*cases.level_arrays(N))
    assert a.learn_kernel_name(K) == "k_discrete_learn_rollout<PHILOX=0,NOISE=1,UNIT=1,QLDS=1,PE=1,DOUBLE=1,NLEV=1>"
    assert a.eval_kernel_name(K) == "k_discrete_eval_rollout<PHILOX=0,NOISE=1,UNIT=1,QLDS=1,DOUBLE=1,NLEV=1>"
    a.clear_noise_levels()
    assert (a.learn_kernel_name(K), a.eval_kernel_name(K)) == plain
    a.close()
