"""Double Q-learning and per-env learner hyper-parameters on the GPU (RLToyVectorEnv.set_learner / set_learner_rates /
rollout_learn; the PE and DOUBLE forms of k_discrete_learn_rollout).

As in tests/test_gpu_learn_rollout.py every launch is held to two yardsticks: the open-loop twin (an identically built handle
fed with the actions the launch returned: outputs, state record, env and space streams, tick) and the numpy restatement
tests/learner_sweep_ref.py fed with the launch's own outputs (actions and get_q(), bit for bit).  N = 320 envs (one full
workgroup and a partial one), K = 37 steps (no multiple of 4), two launches in a row.  What the passes must have exercised
is stated in tests/learner_sweep_cases.py and shown reachable on the CPU by tests/test_learner_sweep_host.py."""
import numpy as np
import pytest
import torch

import learner_sweep_cases as cases
import learner_sweep_ref as ref
from test_gpu_learn_rollout import (REFUSED, _assert_same_handles, _assert_same_outputs, _bits, _mk, _np, _obs_now, _tick)

pytestmark = pytest.mark.gpu

N, K = 320, cases.K
OFF = 1000
SEED, ALPHA, GAMMA, EPS = cases.SEED, cases.ALPHA, cases.GAMMA, cases.EPS
BASE_NAME = "k_discrete_learn_rollout<PHILOX=%d,NOISE=%d,UNIT=%d,QLDS=%d"


class Restated:
    """the restatement, carried from launch to launch beside a handle"""

    def __init__(self, env, algo, q0=None, off=0, alpha=ALPHA, gamma=GAMMA, eps=EPS, autoreset=ref.SAME_STEP):
        m = env.mdps[0]
        self.algo, self.off, self.alpha, self.gamma, self.eps, self.autoreset = algo, off, alpha, gamma, eps, autoreset
        self.P = np.asarray(m.P)
        shape = (env.num_envs, 2, m.S, m.A) if algo == "double_q" else (env.num_envs, m.S, m.A)
        self.Q = np.zeros(shape, np.float32) if q0 is None else q0.copy()
        self.pending = np.zeros(env.num_envs, bool)
        self.info = {}

    def launch(self, tick0, obs_before, out):
        obs, rew, term, trunc = (_np(x) for x in out[:4])
        k, n = obs.shape
        w_e, w_a, w_u = (ref.tick_words(SEED, self.off, tick0, k + 1, n, st) for st in (ref.EXPLORE_STREAM, ref.ACTION_STREAM, ref.UPDATE_STREAM))
        act, self.Q, self.pending, info = ref.run(self.algo, self.alpha, self.gamma, self.eps, self.Q, obs_before, obs, rew, term, trunc,
                                                  self.P, self.autoreset, w_e, w_a, w_u, self.pending)
        ref.merge_info(self.info, info)
        return act


def _check_launch(a, r, k, what):
    """one learning launch of handle a against the restatement r; returns its outputs"""
    before, tick0 = _obs_now(a), _tick(a)
    out = a.rollout_learn(k)
    assert out[4].dtype == torch.int32 and tuple(out[4].shape) == (k, a.num_envs)
    want = r.launch(tick0, before, out)
    got = _np(out[4])
    assert np.array_equal(got, want), (what, "actions", np.argwhere(got != want)[:5])
    q = _np(a.get_q())
    assert q.dtype == np.float32 and q.shape == r.Q.shape
    assert np.array_equal(_bits(q), _bits(r.Q)), (what, "Q", np.argwhere(_bits(q) != _bits(r.Q))[:5])
    return out


def _twin_run(a, b, r, what, rng):
    for launch in range(cases.LAUNCHES):
        assert _tick(a) == launch * K
        out = _check_launch(a, r, K, what + (launch,))
        _assert_same_outputs(out[:4], b.rollout(out[4]), what + (launch,))
    _assert_same_handles(a, b, rng)


def _name(cfg, rng, qlds, tail):
    return BASE_NAME % (rng == "philox", "transition_noise" in cfg, "reward_dist" not in cfg, qlds) + tail + ">"


@pytest.mark.parametrize("rng", ["numpy", "philox"])
@pytest.mark.parametrize("case", list(cases.DOUBLE_CASES))
def test_double_q_twin_and_restatement(case, rng):
    cfg, kw = cases.DOUBLE_CASES[case]
    a, b = _mk(cfg, rng, env_id_offset=OFF, **kw), _mk(cfg, rng, env_id_offset=OFF, **kw)
    rand = case == "cfg2_random_q"
    q0 = cases.random_q(5, N, cfg["state_space_size"], cfg["action_space_size"], True) if rand else None
    a.set_learner("double_q", alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=SEED, q=None if q0 is None else torch.as_tensor(q0, device=a.device))
    name = a.learn_kernel_name(K)
    assert name == _name(cfg, rng, case not in cases.GLOBAL_FORM, ",DOUBLE=1"), name
    q = a.get_q()
    assert tuple(q.shape) == (N, 2, cfg["state_space_size"], cfg["action_space_size"])
    assert np.array_equal(_bits(_np(q)), _bits(q0 if rand else np.zeros_like(_np(q))))
    r = Restated(a, "double_q", q0=q0, off=OFF, autoreset=kw.get("autoreset", ref.SAME_STEP))
    _twin_run(a, b, r, (case, rng), rng)
    print(case, rng, {k: v for k, v in r.info.items() if not isinstance(v, np.ndarray)})
    cases.double_honest(r.info, r.Q, rand)
    a.close(); b.close()


def test_double_q_global_form_by_option_equals_the_lds_form():
    one, two = _mk(cases.CFG2, "numpy"), _mk(cases.CFG2, "numpy")
    two.set_kernel_options("NO_LEARN_LDS")
    for e in (one, two):
        e.set_learner("double_q", alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=SEED)
    assert one.learn_kernel_name(K).endswith("QLDS=1,DOUBLE=1>") and two.learn_kernel_name(K).endswith("QLDS=0,DOUBLE=1>")
    for launch in range(2):
        for g, w in zip(two.rollout_learn(K), one.rollout_learn(K)):
            assert torch.equal(g, w), launch
    assert torch.equal(one.get_q().view(torch.int32), two.get_q().view(torch.int32))
    one.close(); two.close()


def _pe(n=N, lo=0):
    return cases.pe_arrays(n, lo)


@pytest.mark.parametrize("rng", ["numpy", "philox"])
@pytest.mark.parametrize("algo", ref.ALGOS)
@pytest.mark.parametrize("case", list(cases.PE_CASES))
def test_per_env_parameters_twin_and_restatement(case, algo, rng):
    cfg, kw = cases.PE_CASES[case]
    a, b = _mk(cfg, rng, env_id_offset=OFF, **kw), _mk(cfg, rng, env_id_offset=OFF, **kw)
    al, ga, ep = _pe()
    # numpy float32, a float64 torch tensor on the host, a tensor on the device: all are converted to float32
    a.set_learner(algo, alpha=al, gamma=torch.as_tensor(ga.astype(np.float64)), epsilon=torch.as_tensor(ep, device=a.device), seed=SEED)
    name = a.learn_kernel_name(K)
    assert name == _name(cfg, rng, case not in cases.GLOBAL_FORM, ",PE=1" + (",DOUBLE=1" if algo == "double_q" else "")), name
    r = Restated(a, algo, off=OFF, alpha=al, gamma=ga, eps=ep)
    _twin_run(a, b, r, (case, algo, rng), rng)
    cases.pe_honest(r.info, ep)
    a.close(); b.close()


@pytest.mark.parametrize("algo", ref.ALGOS)
def test_equal_arrays_reproduce_the_uniform_handle_and_mixed_arrays_its_matching_envs(algo):
    uni, same, mixed = (_mk(cases.CFG2, "numpy") for _ in range(3))
    al, ga, ep = _pe()
    ua, ug, ue = np.float32(0.3), np.float32(0.9), np.float32(0.25)          # a triple of the cycle
    match = (al == ua) & (ga == ug) & (ep == ue)
    assert match.sum() >= 5 and not match.all()
    uni.set_learner(algo, alpha=0.3, gamma=0.9, epsilon=0.25, seed=SEED)
    same.set_learner(algo, alpha=np.full(N, 0.3), gamma=np.full(N, 0.9), epsilon=np.full(N, 0.25), seed=SEED)
    mixed.set_learner(algo, alpha=al, gamma=ga, epsilon=ep, seed=SEED)
    assert ",PE=1" not in uni.learn_kernel_name(K) and ",PE=1" in same.learn_kernel_name(K) and ",PE=1" in mixed.learn_kernel_name(K)
    for launch in range(2):
        want, got, mix = uni.rollout_learn(K), same.rollout_learn(K), mixed.rollout_learn(K)
        for w, g, m in zip(want, got, mix):
            assert torch.equal(g, w), (algo, launch)
            assert torch.equal(m[:, torch.as_tensor(match)], w[:, torch.as_tensor(match)]), (algo, launch)
        assert not torch.equal(mix[4], want[4])
    qu, qs, qm = (_bits(_np(e.get_q())) for e in (uni, same, mixed))
    assert np.array_equal(qs, qu) and np.array_equal(qm[match], qu[match])
    # one array only: the other two travel as arrays of their uniform values
    one = _mk(cases.CFG2, "numpy")
    one.set_learner(algo, alpha=0.3, gamma=0.9, epsilon=torch.full((N,), 0.25), seed=SEED)
    assert ",PE=1" in one.learn_kernel_name(K)
    uni2 = _mk(cases.CFG2, "numpy")
    uni2.set_learner(algo, alpha=0.3, gamma=0.9, epsilon=0.25, seed=SEED)
    for g, w in zip(one.rollout_learn(K), uni2.rollout_learn(K)):
        assert torch.equal(g, w), algo
    assert torch.equal(one.get_q().view(torch.int32), uni2.get_q().view(torch.int32))
    for e in (uni, same, mixed, one, uni2):
        assert not e.status().any()
        e.close()


@pytest.mark.parametrize("algo", ["q_learning", "double_q"])
def test_set_learner_rates_with_arrays_between_launches_then_back_to_scalars(algo):
    a = _mk(cases.CFG2, "philox")
    a.set_learner(algo, alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=SEED)
    tail = ",DOUBLE=1>" if algo == "double_q" else ">"
    r = Restated(a, algo)
    _check_launch(a, r, K, "uniform")
    assert ",PE=1" not in a.learn_kernel_name(K)
    al, ga, ep = _pe()
    a.set_learner_rates(alpha=al, epsilon=ep)                  # gamma stays uniform
    r.alpha, r.eps, r.info = al, ep, {}
    _check_launch(a, r, K, "alpha and epsilon per env")
    assert a.learn_kernel_name(K).endswith(",PE=1" + tail)
    cases.pe_honest(r.info, ep)
    a.set_learner_rates(gamma=ga)
    r.gamma = ga
    _check_launch(a, r, 9, "gamma per env too")
    a.set_learner_rates(alpha=0.5)                             # alpha uniform again, epsilon and gamma stay per env
    r.alpha = 0.5
    _check_launch(a, r, 9, "alpha back to a scalar")
    assert a.learn_kernel_name(K).endswith(",PE=1" + tail)
    a.set_learner_rates(epsilon=1.0, gamma=0.5)
    r.eps, r.gamma, r.info = 1.0, 0.5, {}
    _check_launch(a, r, 9, "all three scalars")
    assert ",PE=1" not in a.learn_kernel_name(K) and a.learn_kernel_name(K).endswith(tail)
    assert r.info["explored"] == 9 * N
    a.set_learner_rates(epsilon=np.zeros(N))
    r.eps, r.info = np.zeros(N), {}
    _check_launch(a, r, 6, "epsilon array of zeros")
    assert r.info["explored"] == 0
    for bad in (dict(alpha=np.full(N - 1, 0.5)), dict(alpha=np.full((N, 1), 0.5)), dict(epsilon=np.full(N, 1.5)), dict(gamma=np.full(N, -0.1)),
                dict(alpha=np.zeros(N)), dict(gamma=np.full(N, np.nan)), dict(alpha=0.0), dict(gamma=1.5)):
        with pytest.raises(ValueError):
            a.set_learner_rates(**bad)
    _check_launch(a, r, 5, "after the refused calls: unchanged")
    assert not a.status().any()
    a.close()


@pytest.mark.parametrize("rng", ["numpy", "philox"])
@pytest.mark.parametrize("algo", ["sarsa", "double_q"])
def test_two_shards_with_their_array_halves_equal_the_whole(algo, rng):
    al, ga, ep = _pe()
    whole = _mk(cases.CFG2, rng)
    whole.set_learner(algo, alpha=al, gamma=ga, epsilon=ep, seed=SEED)
    outs = [whole.rollout_learn(K) for _ in range(2)]
    q = whole.get_q()
    for lo in (0, N // 2):
        sh = _mk(cases.CFG2, rng, n=N // 2, env_id_offset=lo)
        sl = slice(lo, lo + N // 2)
        sh.set_learner(algo, alpha=al[sl], gamma=ga[sl], epsilon=ep[sl], seed=SEED)
        for launch in range(2):
            for g, w in zip(sh.rollout_learn(K), outs[launch]):
                assert torch.equal(g, w[:, sl]), (algo, rng, lo, launch)
        assert torch.equal(sh.get_q().view(torch.int32), q[sl].view(torch.int32))
        sh.close()
    whole.close()


@pytest.mark.parametrize("rng", ["numpy", "philox"])
@pytest.mark.parametrize("pe", [False, True])
def test_a_double_q_call_sent_out_in_pieces_equals_one_launch(pe, rng):
    one, many = _mk(cases.CFG2, rng), _mk(cases.CFG2, rng)
    many.set_kernel_options("LEARN_SHORT_PIECES")
    al, ga, ep = _pe() if pe else (ALPHA, GAMMA, EPS)
    for e in (one, many):
        e.set_learner("double_q", alpha=al, gamma=ga, epsilon=ep, seed=SEED)
    r = Restated(many, "double_q", alpha=al, gamma=ga, eps=ep)
    for launch in range(2):
        want = one.rollout_learn(K)
        got = _check_launch(many, r, K, (pe, rng, launch))
        for g, w in zip(got, want):
            assert torch.equal(g, w), (pe, rng, launch)
    assert torch.equal(one.get_q().view(torch.int32), many.get_q().view(torch.int32))
    _assert_same_handles(one, many, rng)
    one.close(); many.close()


def test_sarsa_per_env_call_sent_out_in_pieces_equals_one_launch():
    one, many = _mk(cases.CFG2, "numpy"), _mk(cases.CFG2, "numpy")
    many.set_kernel_options("LEARN_SHORT_PIECES")
    al, ga, ep = _pe()
    for e in (one, many):
        e.set_learner("sarsa", alpha=al, gamma=ga, epsilon=ep, seed=SEED)
    for launch in range(2):
        for g, w in zip(many.rollout_learn(K), one.rollout_learn(K)):
            assert torch.equal(g, w), launch
    assert torch.equal(one.get_q().view(torch.int32), many.get_q().view(torch.int32))
    one.close(); many.close()


@pytest.mark.parametrize("case", list(REFUSED))
def test_unsupported_handles_are_refused_for_double_q_with_the_reason(case):
    from mdp_playground_amd import RLToyVectorEnv
    cfg, kw, reason = REFUSED[case]
    cfg = dict(cfg)
    if "seeds" in kw:
        cfg.pop("seed")
    env = RLToyVectorEnv(**({} if "seeds" in kw else {"num_envs": 64}), **kw, **cfg)
    with pytest.raises(NotImplementedError, match=reason):
        env.set_learner("double_q", alpha=ALPHA, gamma=GAMMA, epsilon=EPS)
    with pytest.raises(NotImplementedError, match=reason):
        env.set_learner("double_q", alpha=np.full(env.num_envs, 0.5), gamma=GAMMA, epsilon=EPS)
    assert env.learn_kernel_name(4) == ""
    env.close()


def test_bad_arrays_and_bad_double_tables_raise_value_error_and_the_tables_round_trip():
    from mdp_playground_amd import _capi as capi
    a = _mk(cases.CFG2, "numpy")
    ok = dict(alpha=ALPHA, gamma=GAMMA, epsilon=EPS)
    for bad in (dict(alpha=np.full(N + 1, 0.5)), dict(gamma=np.full((N, 1), 0.5)), dict(epsilon=np.full(N, 2.0)), dict(alpha=np.zeros(N)),
                dict(epsilon=torch.full((N,), float("nan"))), dict(gamma=torch.full((2, N), 0.5))):
        for algo in ("q_learning", "double_q"):
            with pytest.raises(ValueError):
                a.set_learner(algo, **dict(ok, **bad))
    with pytest.raises(capi.MdppError, match="no learner"):     # (nothing above set one)
        a.rollout_learn(4)
    with pytest.raises(ValueError):
        a.set_learner("double_q_learning", **ok)
    a.set_learner("double_q", seed=SEED, **ok)
    q = cases.random_q(6, N, 8, 8, True)
    a.set_q(torch.as_tensor(q, device=a.device))
    assert np.array_equal(_bits(_np(a.get_q())), _bits(q))
    r = Restated(a, "double_q", q0=q)
    _check_launch(a, r, 5, "after set_q")
    dev = a.device
    for bad in (torch.zeros((N, 8, 8), device=dev), torch.zeros((N, 2, 8, 7), device=dev), torch.zeros((N, 1, 8, 8), device=dev),
                torch.zeros((N, 2, 8, 8), dtype=torch.float64, device=dev), torch.zeros((N, 2, 8, 8)), q):
        with pytest.raises(ValueError):
            a.set_q(bad)
        with pytest.raises(ValueError):
            a.set_learner("double_q", q=bad, **ok)
    # back to one table on the same handle, and to two again
    a.set_learner("q_learning", seed=SEED, **ok)
    assert tuple(a.get_q().shape) == (N, 8, 8) and not a.get_q().any()
    with pytest.raises(ValueError):
        a.set_q(torch.zeros((N, 2, 8, 8), device=dev))
    a.set_learner("double_q", seed=SEED, **ok)
    assert tuple(a.get_q().shape) == (N, 2, 8, 8) and not a.get_q().any()
    assert not a.status().any()
    a.close()


def test_the_dispatcher_routes_every_state_of_a_handle_to_the_form_of_that_name():
    """A launch that lands on the wrong form is silent where the forms agree (uniform parameters give the same numbers with and
    without PE), so the routes are pinned by name: nothing is launched."""
    cfg = dict(cases._S8, reward_noise=0.5)         # (a reward_noise key: reward levels are admissible)
    al = np.linspace(0.1, 0.9, 64)

    def names(algo, per_env=False, levels=False):
        e = _mk(cfg, "numpy", n=64)
        e.set_learner(algo, alpha=al if per_env else ALPHA, gamma=GAMMA, epsilon=EPS, seed=SEED)
        if levels:
            e.set_noise_levels(reward_noise=np.linspace(0.0, 2.0, 64))
        got = e.learn_kernel_name(K), e.eval_kernel_name(K)
        e.close()
        return got

    assert names("q_learning") == ("k_discrete_learn_rollout<PHILOX=0,NOISE=1,UNIT=1,QLDS=1>",
                                   "k_discrete_eval_rollout<PHILOX=0,NOISE=1,UNIT=1,QLDS=1,DOUBLE=0>")
    assert names("q_learning", per_env=True)[0] == "k_discrete_learn_rollout<PHILOX=0,NOISE=1,UNIT=1,QLDS=1,PE=1>"
    assert names("double_q") == ("k_discrete_learn_rollout<PHILOX=0,NOISE=1,UNIT=1,QLDS=1,DOUBLE=1>",
                                 "k_discrete_eval_rollout<PHILOX=0,NOISE=1,UNIT=1,QLDS=1,DOUBLE=1>")
    assert names("double_q", per_env=True)[0] == "k_discrete_learn_rollout<PHILOX=0,NOISE=1,UNIT=1,QLDS=1,PE=1,DOUBLE=1>"
    assert names("q_learning", levels=True) == ("k_discrete_learn_rollout<PHILOX=0,NOISE=1,UNIT=1,QLDS=1,PE=1,NLEV=1>",
                                                "k_discrete_eval_rollout<PHILOX=0,NOISE=1,UNIT=1,QLDS=1,DOUBLE=0,NLEV=1>")
    assert names("double_q", levels=True) == ("k_discrete_learn_rollout<PHILOX=0,NOISE=1,UNIT=1,QLDS=1,PE=1,DOUBLE=1,NLEV=1>",
                                              "k_discrete_eval_rollout<PHILOX=0,NOISE=1,UNIT=1,QLDS=1,DOUBLE=1,NLEV=1>")
