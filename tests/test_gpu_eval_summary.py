"""Greedy evaluation of the in-kernel learners' tables and the in-kernel episode summaries on the GPU
(RLToyVectorEnv.rollout_eval, and summary= on rollout_learn / rollout_eval; k_discrete_eval_rollout, k_discrete_eval_summary,
k_discrete_learn_summary).

Evaluation is held to the yardsticks of tests/test_gpu_learn_rollout.py: the open-loop twin (an identically built handle fed
with the actions the launch returned: outputs, state record, env and space streams, tick) and the numpy restatement
tests/eval_summary_ref.py fed with the launch's own outputs (actions, bit for bit).  On top: the tables are bit for bit what
they were, and the learner's Philox streams are untouched -- the handle that evaluated and the twin that ran rollout(actions)
carry the same learner and tables and then make identical rollout_learn launches.
A summary launch is held to a twin that makes the full-output call with the same learner: the five arrays equal the
restatement of the rule applied to the twin's outputs (float64 compared as int64), tables, state, streams and tick the twin's.
N = 320 envs (one full workgroup and a partial one), K = 37 steps, two launches in a row.  What the passes must have exercised
is stated in tests/eval_summary_cases.py and shown reachable on the CPU by tests/test_eval_summary_host.py."""
import numpy as np
import pytest
import torch

import eval_summary_cases as cases
import eval_summary_ref as ref
from test_gpu_learn_rollout import REFUSED, _assert_same_handles, _assert_same_outputs, _bits, _mk, _np, _obs_now, _tick

pytestmark = pytest.mark.gpu

N, K = 320, cases.K
OFF = 1000
SEED, ALPHA, GAMMA, EPS = cases.SEED, cases.ALPHA, cases.GAMMA, cases.EPS
EVAL_NAME = "k_discrete_eval_rollout<PHILOX=%d,NOISE=%d,UNIT=%d,QLDS=%d,DOUBLE=%d>"


def _tables(cfg, double, n=N):
    return cases.tie_q(cases.random_q(cases.Q_SEED, n, cfg["state_space_size"], cfg["action_space_size"], double))


def _learner(env, algo, q0, **kw):
    env.set_learner(algo, **dict(dict(alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=SEED), **kw), q=torch.as_tensor(q0, device=env.device))


def _qbits(env):
    return env.get_q().view(torch.int32).clone()


# ---- evaluation
@pytest.mark.parametrize("rng", ["numpy", "philox"])
@pytest.mark.parametrize("algo", cases.EVAL_ALGOS)
@pytest.mark.parametrize("case", list(cases.EVAL_CASES))
def test_evaluation_twin_restatement_untouched_tables_and_untouched_learner_streams(case, algo, rng):
    cfg, kw = cases.EVAL_CASES[case]
    double = algo == "double_q"
    a, b = _mk(cfg, rng, env_id_offset=OFF, **kw), _mk(cfg, rng, env_id_offset=OFF, **kw)
    q0 = _tables(cfg, double)
    for e in (a, b):
        _learner(e, algo, q0)
    name = a.eval_kernel_name(K)
    assert name == EVAL_NAME % (rng == "philox", "transition_noise" in cfg, "reward_dist" not in cfg, case not in cases.GLOBAL_FORM, double), name
    autoreset = kw.get("autoreset", ref.SAME_STEP)
    q_before = _qbits(a)
    assert np.array_equal(_np(q_before), _bits(q0))
    pending, info = None, {}
    for launch in range(cases.LAUNCHES):
        assert _tick(a) == launch * K
        before = _obs_now(a)
        out = a.rollout_eval(K)
        assert out[4].dtype == torch.int32 and tuple(out[4].shape) == (K, N)
        _assert_same_outputs(out[:4], b.rollout(out[4]), (case, algo, rng, launch))
        obs, _, term, trunc = (_np(x) for x in out[:4])
        want, _, pending, i = ref.eval_run(q0, before, obs, term, trunc, autoreset, pending)
        ref.merge_info(info, i)
        got = _np(out[4])
        assert np.array_equal(got, want), (case, algo, rng, launch, "actions", np.argwhere(got != want)[:5])
        assert torch.equal(_qbits(a), q_before), (case, algo, rng, launch, "the tables changed")
    _assert_same_handles(a, b, rng)
    print(case, algo, rng, info)
    cases.eval_honest(info, double)
    if autoreset == ref.NEXT_STEP:
        assert info["reset_calls"] > 0
    # the learner's streams: had the evaluation consumed a word of them (or kept a carry), these launches would differ
    for launch in range(2):
        for x, (g, w) in enumerate(zip(a.rollout_learn(K), b.rollout_learn(K))):
            assert torch.equal(g, w), (case, algo, rng, "rollout_learn after", launch, x)
    assert torch.equal(_qbits(a), _qbits(b)) and not torch.equal(_qbits(a), q_before)
    _assert_same_handles(a, b, rng)
    a.close(); b.close()


@pytest.mark.parametrize("algo", cases.EVAL_ALGOS)
def test_a_per_env_parameter_handle_evaluates_to_the_same_bits_as_the_uniform_one(algo):
    uni, pe = _mk(cases.EVAL_CASES["cfg2"][0], "numpy"), _mk(cases.EVAL_CASES["cfg2"][0], "numpy")
    q0 = _tables(cases.EVAL_CASES["cfg2"][0], algo == "double_q")
    al, ga, ep = cases.pe_arrays(N)
    _learner(uni, algo, q0)
    _learner(pe, algo, q0, alpha=al, gamma=ga, epsilon=ep)
    assert ",PE=1" in pe.learn_kernel_name(K) and ",PE=1" not in uni.learn_kernel_name(K)
    assert pe.eval_kernel_name(K) == uni.eval_kernel_name(K) != ""          # one form serves both
    for launch in range(2):
        for g, w in zip(pe.rollout_eval(K), uni.rollout_eval(K)):
            assert torch.equal(g, w), launch
    assert torch.equal(_qbits(pe), _qbits(uni))
    _assert_same_handles(pe, uni, "numpy")
    uni.close(); pe.close()


@pytest.mark.parametrize("algo", cases.EVAL_ALGOS)
def test_the_global_form_by_option_equals_the_lds_form_and_the_names_say_which(algo):
    cfg = cases.EVAL_CASES["cfg2"][0]
    one, two = _mk(cfg, "numpy"), _mk(cfg, "numpy")
    two.set_kernel_options("NO_LEARN_LDS")
    q0 = _tables(cfg, algo == "double_q")
    for e in (one, two):
        _learner(e, algo, q0)
    tail = ",DOUBLE=%d>" % (algo == "double_q")
    assert one.eval_kernel_name(K).endswith("QLDS=1" + tail) and two.eval_kernel_name(K).endswith("QLDS=0" + tail)
    for launch in range(2):
        for g, w in zip(two.rollout_eval(K), one.rollout_eval(K)):
            assert torch.equal(g, w), launch
    assert torch.equal(_qbits(one), _qbits(two))
    big = _mk(cases.EVAL_CASES["s20"][0], "numpy")                          # 256 tables of 20 x 20 do not fit
    _learner(big, algo, _tables(cases.EVAL_CASES["s20"][0], algo == "double_q"))
    assert big.eval_kernel_name(K).endswith("QLDS=0" + tail)
    for e in (one, two, big):
        e.close()


def test_a_sarsa_handle_evaluates_like_a_q_learning_one_with_the_same_tables():
    cfg = cases.EVAL_CASES["cfg2"][0]
    q0 = _tables(cfg, False)
    a_s, a_q = _mk(cfg, "philox"), _mk(cfg, "philox")
    _learner(a_s, "sarsa", q0)
    _learner(a_q, "q_learning", q0)
    assert a_s.eval_kernel_name(K) == a_q.eval_kernel_name(K) != ""
    for launch in range(2):
        out = a_s.alloc_rollout_eval(K)
        got = a_s.rollout_eval(K, out=out)
        assert got[0].data_ptr() == out[0].data_ptr() and got[4].data_ptr() == out[4].data_ptr()
        for g, w in zip(got, a_q.rollout_eval(K)):
            assert torch.equal(g, w), launch
    _assert_same_handles(a_s, a_q, "philox")
    a_s.close(); a_q.close()


# ---- summaries
def _launch(env, algo, k, **kw):
    return env.rollout_eval(k, **kw) if algo == "eval" else env.rollout_learn(k, **kw)


def _assert_summary(summ, st, what):
    for (name, dt), t in zip(ref.FIELDS, summ.tensors()):
        g, w = _np(t), st[name]
        assert g.dtype == dt and g.shape == w.shape, (what, name)
        if dt == np.float64:
            g, w = g.view(np.int64), w.view(np.int64)
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5])


@pytest.mark.parametrize("rng", ["numpy", "philox"])
@pytest.mark.parametrize("algo", cases.SUMMARY_ALGOS + ("eval",))
@pytest.mark.parametrize("case", list(cases.SUMMARY_CASES))
def test_summary_launch_equals_the_rule_on_the_full_output_twin(case, algo, rng):
    cfg, kw = cases.SUMMARY_CASES[case]
    s, t = _mk(cfg, rng, env_id_offset=OFF, **kw), _mk(cfg, rng, env_id_offset=OFF, **kw)
    learner = "q_learning" if algo == "eval" else algo
    q0 = _tables(cfg, learner == "double_q")
    for e in (s, t):
        _learner(e, learner, q0)
    autoreset = kw.get("autoreset", ref.SAME_STEP)
    summ = s.episode_summary()
    assert all(not x.any() for x in summ.tensors())
    st, c, total, pending = ref.new_state5(N), ref.new_counters(), np.zeros(N), None
    for launch in range(cases.LAUNCHES):
        what = (case, algo, rng, launch)
        out = _launch(t, algo, K)
        assert _launch(s, algo, K, summary=summ) is summ
        _, rew, term, trunc = (_np(x) for x in out[:4])
        rc, pending = ref.reset_calls(term, trunc, autoreset, pending)
        st = ref.summary(rew, term, trunc, rc, st, c)
        _assert_summary(summ, st, what)
        assert torch.equal(_qbits(s), _qbits(t)), what
        assert _tick(s) == _tick(t) == (launch + 1) * K
        if launch == 0:                                  # a pop() in between: the running pair carries on
            got = summ.pop()
            want, st = ref.pop(st)
            for g, w in zip(got, want):
                assert np.array_equal(_np(g), w), what
            total += want[1]
            _assert_summary(summ, st, what + ("after pop",))
    total += st["return_sum"]
    # the observation every env shows: reset(mask=none set) after a launch that wrote no observation
    none = torch.zeros(N, dtype=torch.bool, device=s.device)
    os_, ot = s.reset(mask=none)[0], t.reset(mask=none)[0]
    assert torch.equal(os_, ot), (case, algo, rng, "observation after the summary launch")
    assert torch.equal(ot, out[0][K - 1])
    _assert_same_handles(s, t, rng)
    print(case, algo, rng, c)
    cases.summary_honest(c, total, case, algo)
    if algo != "eval":
        assert not np.array_equal(_np(_qbits(s)), _bits(q0))          # (it did learn)
    s.close(); t.close()


@pytest.mark.parametrize("algo", cases.SUMMARY_ALGOS + ("eval",))
def test_a_summary_call_sent_out_in_pieces_equals_one_launch(algo):
    """LEARN_SHORT_PIECES: launches of at most 5 steps; SARSA's carry and the summary's running pair cross the pieces"""
    cfg = cases.SUMMARY_CASES["cfg2"][0]
    one, many, full = (_mk(cfg, "numpy") for _ in range(3))
    many.set_kernel_options("LEARN_SHORT_PIECES")
    learner = "q_learning" if algo == "eval" else algo
    q0 = _tables(cfg, learner == "double_q")
    for e in (one, many, full):
        _learner(e, learner, q0)
    s1, sm = one.episode_summary(), many.episode_summary()
    st, c = ref.new_state5(N), ref.new_counters()
    for launch in range(2):
        _launch(one, algo, K, summary=s1)
        _launch(many, algo, K, summary=sm)
        out = _launch(full, algo, K)
        st = ref.summary(_np(out[1]), _np(out[2]), _np(out[3]), np.zeros((K, N), bool), st, c)
        for x in (s1, sm):
            _assert_summary(x, st, (algo, launch))
    assert c["spans_boundary"] > 0 and c["two_in_one_launch"] > 0, c
    assert torch.equal(_qbits(one), _qbits(many)) and torch.equal(_qbits(one), _qbits(full))
    _assert_same_handles(one, many, "numpy")
    _assert_same_handles(one, full, "numpy")
    for e in (one, many, full):
        e.close()


def test_step_after_a_summary_launch_and_clear_after_reset():
    cfg = cases.SUMMARY_CASES["cfg2"][0]
    s, t = _mk(cfg, "numpy"), _mk(cfg, "numpy")
    q0 = _tables(cfg, False)
    for e in (s, t):
        _learner(e, "q_learning", q0)
    summ = s.episode_summary()
    s.rollout_learn(K, summary=summ)
    t.rollout_learn(K)
    x = torch.as_tensor(np.random.default_rng(2).integers(0, 8, N).astype(np.int32), device=s.device)
    _assert_same_outputs(s.step(x)[:4], t.step(x)[:4], "step after a summary launch")
    mask = torch.as_tensor(np.random.default_rng(3).random(N) < 0.4, device=s.device)
    s.rollout_learn(5, summary=summ)
    t.rollout_learn(5)
    assert torch.equal(s.reset(mask=mask)[0], t.reset(mask=mask)[0])
    assert torch.equal(s.reset()[0], t.reset()[0])
    summ.clear()
    assert all(not v.any() for v in summ.tensors())
    out = t.rollout_eval(K)
    s.rollout_eval(K, summary=summ)
    _assert_summary(summ, ref.summary(_np(out[1]), _np(out[2]), _np(out[3]), np.zeros((K, N), bool), ref.new_state5(N)), "after clear")
    _assert_same_handles(s, t, "numpy")
    s.close(); t.close()


# ---- refusals
@pytest.mark.parametrize("case", list(REFUSED))
def test_unsupported_handles_are_refused_for_evaluation_with_the_reason(case):
    from mdp_playground_amd import RLToyVectorEnv
    cfg, kw, reason = REFUSED[case]
    cfg = dict(cfg)
    if "seeds" in kw:
        cfg.pop("seed")
    env = RLToyVectorEnv(**({} if "seeds" in kw else {"num_envs": 64}), **kw, **cfg)
    out = env.alloc_rollout(4) + (torch.empty((4, env.num_envs), dtype=torch.int32, device=env.device),)
    with pytest.raises(NotImplementedError, match=reason):
        env.rollout_eval(4, out=out)
    for call in (env.rollout_eval, env.rollout_learn):
        with pytest.raises(NotImplementedError, match=reason):
            call(4, summary=env.episode_summary())
    assert env.eval_kernel_name(4) == ""
    env.close()


def test_rollout_eval_needs_a_learner():
    from mdp_playground_amd import _capi as capi
    env = _mk(cases.EVAL_CASES["cfg2"][0], "numpy")
    assert env.eval_kernel_name(4) == ""
    for kw in ({}, dict(summary=env.episode_summary())):
        with pytest.raises(capi.MdppError, match="no learner"):
            env.rollout_eval(4, **kw)
    with pytest.raises(capi.MdppError, match="no learner"):
        env.rollout_learn(4, summary=env.episode_summary())
    env.set_learner("sarsa", alpha=ALPHA, gamma=GAMMA, epsilon=EPS)
    env.rollout_eval(4)
    env.set_learner(None)
    with pytest.raises(capi.MdppError, match="no learner"):
        env.rollout_eval(4)
    assert _tick(env) == 4 and not env.status().any()
    env.close()


def test_a_summary_of_another_size_device_or_dtype_is_a_value_error_before_any_device_work():
    from mdp_playground_amd.summary import EpisodeSummary
    env, other = _mk(cases.EVAL_CASES["cfg2"][0], "numpy"), _mk(cases.EVAL_CASES["cfg2"][0], "numpy", n=N - 1)
    _learner(env, "q_learning", _tables(cases.EVAL_CASES["cfg2"][0], False))
    q_before, state_before = _qbits(env), env.get_augmented_state()
    wrong_dtype = env.episode_summary()
    wrong_dtype.ret = wrong_dtype.ret.to(torch.float32)
    wrong_int = env.episode_summary()
    wrong_int.episodes = wrong_int.episodes.to(torch.int64)
    strided = env.episode_summary()
    strided.len = torch.zeros(2 * N, dtype=torch.int32, device=env.device)[::2]
    bad = (other.episode_summary(), EpisodeSummary(N, "cpu"), wrong_dtype, wrong_int, strided, "summary", (1, 2, 3, 4, 5))
    for summ in bad:
        for call in (env.rollout_learn, env.rollout_eval):
            with pytest.raises(ValueError):
                call(K, summary=summ)
    with pytest.raises(ValueError):
        env.rollout_learn(K, out=env.alloc_rollout_learn(K), summary=env.episode_summary())
    assert _tick(env) == 0 and torch.equal(_qbits(env), q_before)
    after = env.get_augmented_state()
    assert all(np.array_equal(after[k], state_before[k]) for k in after)
    env.rollout_learn(K, summary=env.episode_summary())
    assert _tick(env) == K and not env.status().any()
    env.close(); other.close()
