"""The closed-loop kernels beyond square 8 x 8 MDPs (k_discrete_policy_rollout, k_discrete_learn_rollout, k_discrete_eval_rollout
and the SUMMARY forms): rectangular shapes (S != A through diameter > 1 and through use_custom_mdp matrices, whose R(s, a)
keys no other closed-loop test runs), sequence_length 4 and 7 (history bytes 4-7 of the state record), truncation with a
reset, the reward plumbing (scale, shift, terminal reward, every-n, the delay line at 32 and 33), A = 1, 6, 9 and 85, S = 255,
the QLDS decision at the device's limit, float edges of the tables, N = 1, 63, 257 and launches of one step.

The yardsticks are those of tests/test_gpu_learn_rollout.py, tests/test_gpu_learn_sweep.py, tests/test_gpu_eval_summary.py and
tests/test_gpu_policy_rollout.py, whose helpers this file uses: the open-loop twin (an identically built handle fed with the
actions the launch returned: outputs, state record, streams, tick -- through it the general kernels read and write the same
record) and the numpy restatements fed with the launch's own outputs, bit for bit.  The cases, and what a pass must have
exercised, are in tests/closed_loop_shape_cases.py; tests/test_closed_loop_shapes_host.py shows on the CPU that those
conditions can be met.  N = 320, K = 37, two launches."""
import numpy as np
import pytest
import torch

import closed_loop_shape_cases as cases
import eval_summary_ref as eref
import learner_sweep_ref as ref
from closed_loop_cpu import closed_loop
from test_gpu_eval_summary import _assert_summary, _launch, _qbits
from test_gpu_learn_rollout import _assert_same_handles, _assert_same_outputs, _bits, _mk, _np, _obs_now, _tick
from test_gpu_learn_sweep import Restated, _check_launch
from test_gpu_policy_rollout import SEED as POLICY_SEED, _assert_action_law, _policy

pytestmark = pytest.mark.gpu

N, K = 320, cases.K
OFF = 1000
SEED, ALPHA, GAMMA, EPS = cases.SEED, cases.ALPHA, cases.GAMMA, cases.EPS
LEARN_NAME = "%s<PHILOX=%d,NOISE=%d,UNIT=%d,QLDS=%d%s%s>"
EVAL_NAME = "%s<PHILOX=%d,NOISE=%d,UNIT=%d,QLDS=%d,DOUBLE=%d>"


def _lds_limit():
    """the device's shared memory per block, as torch reports it"""
    p = torch.cuda.get_device_properties(torch.cuda.current_device())
    return max(int(p.shared_memory_per_block), int(getattr(p, "shared_memory_per_block_optin", 0)))


def _learn_name(cfg, rng, double, pe=False, summary=False, qlds=None):
    _, _, _, _, unit, _ = cases.shape_of(cfg)
    qlds = cases.qlds_expected(cfg, double, _lds_limit()) if qlds is None else qlds
    return LEARN_NAME % ("k_discrete_learn_summary" if summary else "k_discrete_learn_rollout", rng == "philox", "reward_noise" in cfg, unit, qlds,
                         ",PE=1" if pe else "", ",DOUBLE=1" if double else "")


def _eval_name(cfg, rng, double, qlds=None):
    _, _, _, _, unit, _ = cases.shape_of(cfg)
    qlds = cases.qlds_expected(cfg, double, _lds_limit()) if qlds is None else qlds
    return EVAL_NAME % ("k_discrete_eval_rollout", rng == "philox", "reward_noise" in cfg, unit, qlds, double)


def _dev(env, q):
    return None if q is None else torch.as_tensor(q, device=env.device)


def _set_learner(env, algo, q0=None, alpha=ALPHA, gamma=GAMMA, epsilon=EPS):
    env.set_learner(algo, alpha=alpha, gamma=gamma, epsilon=epsilon, seed=SEED, q=_dev(env, q0))


class Flow:
    """the steps of a pass, gathered launch by launch for cases.flow_honest"""

    def __init__(self, autoreset):
        self.autoreset, self.pending, self.rows = autoreset, None, []

    def add(self, before, out):
        obs, rew, term, trunc, act = (_np(x) for x in out)
        rc, self.pending = eref.reset_calls(term, trunc, self.autoreset, self.pending)
        self.rows.append((np.concatenate([before[None], obs[:-1]]).astype(np.int64), act.astype(np.int64), rew, term, trunc, rc))

    def arrays(self):
        return tuple(np.concatenate(x) for x in zip(*self.rows))


# ---- the learners
def _learner_pass(case, algo, rng, pe):
    cfg, kw = cases.CASES[case]
    double = algo == "double_q"
    a, b = _mk(cfg, rng, env_id_offset=OFF, **kw), _mk(cfg, rng, env_id_offset=OFF, **kw)
    q0 = cases.start_tables(case, N, double)
    al, ga, ep = cases.pe_arrays(N) if pe else (ALPHA, GAMMA, EPS)
    _set_learner(a, algo, q0, al, ga, ep)
    name = a.learn_kernel_name(K)
    assert name == _learn_name(cfg, rng, double, pe), name
    autoreset = kw.get("autoreset", ref.SAME_STEP)
    r = Restated(a, algo, q0=q0, off=OFF, alpha=al, gamma=ga, eps=ep, autoreset=autoreset)
    assert r.Q.shape[-2:] == cases.shape_of(cfg)[:2]
    flow = Flow(autoreset)
    for launch in range(cases.LAUNCHES):
        what = (case, algo, rng, pe, launch)
        assert _tick(a) == launch * K
        before = _obs_now(a)
        out = _check_launch(a, r, K, what)
        _assert_same_outputs(out[:4], b.rollout(out[4]), what)
        flow.add(before, out)
    _assert_same_handles(a, b, rng)
    print(case, algo, rng, "pe" if pe else "", name, {k: v for k, v in r.info.items() if not isinstance(v, np.ndarray)})
    if pe:
        cases.pe_honest(r.info, ep)
    else:
        cases.learner_honest(case, algo, r.info, r.Q, q0)
        cases.flow_honest(case, cfg, *flow.arrays())
    a.close(); b.close()


@pytest.mark.parametrize("case,algo,rng", cases.LEARN_RUNS)
def test_learners_twin_and_restatement(case, algo, rng):
    assert cases.learner_refused(cases.CASES[case][0]) is None        # (no case's tables are beyond LDS: every one runs)
    _learner_pass(case, algo, rng, False)


@pytest.mark.parametrize("algo", cases.ALGOS)
@pytest.mark.parametrize("case", list(cases.CASES))
def test_learners_with_per_env_parameters_on_the_first_stream(case, algo):
    _learner_pass(case, algo, cases.STREAMS[case][algo][0], True)


def test_truncation_noise_and_same_step_autoreset_predicted_on_the_cpu():
    """learn() sees a next state that no output shows: the whole launch -- actions, the four outputs, the tables -- is the
    oracle env's, driven by the restatement on the CPU (Philox streams, N = 64)"""
    name, cfg, kw = cases.PREDICTED_CASE
    n = cases.PREDICTED_N
    for algo in cases.ALGOS:
        info, Q, traj = closed_loop(cfg, kw, algo, ALPHA, GAMMA, EPS, n, None, seed=SEED, K=K, launches=cases.LAUNCHES)
        a = _mk(cfg, "philox", n=n, **kw)
        _set_learner(a, algo)
        assert a.learn_kernel_name(K) == _learn_name(cfg, "philox", algo == "double_q")
        assert np.array_equal(_obs_now(a), traj["obs0"])
        for launch in range(cases.LAUNCHES):
            sl = slice(launch * K, (launch + 1) * K)
            obs, rew, term, trunc, act = (_np(x) for x in a.rollout_learn(K))
            for nm, g, w in (("actions", act, traj["actions"][sl]), ("obs", obs, traj["obs"][sl]), ("reward", _bits(rew), _bits(traj["reward"][sl])),
                             ("terminated", term, traj["terminated"][sl]), ("truncated", trunc, traj["truncated"][sl])):
                assert np.array_equal(g, w), (algo, launch, nm, np.argwhere(g != w)[:5])
        q = _np(a.get_q())
        assert np.array_equal(_bits(q), _bits(Q)), (algo, np.argwhere(_bits(q) != _bits(Q))[:5])
        cut = traj["truncated"] & ~traj["terminated"]
        assert (traj["next_state"][cut] != traj["obs"][cut]).any() and info["trunc_resets"] > 0
        if algo == "sarsa":
            assert info["trunc_carry_differs"] > 0
        assert not a.status().any()
        a.close()


# ---- evaluation
@pytest.mark.parametrize("rng", ["numpy", "philox"])
@pytest.mark.parametrize("algo", cases.EVAL_ALGOS)
@pytest.mark.parametrize("case", list(cases.CASES))
def test_evaluation_twin_restatement_and_untouched_tables(case, algo, rng):
    cfg, kw = cases.CASES[case]
    double = algo == "double_q"
    a, b = _mk(cfg, rng, env_id_offset=OFF, **kw), _mk(cfg, rng, env_id_offset=OFF, **kw)
    q0 = cases.eval_tables(cfg, N, double)
    _set_learner(a, algo, q0)
    name = a.eval_kernel_name(K)
    assert name == _eval_name(cfg, rng, double), name
    autoreset = kw.get("autoreset", ref.SAME_STEP)
    q_before = _qbits(a)
    assert np.array_equal(_np(q_before), _bits(q0))
    pending, info, flow = None, {}, Flow(autoreset)
    for launch in range(cases.LAUNCHES):
        what = (case, algo, rng, launch)
        before = _obs_now(a)
        out = a.rollout_eval(K)
        _assert_same_outputs(out[:4], b.rollout(out[4]), what)
        obs, _, term, trunc = (_np(x) for x in out[:4])
        want, _, pending, i = eref.eval_run(q0, before, obs, term, trunc, autoreset, pending)
        eref.merge_info(info, i)
        got = _np(out[4])
        assert np.array_equal(got, want), (what, "actions", np.argwhere(got != want)[:5])
        assert torch.equal(_qbits(a), q_before), (what, "the tables changed")
        flow.add(before, out)
    _assert_same_handles(a, b, rng)
    print(case, algo, rng, name, info)
    cases.eval_honest(case, info, double)
    if case in cases.DELAY_LINE:
        _, _, rew, _, _, rc = flow.arrays()
        cases.delay_line_honest(cfg, rew, rc)
    a.close(); b.close()


# ---- the policy
@pytest.mark.parametrize("rng", ["numpy", "philox"])
@pytest.mark.parametrize("case", list(cases.CASES))
def test_policy_twin_and_action_law_or_the_refusal(case, rng):
    from mdp_playground_amd.policy import policy_thresholds
    cfg, kw = cases.CASES[case]
    S, A = cases.shape_of(cfg)[:2]
    a = _mk(cfg, rng, env_id_offset=OFF, **kw)
    stochastic, deterministic = _policy(11, S, A), np.random.default_rng(12).integers(0, A, S)
    reason = cases.policy_refused(cfg)
    if reason is not None:               # the case does not vanish: it is refused, and says why
        for pol in (stochastic, deterministic):
            with pytest.raises(NotImplementedError, match=reason):
                a.set_policy(pol, seed=POLICY_SEED)
        with pytest.raises(NotImplementedError, match=reason):
            a.rollout_policy(4)
        assert a.policy_kernel_name(K) == ""
        a.close()
        return
    b = _mk(cfg, rng, env_id_offset=OFF, **kw)
    name = a.policy_kernel_name(K)
    assert name == "k_discrete_policy_rollout<PHILOX=%d,UNIT=%d,OBS64=1,A8=%d>" % (rng == "philox", cases.shape_of(cfg)[4], A <= 8), name
    obs_before = _np(a._obs)
    ended = 0
    for launch, pol in enumerate((stochastic, deterministic)):
        a.set_policy(pol, seed=POLICY_SEED)
        T = policy_thresholds(pol, S, A)
        assert T.shape == (S, A)
        tick0 = _tick(a)
        obs, rew, term, trunc, act = a.rollout_policy(K)
        _assert_action_law(T, POLICY_SEED, OFF, tick0, obs_before, _np(obs), _np(act))
        if launch == 1:
            states = np.concatenate([obs_before[None], _np(obs)[:-1]])
            assert np.array_equal(_np(act), deterministic[states])
        _assert_same_outputs((obs, rew, term, trunc), b.rollout(act), (case, rng, launch))
        ended += int(_np(term).sum()) + int(_np(trunc).sum())
        obs_before = _np(obs)[-1]
        if case in cases.RECT:
            assert int(_np(obs).max()) >= A
    _assert_same_handles(a, b, rng)
    assert ended > 0 or case == "a1_s3"
    a.close(); b.close()


# ---- summaries
@pytest.mark.parametrize("rng", ["numpy", "philox"])
@pytest.mark.parametrize("algo", cases.ALGOS + ("eval",))
@pytest.mark.parametrize("case", cases.SUMMARY_CASES)
def test_summary_launch_equals_the_rule_on_the_full_output_twin(case, algo, rng):
    cfg, kw = cases.CASES[case]
    s, t = _mk(cfg, rng, env_id_offset=OFF, **kw), _mk(cfg, rng, env_id_offset=OFF, **kw)
    learner = "q_learning" if algo == "eval" else algo
    q0 = cases.eval_tables(cfg, N, learner == "double_q")
    for e in (s, t):
        _set_learner(e, learner, q0)
    autoreset = kw.get("autoreset", ref.SAME_STEP)
    summ = s.episode_summary()
    st, c, total, pending = eref.new_state5(N), eref.new_counters(), np.zeros(N), None

    def both(k, what):
        nonlocal st, pending
        out = _launch(t, algo, k)
        assert _launch(s, algo, k, summary=summ) is summ
        _, rew, term, trunc = (_np(x) for x in out[:4])
        rc, pending = eref.reset_calls(term, trunc, autoreset, pending)
        st = eref.summary(rew, term, trunc, rc, st, c)
        _assert_summary(summ, st, what)
        assert torch.equal(_qbits(s), _qbits(t)), what
        assert _tick(s) == _tick(t)
        return out

    for launch in range(cases.LAUNCHES):
        both(K, (case, algo, rng, launch))
        if launch == 0:
            got = summ.pop()
            want, st = eref.pop(st)
            for g, w in zip(got, want):
                assert np.array_equal(_np(g), w), (case, algo, rng)
            total += want[1]
    total += st["return_sum"]
    _assert_same_handles(s, t, rng)
    print(case, algo, rng, c)
    cases.summary_honest(c, total, case, algo)
    # reset(mask=...) after a launch that wrote no observation, and one more launch
    mask = torch.as_tensor(np.random.default_rng(3).random(N) < 0.4, device=s.device)
    os_, ot = s.reset(mask=mask)[0], t.reset(mask=mask)[0]
    assert torch.equal(os_, ot), (case, algo, rng, "observation after the summary launch and a masked reset")
    if autoreset == ref.NEXT_STEP:
        pending = pending & ~_np(mask)                   # (a reset env has no reset call pending)
    # the running pair of a reset env goes on counting: the handle knows nothing of the summary object
    both(9, (case, algo, rng, "after reset(mask)"))
    _assert_same_handles(s, t, rng)
    s.close(); t.close()


# ---- hand-over of the state record to and from the other kernels
@pytest.mark.parametrize("rng", ["numpy", "philox"])
@pytest.mark.parametrize("algo", ["q_learning", "sarsa"])
@pytest.mark.parametrize("case", cases.HANDOVER_CASES)
def test_interleaved_with_policy_rollouts_open_loop_rollouts_steps_and_resets(case, algo, rng):
    """rollout_learn(5), step(), rollout(9), rollout_policy(8), rollout_learn(8), reset(mask), rollout_learn(6): on s4_L7 word 1
    of the state record is history bytes 4-7 (not a queue of start states), on custom_13x12 the key ring holds R(s, a) keys"""
    cfg, kw = cases.CASES[case]
    a, b = _mk(cfg, rng, **kw), _mk(cfg, rng, **kw)
    S, A = cases.shape_of(cfg)[:2]
    rs = np.random.default_rng(21)
    dev = a.device
    _set_learner(a, algo)
    r = Restated(a, algo)
    rewards = []

    def learn(k, what):
        out = _check_launch(a, r, k, what)
        _assert_same_outputs(out[:4], b.rollout(out[4]), what)
        rewards.append(_np(out[1]))

    learn(5, "rollout_learn(5)")
    x = torch.as_tensor(rs.integers(0, A, N).astype(np.int32), device=dev)
    _assert_same_outputs(a.step(x)[:4], b.step(x)[:4], "step")
    xs = torch.as_tensor(rs.integers(0, A, (9, N)).astype(np.int32), device=dev)
    _assert_same_outputs(a.rollout(xs), b.rollout(xs), "rollout(9)")
    a.set_policy(rs.integers(0, A, S), seed=3)
    out = a.rollout_policy(8)
    _assert_same_outputs(out[:4], b.rollout(out[4]), "rollout_policy(8)")
    assert np.array_equal(_bits(_np(a.get_q())), _bits(r.Q))       # (none of these touched the tables)
    learn(8, "rollout_learn(8)")
    mask = torch.as_tensor(rs.random(N) < 0.4, device=dev)
    assert torch.equal(a.reset(mask=mask)[0], b.reset(mask=mask)[0])
    learn(6, "rollout_learn(6)")
    _assert_same_handles(a, b, rng)
    # the learning launches after the other kernels' steps paid rewards: histories of 7 states built up across the hand-overs
    assert any((x != 0).any() for x in rewards[1:]), case
    a.close(); b.close()


# ---- the QLDS decision at the device's limit
@pytest.mark.parametrize("shape", list(cases.QLDS_EDGE))
def test_the_lds_form_near_the_limit_equals_the_global_form_and_the_name_says_which(shape):
    cfg, double = cases.QLDS_EDGE[shape]
    algo = "double_q" if double else "q_learning"
    limit = _lds_limit()
    need = cases.static_lds(cfg) + cases.lds_bytes(cfg) + cases.q_lds(cfg, double)
    fits = cases.qlds_expected(cfg, double, limit)
    print(shape, "static %d + MDP %d + Q %d = %d bytes against %d: QLDS=%d" % (cases.static_lds(cfg), cases.lds_bytes(cfg), cases.q_lds(cfg, double),
                                                                                need, limit, fits))
    q0 = cases.eval_tables(cfg, N, double)
    for form in ("learn", "eval"):
        one, two = _mk(cfg, "numpy"), _mk(cfg, "numpy")
        two.set_kernel_options("NO_LEARN_LDS")
        for e in (one, two):
            _set_learner(e, algo, q0)
        if form == "learn":
            assert one.learn_kernel_name(K) == _learn_name(cfg, "numpy", double, qlds=fits), one.learn_kernel_name(K)
            assert two.learn_kernel_name(K) == _learn_name(cfg, "numpy", double, qlds=False), two.learn_kernel_name(K)
        else:
            assert one.eval_kernel_name(K) == _eval_name(cfg, "numpy", double, qlds=fits), one.eval_kernel_name(K)
            assert two.eval_kernel_name(K) == _eval_name(cfg, "numpy", double, qlds=False), two.eval_kernel_name(K)
        s1, s2 = one.episode_summary(), two.episode_summary()
        for launch in range(2):
            for x, (g, w) in enumerate(zip(_launch(two, form, K), _launch(one, form, K))):
                assert torch.equal(g, w), (shape, form, launch, x)
            assert torch.equal(_qbits(one), _qbits(two)), (shape, form, launch)
            # the summary forms, from where the full-output launches left the handles
            _launch(one, form, K, summary=s1)
            _launch(two, form, K, summary=s2)
            for g, w in zip(s2.tensors(), s1.tensors()):
                assert torch.equal(g, w), (shape, form, launch, "summary")
            assert torch.equal(_qbits(one), _qbits(two)), (shape, form, launch, "summary")
        assert int(s1.episodes.sum()) > 0
        if form == "learn":
            assert not np.array_equal(_np(_qbits(one)), _bits(q0))
        else:
            assert np.array_equal(_np(_qbits(one)), _bits(q0))
        _assert_same_handles(one, two, "numpy")
        one.close(); two.close()


# ---- float edges of the tables
def _same_floats(got, want, what):
    """bit for bit, except that a NaN is compared by position (inf - inf has no one bit pattern)"""
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (what, "NaN positions", np.argwhere(gn != wn)[:5])
    g, w = _bits(got)[~gn], _bits(want)[~gn]
    assert np.array_equal(g, w), (what, int((g != w).sum()))


@pytest.mark.parametrize("algo", cases.ALGOS)
@pytest.mark.parametrize("case", list(cases.FLOAT_EDGE_CASES))
def test_float_edges_of_the_tables_learners_and_evaluation(case, algo):
    cfg, kw = cases.FLOAT_EDGE_CASES[case]
    S, A = cases.shape_of(cfg)[:2]
    double = algo == "double_q"
    q0 = cases.float_edge_tables(3, N, S, A, double)
    a, b = _mk(cfg, "philox", **kw), _mk(cfg, "philox", **kw)
    _set_learner(a, algo, q0)
    assert np.array_equal(_bits(_np(a.get_q())), _bits(q0))                  # (the round trip keeps -0.0 and the denormals)
    # evaluation first: it changes nothing
    before = _obs_now(a)
    out = a.rollout_eval(K)
    obs, _, term, trunc = (_np(x) for x in out[:4])
    want, _, _, einfo = eref.eval_run(q0, before, obs, term, trunc, ref.SAME_STEP)
    assert np.array_equal(_np(out[4]), want), (case, algo, "evaluation", np.argwhere(_np(out[4]) != want)[:5])
    assert np.array_equal(_bits(_np(a.get_q())), _bits(q0))
    _assert_same_outputs(out[:4], b.rollout(out[4]), (case, algo, "evaluation"))
    assert einfo["greedy_ties"] > 0 and einfo["greedy_strict"] > 0
    r = Restated(a, algo, q0=q0)
    for launch in range(cases.LAUNCHES):
        what = (case, algo, launch)
        before, tick0 = _obs_now(a), _tick(a)
        out = a.rollout_learn(K)
        want = r.launch(tick0, before, out)
        got = _np(out[4])
        assert np.array_equal(got, want), (what, "actions", np.argwhere(got != want)[:5])
        _same_floats(_np(a.get_q()), r.Q, what)
        _assert_same_outputs(out[:4], b.rollout(out[4]), what)
    print(case, algo, {k: v for k, v in r.info.items() if not isinstance(v, np.ndarray)})
    cases.float_edge_honest(r.info)
    assert np.isnan(r.Q).any()
    # and greedy evaluation of tables that now hold NaNs: the scan never moves on to a NaN, and never off one at j = 0
    before = _obs_now(a)
    out = a.rollout_eval(K)
    obs, _, term, trunc = (_np(x) for x in out[:4])
    want = eref.eval_run(r.Q, before, obs, term, trunc, ref.SAME_STEP)[0]
    assert np.array_equal(_np(out[4]), want), (case, algo, "evaluation of NaNs", np.argwhere(_np(out[4]) != want)[:5])
    _assert_same_outputs(out[:4], b.rollout(out[4]), (case, algo, "evaluation of NaNs"))
    _assert_same_handles(a, b, "philox")
    a.close(); b.close()


# ---- N edges
@pytest.mark.parametrize("algo", ["q_learning", "double_q"])
@pytest.mark.parametrize("n", cases.N_EDGES)
def test_one_env_63_envs_and_a_one_lane_second_workgroup(n, algo):
    a, b = _mk(cases.CFG2, "numpy", n=n), _mk(cases.CFG2, "numpy", n=n)
    double = algo == "double_q"
    _set_learner(a, algo)
    q = cases.random_q(6, n, 8, 8, double)
    a.set_q(torch.as_tensor(q, device=a.device))
    got = _np(a.get_q())
    assert got.shape == q.shape and np.array_equal(_bits(got), _bits(q))      # (the entry-major buffer and back: the transpose divides by N)
    r = Restated(a, algo, q0=q)
    for launch in range(cases.LAUNCHES):
        out = _check_launch(a, r, K, (n, algo, launch))
        _assert_same_outputs(out[:4], b.rollout(out[4]), (n, algo, launch))
    _assert_same_handles(a, b, "numpy")
    assert r.info["explored"] > 0 and r.info["greedy_strict"] > 0
    a.close(); b.close()


# ---- launches of one step at every tick phase
@pytest.mark.parametrize("rng", ["numpy", "philox"])
@pytest.mark.parametrize("algo", cases.ALGOS)
def test_nine_launches_of_one_step(algo, rng):
    a, b = _mk(cases.CFG2, rng), _mk(cases.CFG2, rng)
    q0 = cases.random_q(7, N, 8, 8, algo == "double_q")
    for e in (a, b):
        _set_learner(e, algo, q0)
    r = Restated(a, algo, q0=q0)
    outs = [[x.clone() for x in _check_launch(a, r, 1, (algo, rng, k))] for k in range(9)]     # (sarsa: no carry from call to call)
    assert _tick(a) == 9 and r.info["carried"] == 0
    if algo == "sarsa":
        # one launch of nine steps carries its action; the nine calls each select afresh, as the restatement above did
        c = _mk(cases.CFG2, rng)
        _set_learner(c, algo, q0)
        rc = Restated(c, algo, q0=q0)
        _check_launch(c, rc, 9, (algo, rng, "one launch"))
        assert rc.info["carried"] > 0
        c.close()
        b.rollout(torch.cat([o[4] for o in outs]))
    else:
        want = b.rollout_learn(9)
        for x, w in enumerate(want):
            got = torch.cat([o[x] for o in outs])
            assert torch.equal(got, w), (algo, rng, x)
        assert torch.equal(_qbits(a), _qbits(b))
    _assert_same_handles(a, b, rng)
    a.close(); b.close()
