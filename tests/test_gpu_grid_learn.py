"""The grid learners on the GPU (k_grid_learn_rollout<PHILOX,NOISE,QLDS,EVAL,SUMMARY>; include/mdpp.h "Grid learners"):
RLToyVectorEnv.set_grid_learner / rollout_grid_learn / rollout_grid_eval, their summary= forms and the Q accessors.

Every case of tests/grid_learner_cases.py x {numpy, philox} x {q_learning, sarsa} runs at N = 320, K = 37, two launches, and is
held to (1) the open-loop twin -- an identically built handle fed the action vectors the launch returned: outputs, state
record, streams, status and step counter, bit for bit; (2) the restatement -- the CPU closed loop of tests/grid_learner_ref.py
on the same streams: every action, every output, and the final tables compared as int32; (3) the kernel's name.
tests/test_grid_learner_host.py shows on the CPU that the cases exercise what a pass claims."""
import ctypes as C

import numpy as np
import pytest
import torch

import eval_summary_ref as eref
import graph_replay_util as gru
import grid_learner_cases as gc
import grid_learner_ref as gref
import learner_sweep_ref as ref

pytestmark = pytest.mark.gpu

N, K = gc.N, gc.K
SEED = gc.LEARNER_SEED


def _mk(case, rng, n=N, **over):
    from mdp_playground_amd import RLToyVectorEnv
    c = gc.CASES[case]
    extra = dict(rng="philox", philox_seed=gc.PHILOX_SEED) if rng == "philox" else {}
    return RLToyVectorEnv(num_envs=n, env_id_offset=gc.ENV_ID_OFFSET, **extra, **dict(c["kw"], **over), **c["cfg"])


def _np(x):
    return x.cpu().numpy().copy()


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def _tick(env):
    return gru.tick(env)


def _dev(env, q, case):
    return None if q is None else torch.as_tensor(gref.as_grid(q, gc.CASES[case]["cfg"]["grid_shape"]), device=env.device)


def _set(env, case, algo, q0="case", rates=None, seed=SEED):
    c = gc.CASES[case]
    al, ga, ep = rates or c["rates"]
    q0 = gc.initial_tables(case, env.num_envs) if isinstance(q0, str) else q0
    env.set_grid_learner(algo, alpha=al, gamma=ga, epsilon=ep, seed=seed, q=_dev(env, q0, case), noop=c["noop"])


def _streams(env):
    from mdp_playground_amd import _capi as capi
    return [env.seeded_streams[s] for s in (capi.STREAM_ENV, capi.STREAM_SPACE, capi.STREAM_ACTION)]


def _assert_same_outputs(got, want, what):
    for name, g, w in zip(("obs", "reward", "terminated", "truncated", "actions"), got, want):
        g, w = _np(g) if torch.is_tensor(g) else np.asarray(g), _np(w) if torch.is_tensor(w) else np.asarray(w)
        if name == "reward":
            g, w = _bits(g.astype(np.float32)), _bits(w.astype(np.float32))
        assert g.shape == w.shape and np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5])


def _assert_same_handles(a, b, rng):
    from mdp_playground_amd import _capi as capi
    sa, sb = a.get_augmented_state(), b.get_augmented_state()
    assert sa.keys() == sb.keys()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    if rng == "numpy":
        for st in (capi.STREAM_ENV, capi.STREAM_SPACE, capi.STREAM_ACTION):
            assert np.array_equal(a.get_rng_streams(st), b.get_rng_streams(st)), st
    assert not a.status().any() and not b.status().any()
    assert _tick(a) == _tick(b)


def _assert_same_q(a, want, what):
    q = _np(a.get_grid_q()) if not isinstance(a, np.ndarray) else a
    w = _np(want.get_grid_q()) if not isinstance(want, np.ndarray) else want
    assert q.shape == w.shape and np.array_equal(_bits(q), _bits(w)), (what, np.argwhere(_bits(q) != _bits(w))[:5])


def _assert_launch_is_restated(out, traj, sl, what):
    want = (traj["obs"][sl], traj["reward"][sl], traj["terminated"][sl], traj["truncated"][sl], traj["vectors"][sl])
    _assert_same_outputs(out, want, what)


# ---- the cases: twin, restatement, name
@pytest.mark.parametrize("algo", gref.ALGOS)
@pytest.mark.parametrize("rng", ["numpy", "philox"])
@pytest.mark.parametrize("case", sorted(gc.CASES))
def test_learners_twin_restatement_and_name(case, rng, algo):
    a, b = _mk(case, rng), _mk(case, rng)
    _set(a, case, algo)
    name = a.grid_learn_kernel_name(K)
    assert name == gc.expected_name(case, rng), name
    info, Q, traj = gc.cpu_run(case, algo, _streams(a) if rng == "numpy" else None)
    assert np.array_equal(_np(a._obs), traj["obs0"])
    for launch in range(gc.LAUNCHES):
        what = (case, rng, algo, launch)
        assert _tick(a) == launch * K
        out = a.rollout_grid_learn(K)
        assert out[4].dtype == torch.int32 and tuple(out[4].shape) == (K, N, 2)
        _assert_launch_is_restated(out, traj, slice(launch * K, (launch + 1) * K), what)
        _assert_same_outputs(out[:4], b.rollout(out[4]), what)
    _assert_same_handles(a, b, rng)
    _assert_same_q(a, gref.as_grid(Q, gc.CASES[case]["cfg"]["grid_shape"]), (case, rng, algo))
    print(case, rng, algo, name, {k: v for k, v in info.items() if not isinstance(v, np.ndarray)})
    a.close(); b.close()


@pytest.mark.parametrize("rng", ["numpy", "philox"])
def test_noise_keys_named_at_zero(rng):
    """transition_noise = 0.0 leaves the handle without the transition key, reward_noise = 0.0 keeps the reward key: the NOISE
    kernel draws its normal and adds 0 times it, as mdpp_step_n does"""
    cfg = dict(gc.CASES["g34_dense"]["cfg"], transition_noise=0.0, reward_noise=0.0)
    kw, n, k = dict(autoreset="same_step", max_episode_steps=8), 130, 21
    from mdp_playground_amd import RLToyVectorEnv
    extra = dict(rng="philox", philox_seed=gc.PHILOX_SEED) if rng == "philox" else {}
    a, b = (RLToyVectorEnv(num_envs=n, env_id_offset=gc.ENV_ID_OFFSET, **extra, **kw, **cfg) for _ in range(2))
    a.set_grid_learner("sarsa", alpha=0.5, gamma=0.9, epsilon=0.3, seed=SEED)
    assert a.grid_learn_kernel_name(k) == "k_grid_learn_rollout<PHILOX=%d,NOISE=1,QLDS=1,EVAL=0,SUMMARY=0>" % (rng == "philox")
    info, Q, traj = gref.closed_loop(cfg, kw, "sarsa", 0.5, 0.9, 0.3, n, seed=SEED, K=k, launches=2, philox_seed=gc.PHILOX_SEED,
                                     off=gc.ENV_ID_OFFSET, streams=_streams(a) if rng == "numpy" else None)
    assert info["terminations"] > 0 and info["truncations"] > 0 and info["redrawn_moves"] == 0
    for launch in range(2):
        out = a.rollout_grid_learn(k)
        _assert_launch_is_restated(out, traj, slice(launch * k, (launch + 1) * k), (rng, launch))
        _assert_same_outputs(out[:4], b.rollout(out[4]), (rng, launch))
    _assert_same_handles(a, b, rng)
    _assert_same_q(a, gref.as_grid(Q, cfg["grid_shape"]), rng)
    a.close(); b.close()


@pytest.mark.parametrize("n", [1, 63, 257])
def test_small_and_ragged_sizes_and_launches_of_one_step(n):
    case, algo = "g34_noise_next_i32", "sarsa"
    c = gc.CASES[case]
    for rng in ("numpy", "philox"):
        a, b = _mk(case, rng, n=n), _mk(case, rng, n=n)
        _set(a, case, algo, q0=None)
        state, Q, t0 = None, None, 0
        for k in (1, 7, 1):
            info, Q, traj = gref.closed_loop(c["cfg"], c["kw"], algo, *c["rates"], n, Q, seed=SEED, K=k, launches=1, noop=c["noop"],
                                             philox_seed=gc.PHILOX_SEED, off=gc.ENV_ID_OFFSET, streams=_streams(a) if rng == "numpy" else None,
                                             tick0=t0, state=state)
            state, t0 = traj["state_out"], t0 + k
            out = a.rollout_grid_learn(k)
            _assert_launch_is_restated(out, traj, slice(0, k), (n, rng, k))
            _assert_same_outputs(out[:4], b.rollout(out[4]), (n, rng, k))
        _assert_same_handles(a, b, rng)
        _assert_same_q(a, gref.as_grid(Q, c["cfg"]["grid_shape"]), (n, rng))
        a.close(); b.close()


def test_per_env_parameters_equal_uniform_handles_at_each_triple():
    case, algo = "g55_sparse_limit_i32", "sarsa"
    triples = [(0.5, 0.9, 0.3), (0.125, 0.5, 0.0), (1.0, 1.0, 1.0)]
    which = np.arange(N) % 3
    al, ga, ep = (np.array([triples[w][j] for w in which], np.float32) for j in range(3))
    a = _mk(case, "philox")
    _set(a, case, algo, rates=(al, torch.as_tensor(ga), ep))
    outs = [a.rollout_grid_learn(K), a.rollout_grid_learn(K)]
    qa = _np(a.get_grid_q())
    for t, triple in enumerate(triples):
        u = _mk(case, "philox")
        _set(u, case, algo, rates=triple)
        sel = which == t
        for launch in range(2):
            o = u.rollout_grid_learn(K)
            for name, g, w in zip(("obs", "reward", "terminated", "truncated", "actions"), outs[launch], o):
                g, w = np.ascontiguousarray(_np(g)[:, sel]), np.ascontiguousarray(_np(w)[:, sel])
                assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), (t, launch, name)
        assert np.array_equal(_bits(qa[sel]), _bits(_np(u.get_grid_q())[sel])), t
        u.close()
    # new rates through set_grid_learner_rates: the handle goes on like one that had them from this launch on
    b = _mk(case, "philox")
    _set(b, case, algo, rates=(al, ga, ep))
    b.rollout_grid_learn(K); b.rollout_grid_learn(K)
    a.set_grid_learner_rates(alpha=0.25, epsilon=ep[::-1].copy())
    b.set_grid_learner_rates(alpha=np.full(N, 0.25, np.float32), gamma=ga, epsilon=ep[::-1].copy())
    _assert_same_outputs(a.rollout_grid_learn(K), b.rollout_grid_learn(K), "rates")
    _assert_same_q(a, b, "rates")
    a.close(); b.close()


def test_initial_tables_and_q_round_trip_on_a_non_square_grid():
    case = "g34_dense"
    a = _mk(case, "numpy")
    r = np.random.default_rng(3)
    q = torch.as_tensor(r.standard_normal((N, 4, 5, 4)).astype(np.float32), device=a.device)
    a.set_grid_learner("q_learning", alpha=0.5, gamma=0.9, epsilon=0.1, q=q)
    assert np.array_equal(_bits(_np(a.get_grid_q())), _bits(_np(q)))
    q2 = torch.as_tensor(r.standard_normal((N, 4, 5, 4)).astype(np.float32), device=a.device)
    a.set_grid_q(q2)
    assert np.array_equal(_bits(_np(a.get_grid_q())), _bits(_np(q2)))
    with pytest.raises(ValueError, match="shape"):
        a.set_grid_q(q2.transpose(1, 2))
    with pytest.raises(ValueError, match="shape"):
        a.set_grid_learner("q_learning", alpha=0.5, gamma=0.9, epsilon=0.1, q=q, noop=True)
    # with the noop the tables have five columns; without q they start as zeros
    a.set_grid_learner("sarsa", alpha=0.5, gamma=0.9, epsilon=0.1, noop=True)
    assert tuple(a.get_grid_q().shape) == (N, 4, 5, 5) and not a.get_grid_q().any()
    a.close()


@pytest.mark.parametrize("case", ["g55_sparse_limit_i32", "g17_noise"])
def test_tables_in_lds_equal_tables_in_global_memory(case):
    for rng in ("numpy", "philox"):
        a, b = _mk(case, rng), _mk(case, rng)
        b.set_kernel_options("NO_GRID_QLDS")
        for env in (a, b):
            _set(env, case, "sarsa")
        assert a.grid_learn_kernel_name(K) == gc.expected_name(case, rng, qlds=1)
        assert b.grid_learn_kernel_name(K) == gc.expected_name(case, rng, qlds=0)
        for launch in range(2):
            _assert_same_outputs(a.rollout_grid_learn(K), b.rollout_grid_learn(K), (case, rng, launch))
        _assert_same_q(a, b, (case, rng))
        assert a.grid_learn_kernel_name(K, eval=True) == gc.expected_name(case, rng, eval=True, qlds=1)
        assert b.grid_learn_kernel_name(K, eval=True) == gc.expected_name(case, rng, eval=True, qlds=0)
        _assert_same_outputs(a.rollout_grid_eval(K), b.rollout_grid_eval(K), (case, rng, "eval"))
        _assert_same_handles(a, b, rng)
        a.close(); b.close()


# ---- greedy evaluation
@pytest.mark.parametrize("case,rng", [("g34_dense", "numpy"), ("g55_noop_next_every3", "philox"), ("g17_noise", "philox"), ("g88_disabled_pnoise", "numpy")])
def test_greedy_evaluation(case, rng):
    c = gc.CASES[case]
    g = c["cfg"]["grid_shape"]
    a, b, d = _mk(case, rng), _mk(case, rng), _mk(case, rng)
    for env in (a, d):
        _set(env, case, "q_learning")
    for _ in range(2):                          # (tables that have learnt something, a state in mid-episode)
        o = a.rollout_grid_learn(K)
        d.rollout_grid_learn(K)
        b.rollout(o[4])
    assert a.grid_learn_kernel_name(K, eval=True) == gc.expected_name(case, rng, eval=True)
    q_before = _np(a.get_grid_q())
    before = _np(a._obs_src)
    t0 = _tick(a)
    out = a.rollout_grid_eval(K)
    assert _tick(a) == t0 + K
    _assert_same_q(_np(a.get_grid_q()), q_before, "evaluation left the tables alone")
    # the actions are the restated argmax of the state each env shows
    obs, act = _np(out[0]).astype(np.int64), _np(out[4])
    Qf = gref.as_flat(q_before)
    s = gref.state_index(before[:, 0], before[:, 1], g)
    strict = 0
    for k in range(K):
        arg, best = ref.scan_best(Qf[np.arange(N), s])
        strict += int(((Qf[np.arange(N), s] == best[:, None]).sum(axis=1) == 1).sum())
        assert np.array_equal(act[k], gref.action_vector(arg)), k
        s = gref.state_index(obs[k, :, 0], obs[k, :, 1], g)
    assert strict > 0
    _assert_same_outputs(out[:4], b.rollout(out[4]), (case, rng, "twin"))
    _assert_same_handles(a, b, rng)
    # a following learn launch equals the same launch on a handle that stepped those actions through rollout()
    d.rollout(out[4])
    _assert_same_outputs(a.rollout_grid_learn(K), d.rollout_grid_learn(K), (case, rng, "learn after eval"))
    _assert_same_q(a, d, (case, rng))
    _assert_same_handles(a, d, rng)
    a.close(); b.close(); d.close()


# ---- summaries
def _state5(s):
    return {name: _np(t) for (name, _), t in zip(eref.FIELDS, s.tensors())}


@pytest.mark.parametrize("case,rng", [("g55_noop_next_every3", "numpy"), ("g17_noise", "philox"), ("g55_sparse_limit_i32", "philox")])
def test_summary_forms_against_the_full_output_twin(case, rng):
    autoreset = gc.CASES[case]["kw"]["autoreset"]
    a, b = _mk(case, rng), _mk(case, rng)
    for env in (a, b):
        _set(env, case, "sarsa")
    assert a.grid_learn_kernel_name(K, summary=True) == gc.expected_name(case, rng, summary=True)
    assert a.grid_learn_kernel_name(K, eval=True, summary=True) == gc.expected_name(case, rng, eval=True, summary=True)
    s = a.episode_summary()
    want, pending = eref.new_state5(N), None
    counters = eref.new_counters()
    for launch, ev in enumerate((False, False, True, False)):
        got = (a.rollout_grid_eval if ev else a.rollout_grid_learn)(K, summary=s)
        assert got is s
        obs, rew, term, trunc, act = (b.rollout_grid_eval if ev else b.rollout_grid_learn)(K)
        rc, pending = eref.reset_calls(_np(term), _np(trunc), autoreset, pending)
        want = eref.summary(_np(rew), _np(term), _np(trunc), rc, want, counters)
        for name, _ in eref.FIELDS:
            g, w = _state5(s)[name], want[name]
            assert g.dtype == w.dtype and np.array_equal(g.view(np.uint8), w.view(np.uint8)), (case, rng, launch, name)
        if launch == 1:                           # pop(): the finished episodes' three are read and zeroed, the running one goes on
            ep, rs, ls = s.pop()
            (wep, wrs, wls), want = eref.pop(want)
            assert np.array_equal(_np(ep), wep) and np.array_equal(_np(rs), wrs) and np.array_equal(_np(ls), wls)
    assert counters["ended_terminated"] > 0 and counters["two_in_one_launch"] > 0 and counters["spans_boundary"] > 0
    if autoreset == "next_step":
        assert counters["reset_calls"] > 0
    _assert_same_q(a, b, (case, rng))
    _assert_same_handles(a, b, rng)
    s.clear()
    assert not any(t.any() for t in s.tensors())
    with pytest.raises(ValueError):
        a.rollout_grid_learn(K, out=a.alloc_rollout_grid(K), summary=s)
    # reset(mask=) after a launch that wrote no observations shows the cells in the state record
    a.rollout_grid_learn(3, summary=s)
    out = b.rollout_grid_learn(3)
    mask = torch.zeros(N, dtype=torch.bool, device=a.device)
    assert np.array_equal(_np(a.reset(mask=mask)[0]), _np(out[0][2]))
    a.close(); b.close()


# ---- HIP graphs
def test_learning_launch_replayed_from_a_hip_graph():
    case, algo, rng = "g17_noise", "sarsa", "philox"
    a, b = _mk(case, rng), _mk(case, rng)
    for env in (a, b):
        _set(env, case, algo)
    out = a.alloc_rollout_grid(K)
    a.rollout_grid_learn(K, out)                 # the eager launch of the same form before the capture
    b.rollout_grid_learn(K)
    call = gru.capture(a, lambda: a.rollout_grid_learn(K, out), K)
    t0 = _tick(a)
    for replay in range(3):
        # open-loop steps in between: the replays run at counter offsets 3, 42 and 81 from the capture, no multiple of 4
        acts = torch.as_tensor(gref.action_vector(np.random.default_rng(replay).integers(0, 4, size=((3, 2, 2)[replay], N))), device=a.device)
        _assert_same_outputs(a.rollout(acts), b.rollout(acts), ("between", replay))
        assert _tick(a) - t0 == (3, 42, 81)[replay]
        call.replay()
        _assert_same_outputs(out, b.rollout_grid_learn(K), ("replay", replay))
    torch.cuda.synchronize()
    _assert_same_q(a, b, "graph")
    _assert_same_handles(a, b, rng)
    a.close(); b.close()


# ---- refusals, no learner, range errors
_GRID = dict(state_space_type="grid", reward_function="move_to_a_point", grid_shape=(4, 4), make_denser=True, target_point=[2, 2], seed=1)
REFUSED = {
    "discrete": (dict(state_space_type="discrete", action_space_type="discrete", state_space_size=8, action_space_size=8, delay=0,
                      sequence_length=1, seed=0), {}, "serve grid envs only"),
    "continuous": (dict(state_space_type="continuous", state_space_dim=4, target_point=[0, 0, 0, 0], target_radius=0.05, state_space_max=10,
                        action_space_max=1, transition_dynamics_order=1, inertia=1, time_unit=0.1, reward_function="move_to_a_point", seed=0),
                   {}, "serve grid envs only"),
    "irrelevant_features": (dict(_GRID, irrelevant_features=True), {}, "grid_dims == 2"),
    "image": (dict(_GRID, image_representations=True, image_width=32, image_height=32), {}, "image observations"),
    "episode_stats": (dict(_GRID), dict(episode_stats=True), "episode_stats"),
    "tables beyond 32-bit offsets": (dict(_GRID, grid_shape=(254, 254), target_point=[3, 3]), dict(num_envs=4224), "2\\^32"),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_unserved_handles_are_refused_with_the_reason(case):
    from mdp_playground_amd import RLToyVectorEnv
    cfg, kw, reason = REFUSED[case]
    env = RLToyVectorEnv(**dict(dict(num_envs=64), **kw), **cfg)
    for algo in gref.ALGOS:
        with pytest.raises(NotImplementedError, match=reason):
            env.set_grid_learner(algo, alpha=0.5, gamma=0.9, epsilon=0.1)
    assert env.grid_learn_kernel_name(4) == ""
    if case != "tables beyond 32-bit offsets":       # (that handle is refused for its tables, which the set call sizes)
        s = env.episode_summary()
        for call in (lambda: env.rollout_grid_learn(4), lambda: env.rollout_grid_eval(4), lambda: env.rollout_grid_learn(4, summary=s)):
            with pytest.raises(NotImplementedError, match=reason):
                call()
    # the discrete learner still refuses a grid handle
    if env.kind == "grid":
        with pytest.raises(NotImplementedError):
            env.set_learner("q_learning", alpha=0.5, gamma=0.9, epsilon=0.1)
    env.close()


def test_launches_and_accessors_need_a_learner():
    from mdp_playground_amd import _capi as capi
    case = "g34_dense"
    env = _mk(case, "numpy")
    s = env.episode_summary()
    for call in (lambda: env.rollout_grid_learn(4), lambda: env.rollout_grid_eval(4), lambda: env.rollout_grid_learn(4, summary=s),
                 lambda: env.rollout_grid_eval(4, summary=s), env.get_grid_q, lambda: env.set_grid_learner_rates(alpha=0.5)):
        with pytest.raises(capi.MdppError, match="no learner"):
            call()
    assert env.grid_learn_kernel_name(4) == ""
    _set(env, case, "sarsa")
    env.rollout_grid_learn(4)
    env.set_grid_learner(None)                   # cleared
    for call in (lambda: env.rollout_grid_learn(4), env.get_grid_q,
                 lambda: env.set_grid_q(torch.zeros((N, 4, 5, 4), dtype=torch.float32, device=env.device))):
        with pytest.raises(capi.MdppError, match="no learner"):
            call()
    assert env.grid_learn_kernel_name(4) == "" and not env.status().any()
    env.close()


def test_parameter_range_errors_change_nothing():
    from mdp_playground_amd import _capi as capi
    case, algo = "g34_dense", "q_learning"
    a, b = _mk(case, "philox"), _mk(case, "philox")
    for env in (a, b):
        _set(env, case, algo)
    for bad in (dict(alpha=0.0), dict(alpha=1.5), dict(gamma=-0.1), dict(epsilon=float("nan")), dict(alpha=np.full(N - 1, 0.5, np.float32)),
                dict(epsilon=np.where(np.arange(N) == 7, 1.25, 0.5).astype(np.float32))):
        with pytest.raises(ValueError):
            a.set_grid_learner_rates(**bad)
        with pytest.raises(ValueError):
            a.set_grid_learner(algo, **dict(dict(alpha=0.5, gamma=0.9, epsilon=0.1), **bad))
    with pytest.raises(ValueError):
        a.set_grid_learner("double_q", alpha=0.5, gamma=0.9, epsilon=0.1)
    # the library's own checks: one bad element refuses the whole call, a good array given beside it included
    good, bad = np.full(N, 0.25, np.float32), np.full(N, 0.5, np.float32)
    bad[N - 1] = np.nan
    lib, stream = a._lib, a._stream()
    for args in ((bad, None, None), (good, bad, None), (good, good, np.where(np.arange(N) == 3, -0.5, 0.5).astype(np.float32)),
                 (np.zeros(N, np.float32), None, None)):
        assert lib.mdpp_set_grid_learner_params(a._h, *(capi.nptr(x) for x in args), stream) == -1
        assert b"need every alpha" in lib.mdpp_last_error(a._h)
        assert lib.mdpp_set_grid_learner(a._h, 0, 4, C.c_uint64(9), *(capi.nptr(good if x is None else x) for x in args), None, stream) == -1
    assert lib.mdpp_set_grid_learner(a._h, 2, 4, C.c_uint64(9), capi.nptr(good), capi.nptr(good), capi.nptr(good), None, stream) == -1
    assert lib.mdpp_set_grid_learner(a._h, 0, 6, C.c_uint64(9), capi.nptr(good), capi.nptr(good), capi.nptr(good), None, stream) == -1
    for launch in range(2):
        _assert_same_outputs(a.rollout_grid_learn(K), b.rollout_grid_learn(K), launch)
    _assert_same_q(a, b, "range errors")
    a.close(); b.close()
