"""Closed-loop continuous rollouts under a linear policy per env (rollout_linear; include/mdpp.h "Linear policies").

Every case of tests/linear_policy_cases.py, on numpy and Philox streams, two launches in a row, is held to three things:
  the twin         rollout(actions) on an identically built handle, fed the actions the closed launch returned, gives the same
                   observations, rewards and flags bit for bit and leaves the same state record, streams, status words and step
                   counter;
  the restatement  the actions equal tests/linear_policy_ref.py on the observations, bit for bit, for every (k, i);
  the form         the kernel's name and its PLDS value.
N = 320 is one full and one partial workgroup, and every lane of five waves is compared.  The conditions that keep a pass
honest (clipped actions, terminations, truncations, walls; tests/test_linear_policy_cases_host.py settles them on the CPU) are
asserted on the twin's outputs.  No tolerance anywhere."""
import warnings

import numpy as np
import pytest
import torch

import graph_replay_util as gr
import linear_policy_cases as lc
import linear_policy_ref as ref

pytestmark = pytest.mark.gpu
F32 = np.float32


def _mk(config, kw=None, rng="numpy", n=lc.N, opts=()):
    from mdp_playground_amd import RLToyVectorEnv
    kw = dict(kw or {})
    if rng == "philox":
        kw = dict(lc.PHILOX, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = RLToyVectorEnv(num_envs=n, env_id_offset=lc.OFF, **kw, **config)
    if opts:
        env.set_kernel_options(*opts)
    return env


def _bits(x):
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    if x.dtype == np.float32:
        return x.view(np.uint32)
    if x.dtype == np.float64:
        return x.view(np.uint64)
    return x.astype(np.uint8) if x.dtype == bool else x


def _same(x, y, what):
    x, y = _bits(x), _bits(y)
    assert x.shape == y.shape and x.dtype == y.dtype, what
    if not np.array_equal(x, y):
        raise AssertionError((what, np.argwhere(x != y)[:5].tolist()))


def _same_handles(a, b, what):
    sa, sb = a.get_augmented_state(), b.get_augmented_state()
    assert sa.keys() == sb.keys()
    for k in sa:
        if isinstance(sa[k], np.ndarray):
            _same(sa[k], sb[k], (what, k))
        else:
            assert sa[k] == sb[k], (what, k)
    if a.rng == "numpy":
        from mdp_playground_amd import _capi as capi
        for s in (capi.STREAM_ENV, capi.STREAM_SPACE):
            assert np.array_equal(a.get_rng_streams(s), b.get_rng_streams(s)), (what, "stream", s)
    _same(a.status(), b.status(), (what, "status"))
    assert gr.tick(a) == gr.tick(b), what


def _start(a, b, name=None):
    """both handles reset (and, for a ``near`` case, given the same placed state); the observation every env shows"""
    oa, _ = a.reset()
    ob, _ = b.reset()
    _same(oa, ob, "reset")
    obs0 = oa.cpu().numpy().copy()
    if name is not None and lc.CASES[name]["near"]:
        st = lc.near_state(name, a.get_augmented_state(), a.mdps[0])
        a.set_augmented_state(st)
        b.set_augmented_state(st)
        obs0 = st["curr_state"].copy()
    return obs0


def _launch_and_check(a, b, theta, obs0, K, what):
    """one closed launch on a, its twin on b, the restatement; returns the twin's outputs as numpy and the actions"""
    obs, rew, term, trunc, act = a.rollout_linear(K)
    tw = b.rollout(act)
    for j, (x, y) in enumerate(zip((obs, rew, term, trunc), tw)):
        _same(x, y, (what, "twin output", j))
    o, ac = obs.cpu().numpy(), act.cpu().numpy()
    want = ref.linear_actions(theta, ref.observed(obs0, o), a.mdps[0].action_space_max)
    _same(ac, want, (what, "actions against the restatement"))
    return o, tw[1].cpu().numpy(), tw[2].cpu().numpy(), tw[3].cpu().numpy(), ac


def _name_ok(env, K, plds, summary=False):
    name = env.linear_kernel_name(K, summary=summary)
    assert name.startswith("k_continuous_linear_summary<" if summary else "k_continuous_linear_rollout<"), name
    assert ("PHILOX=%d" % (env.rng == "philox")) in name, name
    assert "PLDS=0" in name or "PLDS=1" in name, name
    if plds is not None:
        assert ("PLDS=%d" % plds) in name, name
    return name


@pytest.mark.parametrize("rng", lc.RNGS)
@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_case_against_twin_and_restatement(name, rng):
    c = lc.CASES[name]
    a, b = _mk(c["config"], c["kw"], rng, opts=c["opts"]), _mk(c["config"], c["kw"], rng, opts=c["opts"])
    try:
        theta = lc.theta_of(name)
        obs0 = _start(a, b, name)
        a.set_linear_policy(theta)
        kname = _name_ok(a, lc.K, c["plds"])
        noise = any(c["config"].get(k) is not None for k in ("transition_noise", "reward_noise"))
        assert ("NOISE=%d" % noise) in kname, kname
        outs = []
        for launch in range(lc.LAUNCHES):
            o, r, te, tr, ac = _launch_and_check(a, b, theta, obs0, lc.K, (name, rng, launch))
            outs.append((o, te, tr, ac))
            obs0 = o[-1]
            _same_handles(a, b, (name, rng, launch))
        o, te, tr, ac = (np.concatenate([x[j] for x in outs]) for j in range(4))
        fig = lc.conditions(name, ac, te, tr, o)
        print(name, rng, kname, fig)
        lc.assert_conditions(name, fig)
        # env 0's parameters on env 1's observations give other actions than env 1 took
        first = outs[0]
        o1 = first[0][:-1, 1]                                       # what env 1 observed at steps 1 .. K - 1 of launch 0
        other = ref.linear_actions(theta[0], o1, a.mdps[0].action_space_max)
        assert not np.array_equal(other, first[3][1:, 1]), name
        assert not (a.status() & 1).any()
    finally:
        a.close(); b.close()


def test_shared_policy_equals_the_same_policy_broadcast_per_env():
    c = lc.CASES["d4_delay3_every2_alw"]
    a, b = _mk(c["config"], c["kw"]), _mk(c["config"], c["kw"])
    try:
        th = lc.theta_of("d4_delay3_every2_alw")[3]
        _start(a, b)
        a.set_linear_policy(th)
        b.set_linear_policy(np.ascontiguousarray(np.broadcast_to(th, (lc.N,) + th.shape)))
        assert a.get_linear_policy().shape == th.shape and b.get_linear_policy().shape == (lc.N,) + th.shape
        assert a.linear_kernel_name(lc.K) == b.linear_kernel_name(lc.K)
        for launch in range(2):
            ra, rb = a.rollout_linear(lc.K), b.rollout_linear(lc.K)
            for j, (x, y) in enumerate(zip(ra, rb)):
                _same(x, y, ("shared", launch, j))
        _same_handles(a, b, "shared")
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("n", (1, 63, 257))
def test_small_and_ragged_env_counts(n):
    c = lc.CASES["c_d2_n0"]
    for rng in lc.RNGS:
        a, b = _mk(c["config"], c["kw"], rng, n=n), _mk(c["config"], c["kw"], rng, n=n)
        try:
            theta = lc.theta_of("c_d2_n0")[:n]
            obs0 = _start(a, b)
            a.set_linear_policy(theta)
            for K in (1, 7, 1):
                obs0 = _launch_and_check(a, b, theta, obs0, K, (n, rng, K))[0][-1]
            _same_handles(a, b, (n, rng))
        finally:
            a.close(); b.close()


def test_set_between_launches_and_get_round_trips():
    c = lc.CASES["d3_order2_rel20_box"]
    a, b = _mk(c["config"], c["kw"]), _mk(c["config"], c["kw"])
    try:
        obs0 = _start(a, b)
        t1, t2 = lc.theta_of("d3_order2_rel20_box"), ref.draw_theta(lc.N, 3, seed=999)
        for th in (t1, t2, t1[7], torch.from_numpy(t2).to(a.device)):
            a.set_linear_policy(th)
            got = a.get_linear_policy()
            want = th if torch.is_tensor(th) else torch.from_numpy(np.ascontiguousarray(th))
            assert got.shape == want.shape
            _same(got, want, "get_linear_policy")
            th_np = want.cpu().numpy()
            obs0 = _launch_and_check(a, b, th_np, obs0, 5, "set between launches")[0][-1]
        _same_handles(a, b, "set between launches")
        a.set_linear_policy(None)
        from mdp_playground_amd._capi import MdppError
        with pytest.raises(MdppError, match="no linear policy set"):
            a.rollout_linear(3)
        assert a.linear_kernel_name(3) == ""
        for bad in (t1.astype(np.float64), t1[:, :2], t1[:5], np.zeros((3, 3), F32), [[1.0]]):
            with pytest.raises(ValueError):
                a.set_linear_policy(bad)
    finally:
        a.close(); b.close()


def test_nan_bias_is_a_bad_action_on_exactly_that_env():
    c = lc.CASES["c_d2_n0"]
    a, b = _mk(c["config"], c["kw"]), _mk(c["config"], c["kw"])
    try:
        theta = lc.theta_of("c_d2_n0").copy()
        theta[70, 1, 2] = np.nan
        obs0 = _start(a, b)
        a.set_linear_policy(theta)
        o, _, _, _, ac = _launch_and_check(a, b, theta, obs0, 6, "nan bias")
        assert np.isnan(ac[:, 70, 1]).all() and not np.isnan(np.delete(ac, 70, axis=1)).any()
        assert np.array_equal(o[:, 70], np.broadcast_to(obs0[70], o[:, 70].shape))        # the env stays
        want = np.zeros(lc.N, bool)
        want[70] = True
        for e in (a, b):
            assert np.array_equal((e.status() & 1).astype(bool), want)
        _same_handles(a, b, "nan bias")
    finally:
        a.close(); b.close()


def test_no_fused_multiply_add_on_the_device():
    """env 0 observes 1 + 2^-12 (through the state setter) under w = 1 + 2^-12, b = -(1 + 2^-11): the product rounds to 1 + 2^-11
    and the action is exactly 0; a fused multiply-add would keep 2^-24."""
    c = lc.CASES["c_d2_n0"]
    a, b = _mk(c["config"], c["kw"], n=64), _mk(c["config"], c["kw"], n=64)
    try:
        _start(a, b)
        w = F32(1 + 2.0 ** -12)
        st = a.get_augmented_state()
        st["curr_state"][0] = (w, 0.0)
        st["state_derivatives"][0] = 0.0
        st["state_derivatives"][0, 0] = (w, 0.0)
        a.set_augmented_state(st)
        b.set_augmented_state(st)
        theta = np.zeros((64, 2, 3), F32)
        theta[0, 0] = (w, 0.0, F32(-(1 + 2.0 ** -11)))
        a.set_linear_policy(theta)
        ac = _launch_and_check(a, b, theta, st["curr_state"], 1, "fma pin")[4]
        assert ac[0, 0].view(np.uint32).tolist() == [0, 0]
        assert float(w) * float(w) + float(theta[0, 0, 2]) == 2.0 ** -24
    finally:
        a.close(); b.close()


_DISC = dict(state_space_type="discrete", action_space_type="discrete", state_space_size=8, action_space_size=8, delay=0,
             sequence_length=1, seed=0)
_GRID = dict(state_space_type="grid", reward_function="move_to_a_point", grid_shape=(8, 8), make_denser=True, target_point=[5, 5], seed=31)
_LINE = dict(state_space_type="continuous", state_space_dim=4, transition_dynamics_order=1, inertia=1, time_unit=1, delay=0,
             sequence_length=10, action_space_max=1, state_space_max=6, reward_function="move_along_a_line", seed=8)
_C2 = dict(lc.C_D2_N0)
REFUSALS = {
    "discrete": (_DISC, {}, 1, "serve continuous envs only"),
    "grid": (_GRID, {}, 2, "serve continuous envs only"),
    "move_along_a_line": (_LINE, {}, 4, "move_along_a_line"),
    "image": (dict(_C2, image_representations=True, image_width=32, image_height=32), {}, 2, "image observations"),
    "episode_stats": (_C2, dict(episode_stats=True), 2, "episode_stats"),
    "d14": (dict(lc.CFG3, state_space_dim=14), {}, 14, "state_space_dim <= 12"),
    "order3": (dict(_C2, transition_dynamics_order=3), {}, 2, "transition_dynamics_order <= 2"),
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_refusals_with_their_reasons(what):
    config, kw, D, reason = REFUSALS[what]
    env = _mk(config, kw, n=16)
    try:
        with pytest.raises(NotImplementedError, match=reason):
            env.set_linear_policy(np.zeros((D, D + 1), F32))
        with pytest.raises(NotImplementedError, match=reason):
            env.rollout_linear(3)
        assert env.linear_kernel_name(3) == ""
    finally:
        env.close()


def test_continuous_handles_keep_refusing_the_tabular_policy():
    c = lc.CASES["c_d2_n0"]
    env = _mk(c["config"], c["kw"], n=16)
    try:
        with pytest.raises(NotImplementedError, match="serve discrete envs only"):
            env.set_policy(np.zeros(4, np.int64))
        with pytest.raises(NotImplementedError, match="serve discrete envs only"):
            env.rollout_policy(3)
    finally:
        env.close()


def test_captured_launch_replays_from_a_graph_against_an_eager_twin():
    """a Philox handle with a delay line in memory: the Philox keys and the ring head come through the device word"""
    name = "d4_delay3_every2_alw"
    c = lc.CASES[name]
    a, b = _mk(c["config"], c["kw"], "philox"), _mk(c["config"], c["kw"], "philox")
    try:
        _start(a, b)
        theta = lc.theta_of(name)
        a.set_linear_policy(theta)
        b.set_linear_policy(theta)
        K = lc.K
        out_a, out_b = a.alloc_rollout_linear(K), b.alloc_rollout_linear(K)
        a.rollout_linear(K, out_a)           # (one eager launch of the same form before the capture)
        b.rollout_linear(K, out_b)
        torch.cuda.synchronize()
        g = gr.capture(a, lambda: a.rollout_linear(K, out_a), K)
        for rep, between in enumerate((1, 2, 3)):
            if rep == 1:                     # the parameter buffer is read at replay
                t2 = ref.draw_theta(lc.N, c["D"], seed=4242)
                a.set_linear_policy(t2)
                b.set_linear_policy(t2)
            g.replay()
            b.rollout_linear(K, out_b)
            torch.cuda.synchronize()
            for j, (x, y) in enumerate(zip(out_a, out_b)):
                _same(x, y, ("replay", rep, j))
            ra, rb = a.rollout_linear(between), b.rollout_linear(between)
            for j, (x, y) in enumerate(zip(ra, rb)):
                _same(x, y, ("between", rep, j))
        _same_handles(a, b, "graph")
        assert not a.status().any()
    finally:
        a.close(); b.close()
