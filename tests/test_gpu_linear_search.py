"""Linear policy search inside the launch (rollout_linear(K, search=); include/mdpp.h "Linear policy search").

Every case of tests/linear_search_cases.py, on numpy and Philox streams, three launches in a row, is held after EVERY launch,
bit for bit, to:
  the twin         rollout(actions) on an identically built handle, fed the actions the search launch returned, gives the same
                   observations, rewards and flags and leaves the same state record, streams, status words and step counter;
  the restatement  every action, the search's eight arrays and get_linear_policy() (the candidate) equal
                   tests/linear_search_ref.py run on the launch's own observations, rewards and flags;
  the form         the kernel's name and its PLDS value.
N = 320 is one full and one partial workgroup; every lane of five waves is compared.  The conditions that keep a pass honest
(tests/test_linear_search_cases_host.py settles them on the CPU) are asserted again on what ran.  No tolerance anywhere."""
import numpy as np
import pytest
import torch

import graph_replay_util as gr
import linear_policy_ref as ref
import linear_search_cases as sc
import linear_search_ref as lsr
from test_gpu_linear_rollout import REFUSALS, _mk, _same, _same_handles

pytestmark = pytest.mark.gpu
F32 = np.float32


def _pair(name, rng, n=sc.N):
    c = sc.CASES[name]
    return _mk(c["config"], c["kw"], rng, n=n, opts=c["opts"]), _mk(c["config"], c["kw"], rng, n=n, opts=c["opts"])


def _start(name, *envs):
    """every handle reset (and, for a ``near`` case, given the same placed state); the observation every env shows"""
    outs = [e.reset()[0] for e in envs]
    for o in outs[1:]:
        _same(outs[0], o, "reset")
    obs0 = outs[0].cpu().numpy().copy()
    if sc.CASES[name]["near"]:
        st = sc.near_state(name, envs[0].get_augmented_state(), envs[0].mdps[0])
        for e in envs:
            e.set_augmented_state(st)
        obs0 = st["curr_state"].copy()
    return obs0


def _search(env, name, n=sc.N, **over):
    c = sc.CASES[name]
    kw = dict(seed=sc.SEED, episodes_per_trial=c["T"], sigma_up=c["up"], sigma_down=c["down"], sigma_max=c["sigma_max"])
    kw.update(over)
    return env.linear_search(sc.sigma_of(name, n), **kw)


def _rule(name, **over):
    c = sc.CASES[name]
    kw = dict(seed=sc.SEED, env0=sc.OFF, T=c["T"], up=c["up"], down=c["down"], sigma_max=c["sigma_max"],
              next_step=c["kw"].get("autoreset") == "next_step")
    kw.update(over)
    return kw


def _same_search(env, search, want, what):
    for k in lsr.ARRAYS:
        _same(getattr(search, k), want[k], (what, k))
    _same(env.get_linear_policy(), want["cand"], (what, "candidate"))


def _launch_and_check(a, b, search, state, obs0, pend, K, rule, what, handles=True):
    """one search launch on a, its twin on b, the restatement; returns (obs, ended, the state and pending after the launch)"""
    obs, rew, term, trunc, act = a.rollout_linear(K, search=search)
    tw = b.rollout(act)
    for j, (x, y) in enumerate(zip((obs, rew, term, trunc), tw)):
        _same(x, y, (what, "twin output", j))
    o = obs.cpu().numpy()
    want_act, state, pend, ended = lsr.run_launch(state, obs0, o, tw[1].cpu().numpy(), tw[2].cpu().numpy(), tw[3].cpu().numpy(),
                                                  amax=a.mdps[0].action_space_max, pending=pend, **rule)
    _same(act, want_act, (what, "actions against the restatement"))
    _same_search(a, search, state, what)
    if handles:                # (status() clears the words it returns: a caller that looks at them itself compares the handles after)
        _same_handles(a, b, what)
    return o, ended, state, pend


def _name_ok(env, K, plds, summary=False):
    name = env.linear_kernel_name(K, summary=summary, search=True)
    assert name.startswith("k_continuous_search_summary<" if summary else "k_continuous_search_rollout<"), name
    assert ("PHILOX=%d" % (env.rng == "philox")) in name, name
    assert "PLDS=0" in name or "PLDS=1" in name, name
    if plds is not None:
        assert ("PLDS=%d" % plds) in name, name
    # the placement rule is the linear kernels': the same template arguments
    assert name.split("<")[1] == env.linear_kernel_name(K, summary=summary).split("<")[1]
    return name


@pytest.mark.parametrize("rng", sc.RNGS)
@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_case_against_twin_and_restatement(name, rng):
    c = sc.CASES[name]
    a, b = _pair(name, rng)
    try:
        theta = sc.theta_of(name)
        obs0 = _start(name, a, b)
        a.set_linear_policy(theta)
        kname = _name_ok(a, sc.K, c["plds"])
        noise = any(c["config"].get(k) is not None for k in ("transition_noise", "reward_noise"))
        assert ("NOISE=%d" % noise) in kname, kname
        search = _search(a, name)
        state, pend, ended = lsr.new_state(theta, sc.sigma_of(name)), None, []
        _same_search(a, search, state, (name, rng, "start"))
        for launch in range(sc.LAUNCHES):
            o, e, state, pend = _launch_and_check(a, b, search, state, obs0, pend, sc.K, _rule(name), (name, rng, launch))
            ended.append(e)
            obs0 = o[-1]
        fig = sc.figures(np.concatenate(ended), state["trial"], state["accepted"])
        print(name, rng, kname, fig)
        sc.assert_figures(name, fig)
        assert not np.array_equal(state["cand"], theta)
        _same(search.best_theta(), np.ascontiguousarray(state["best"].T).reshape(theta.shape), "best_theta")
        if c["sigma"] == "zeros3":        # sigma 0: the candidate stays the start policy, trial after trial
            assert np.array_equal(state["cand"][::3], theta[::3]) and (state["trial"][::3] >= 2).all()
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("name", ("c_d2_n0", "autoreset_next_step", "cfg5"))
def test_three_launches_of_37_equal_one_launch_of_111(name):
    for rng in sc.RNGS:
        a, b = _pair(name, rng)
        try:
            theta = sc.theta_of(name)
            _start(name, a, b)
            for e in (a, b):
                e.set_linear_policy(theta)
            sa, sb = _search(a, name), _search(b, name)
            parts = [a.rollout_linear(sc.K, search=sa) for _ in range(3)]
            whole = b.rollout_linear(3 * sc.K, search=sb)
            for j in range(5):
                _same(torch.cat([p[j] for p in parts]), whole[j], (name, rng, "output", j))
            for x, y, k in zip(sa.tensors(), sb.tensors(), lsr.ARRAYS):
                _same(x, y, (name, rng, k))
            _same(a.get_linear_policy(), b.get_linear_policy(), (name, rng, "candidate"))
            _same_handles(a, b, (name, rng))
            assert int(sa.trial.min()) >= 2
        finally:
            a.close(); b.close()


@pytest.mark.parametrize("n", (1, 63, 257))
def test_small_and_ragged_env_counts(n):
    name = "c_d2_n0"
    for rng in sc.RNGS:
        a, b = _pair(name, rng, n=n)
        try:
            theta = sc.theta_of(name)[:n]
            obs0 = _start(name, a, b)
            a.set_linear_policy(theta)
            search = _search(a, name, n)
            state, pend = lsr.new_state(theta, sc.sigma_of(name, n)), None
            for K in (1, 7, 1, 7, 7):
                o, _, state, pend = _launch_and_check(a, b, search, state, obs0, pend, K, _rule(name), (n, rng, K))
                obs0 = o[-1]
            assert (state["trial"] >= 1).all()
        finally:
            a.close(); b.close()


def test_a_trial_longer_than_the_launch_carries_over():
    name = "c_d2_n0"
    a, b = _pair(name, "numpy")
    try:
        theta = sc.theta_of(name)
        obs0 = _start(name, a, b)
        a.set_linear_policy(theta)
        search = _search(a, name, episodes_per_trial=1000)
        state, pend = lsr.new_state(theta, sc.sigma_of(name)), None
        for launch in range(2):
            o, ended, state, pend = _launch_and_check(a, b, search, state, obs0, pend, sc.K, _rule(name, T=1000), ("long trial", launch))
            obs0 = o[-1]
            assert not ended.any()
            _same(a.get_linear_policy(), theta, "the candidate is unchanged")
        assert (state["eps"] >= 10).all() and (state["acc"] != 0).all() and not state["trial"].any() and not state["accepted"].any()
        assert np.isneginf(state["score"]).all()
    finally:
        a.close(); b.close()


def test_nan_bias_is_a_bad_action_and_a_rejected_trial_0():
    name = "c_d2_n0"
    a, b = _pair(name, "numpy")
    try:
        theta = sc.theta_of(name).copy()
        theta[70, 1, 2] = np.nan
        obs0 = _start(name, a, b)
        a.set_linear_policy(theta)
        search = _search(a, name)
        state = lsr.new_state(theta, sc.sigma_of(name))
        o, ended, state, _ = _launch_and_check(a, b, search, state, obs0, None, 16, _rule(name), "nan bias", handles=False)
        want = np.zeros(sc.N, bool)
        want[70] = True
        for e in (a, b):
            assert np.array_equal((e.status() & 1).astype(bool), want)
        _same_handles(a, b, "nan bias")
        # the env stays where it is, its episodes are truncated, and (make_denser, no movement, a NaN action penalty) its
        # return is NaN: every trial is rejected, the incumbent stays the start policy and every candidate keeps the NaN
        assert ended[:, 70].sum() == 2 and state["trial"][70] == 2 and state["accepted"][70] == 0 and np.isneginf(state["score"][70])
        assert np.isnan(state["cand"][70, 1, 2]) and np.isnan(state["best"][5, 70])
        assert (np.delete(state["accepted"], 70) >= 1).all()
    finally:
        a.close(); b.close()


def test_state_dict_round_trip_mid_trial():
    name = "d3_order2_rel20_box"
    a, b = _pair(name, "philox")
    try:
        theta = sc.theta_of(name)
        _start(name, a, b)
        for e in (a, b):
            e.set_linear_policy(theta)
        sa, sb = _search(a, name), _search(b, name)
        a.rollout_linear(sc.K, search=sa)
        b.rollout_linear(sc.K, search=sb)
        assert sa.eps.any() and sa.ret.any()                           # mid-trial, mid-episode
        d = sa.state_dict()
        cand = a.get_linear_policy().clone()
        a.set_linear_policy(theta)                                     # the search goes on from a fresh object and a policy set again
        fresh = a.linear_search(1.0, seed=0)
        fresh.load_state_dict(d)
        a.set_linear_policy(cand)
        ra, rb = a.rollout_linear(sc.K, search=fresh), b.rollout_linear(sc.K, search=sb)
        for j, (x, y) in enumerate(zip(ra, rb)):
            _same(x, y, ("state_dict", j))
        for x, y, k in zip(fresh.tensors(), sb.tensors(), lsr.ARRAYS):
            _same(x, y, ("state_dict", k))
        _same(a.get_linear_policy(), b.get_linear_policy(), "state_dict candidate")
        _same_handles(a, b, "state_dict")
        fresh.abandon_episode()
        assert not fresh.ret.any() and fresh.acc.any()
    finally:
        a.close(); b.close()


SUMMARY_CASES = ("c_d2_n0", "c_d2_n0_no_lds", "d3_order2_rel20_box", "d4_delay3_every2_alw", "cfg3", "cfg5", "autoreset_next_step",
                 "max5_autoreset_disabled")


@pytest.mark.parametrize("rng", sc.RNGS)
@pytest.mark.parametrize("name", SUMMARY_CASES)
def test_summary_form_against_the_full_output_twin(name, rng):
    c = sc.CASES[name]
    a, b = _pair(name, rng)
    try:
        theta = sc.theta_of(name)
        _start(name, a, b)
        for e in (a, b):
            e.set_linear_policy(theta)
        kname = _name_ok(a, sc.K, c["plds"], summary=True)
        assert kname.split("<")[1] == _name_ok(b, sc.K, c["plds"]).split("<")[1]
        sa, sb = _search(a, name), _search(b, name)
        s = a.episode_summary()
        want, pend = ref.new_summary(sc.N), None
        for launch in range(sc.LAUNCHES):
            assert a.rollout_linear(sc.K, summary=s, search=sa) is s
            _, rew, term, trunc, _ = b.rollout_linear(sc.K, search=sb)
            want, pend = ref.summarise(want, rew.cpu().numpy(), term.cpu().numpy(), trunc.cpu().numpy(),
                                       next_step=c["kw"].get("autoreset") == "next_step", pending=pend)
            for t, k in zip(s.tensors(), ("ret", "len", "episodes", "return_sum", "length_sum")):
                _same(t, want[k], (name, rng, launch, k))
            for x, y, k in zip(sa.tensors(), sb.tensors(), lsr.ARRAYS):
                _same(x, y, (name, rng, launch, k))
            _same(a.get_linear_policy(), b.get_linear_policy(), (name, rng, launch, "candidate"))
            _same_handles(a, b, (name, rng, launch))
        assert int(sa.trial.min()) >= 2 and int(want["episodes"].sum()) > 0
    finally:
        a.close(); b.close()


def test_explicit_reset_leaves_the_search_alone():
    name = "c_d2_n0"
    a, b = _pair(name, "numpy")
    try:
        _start(name, a, b)
        a.set_linear_policy(sc.theta_of(name))
        search = _search(a, name)
        a.rollout_linear(5, search=search)
        before = [t.clone() for t in search.tensors()]
        cand = a.get_linear_policy().clone()
        a.reset()
        for x, y, k in zip(search.tensors(), before, lsr.ARRAYS):
            _same(x, y, ("reset", k))
        _same(a.get_linear_policy(), cand, "reset candidate")
        mask = torch.zeros(sc.N, dtype=torch.bool)
        mask[5] = True
        search.abandon_episode(mask)
        assert search.ret[5] == 0 and np.array_equal(np.delete(search.ret.cpu().numpy(), 5), np.delete(before[4].cpu().numpy(), 5))
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_refusals_of_the_linear_kernels_with_their_reasons(what):
    config, kw, D, reason = REFUSALS[what]
    from mdp_playground_amd.linear_search import LinearSearch
    env = _mk(config, kw, n=16)
    try:
        with pytest.raises(NotImplementedError, match=reason):
            env.linear_search(0.1, seed=1)
        search = LinearSearch(torch.zeros((16, D, D + 1), dtype=torch.float32, device=env.device), 0.1, seed=1)
        with pytest.raises(NotImplementedError, match=reason):
            env.rollout_linear(3, search=search)
        assert env.linear_kernel_name(3, search=True) == ""
    finally:
        env.close()


def test_refusals_of_the_search_itself():
    import ctypes as C
    from mdp_playground_amd import _capi as capi
    from mdp_playground_amd._capi import MdppError
    name = "c_d2_n0"
    c = sc.CASES[name]
    env = _mk(c["config"], c["kw"], n=64)
    try:
        env.reset()
        theta = sc.theta_of(name)[:64]
        with pytest.raises(MdppError, match="no linear policy set"):
            env.linear_search(0.1, seed=1)
        env.set_linear_policy(theta[0])                                 # a shared policy
        with pytest.raises(NotImplementedError, match="the search needs one parameter set per env"):
            env.linear_search(0.1, seed=1)
        assert env.linear_kernel_name(3, search=True) == ""
        env.set_linear_policy(theta)
        search = env.linear_search(0.1, seed=1)
        env.set_linear_policy(theta[0])
        with pytest.raises(NotImplementedError, match="the search needs one parameter set per env"):
            env.rollout_linear(3, search=search)
        with pytest.raises(NotImplementedError, match="the search needs one parameter set per env"):
            env.rollout_linear(3, summary=env.episode_summary(), search=search)
        env.set_linear_policy(None)
        with pytest.raises(MdppError, match="no linear policy set"):
            env.rollout_linear(3, search=search)
        env.set_linear_policy(theta)
        for bad in (dict(sigma=-1.0), dict(sigma=np.nan), dict(sigma=np.zeros(64, np.float64)), dict(sigma=np.zeros(63, F32)),
                    dict(episodes_per_trial=0), dict(sigma_up=-1.0), dict(sigma_max=np.nan)):
            kw = dict(dict(sigma=0.1, seed=1), **bad)
            with pytest.raises(ValueError):
                env.linear_search(kw.pop("sigma"), **kw)
        with pytest.raises(ValueError):
            env.rollout_linear(3, search=object())
        search.trial = search.trial.to(torch.int64)
        with pytest.raises(ValueError):
            env.rollout_linear(3, search=search)
        # the C entry point's own checks (the Python object makes them first): MDPP_EINVAL, nothing launched
        search = env.linear_search(0.1, seed=1)
        out = env.alloc_rollout_linear(3)
        ptr = [C.c_void_p(t.data_ptr()) for t in (out[4], out[0], out[1], out[2], out[3])]
        t0 = gr.tick(env)
        for field, value in (("episodes_per_trial", 0), ("best", None), ("accepted", None), ("sigma_up", float("inf")),
                             ("sigma_down", -1.0), ("sigma_max", float("nan")), ("sigma_max", -0.5)):
            s = search.c_struct()
            setattr(s, field, value)
            assert env._lib.mdpp_step_n_linear_search(env._h, 3, C.byref(s), *ptr, None) == -1, field
            sm = [C.c_void_p(t.data_ptr()) for t in env.episode_summary().tensors()]
            assert env._lib.mdpp_step_n_linear_search_summary(env._h, 3, C.byref(s), *sm, None) == -1, field
        assert env._lib.mdpp_step_n_linear_search(env._h, 3, None, *ptr, None) == -1
        assert env._lib.mdpp_step_n_linear_search(env._h, 0, C.byref(search.c_struct()), *ptr, None) == -1
        assert gr.tick(env) == t0
    finally:
        env.close()


def test_captured_launch_replays_from_a_graph_against_an_eager_twin():
    """a Philox handle with a delay line in memory; the search's arrays and the candidate are read and written at replay"""
    name = "d4_delay3_every2_alw"
    a, b = _pair(name, "philox")
    try:
        _start(name, a, b)
        theta = sc.theta_of(name)
        for e in (a, b):
            e.set_linear_policy(theta)
        sa, sb = _search(a, name), _search(b, name)
        K = sc.K
        out_a, out_b = a.alloc_rollout_linear(K), b.alloc_rollout_linear(K)
        a.rollout_linear(K, out_a, search=sa)       # (one eager launch of the same form before the capture)
        b.rollout_linear(K, out_b, search=sb)
        torch.cuda.synchronize()
        g = gr.capture(a, lambda: a.rollout_linear(K, out_a, search=sa), K)
        for rep, between in enumerate((1, 2, 3)):
            g.replay()
            b.rollout_linear(K, out_b, search=sb)
            torch.cuda.synchronize()
            for j, (x, y) in enumerate(zip(out_a, out_b)):
                _same(x, y, ("replay", rep, j))
            ra, rb = a.rollout_linear(between, search=sa), b.rollout_linear(between, search=sb)
            for j, (x, y) in enumerate(zip(ra, rb)):
                _same(x, y, ("between", rep, j))
            for x, y, k in zip(sa.tensors(), sb.tensors(), lsr.ARRAYS):
                _same(x, y, ("replay", rep, k))
            _same(a.get_linear_policy(), b.get_linear_policy(), ("replay", rep, "candidate"))
        _same_handles(a, b, "graph")
        assert int(sa.trial.min()) >= 20 and not a.status().any()
    finally:
        a.close(); b.close()
