"""Closed-loop continuous rollouts under a linear policy WITH MEMORY (set_linear_policy(theta, history=2); include/mdpp.h "Linear
policies with memory").

Every case of tests/linear_history_cases.py, on numpy and Philox streams, two launches in a row, is held to four things:
  the twin         rollout(actions) on an identically built handle, fed the actions the closed launch returned, gives the same
                   observations, rewards and flags bit for bit and leaves the same state record, streams, status words and step
                   counter;
  the restatement  the actions equal tests/linear_history_ref.py -- the act on o and p, p by the memory rule followed from the
                   launch's own flags -- bit for bit, for every (k, i);
  the memory       get_linear_memory() after each launch is the restatement's, bit for bit;
  the form         the kernel's name, HIST=2 and its PLDS value.
N = 320 is one full and one partial workgroup, and every lane of five waves is compared.  The conditions that keep a pass
honest (tests/test_linear_history_cases_host.py settles them on the CPU) are asserted on what ran.  No tolerance anywhere."""
import numpy as np
import pytest
import torch

import graph_replay_util as gr
import linear_history_cases as hc
import linear_history_ref as href
import linear_policy_ref as ref
from test_gpu_linear_rollout import _mk, _same, _same_handles

pytestmark = pytest.mark.gpu
F32 = np.float32


def _start(a, b, name=None):
    """both handles reset (and, for a ``near`` case, given the same placed state); the observation every env shows"""
    oa, _ = a.reset()
    ob, _ = b.reset()
    _same(oa, ob, "reset")
    obs0 = oa.cpu().numpy().copy()
    if name is not None and hc.CASES[name]["near"]:
        st = hc.near_state(name, a.get_augmented_state(), a.mdps[0])
        a.set_augmented_state(st)
        b.set_augmented_state(st)
        obs0 = st["curr_state"].copy()
    return obs0


def _steps(env):
    return env.get_augmented_state()["total_transitions_episode"].astype(np.int64)


def _launch_and_check(a, b, theta, carry, obs0, K, what, mode="same_step"):
    """one closed launch on a, its twin on b, the restatement of the actions and of the memory; returns the twin's outputs as
    numpy, the actions, what the two passes read, and the carry after the launch"""
    assert np.array_equal(_steps(a), carry["steps"]), (what, "step counts before the launch")
    obs, rew, term, trunc, act = a.rollout_linear(K)
    tw = b.rollout(act)
    for j, (x, y) in enumerate(zip((obs, rew, term, trunc), tw)):
        _same(x, y, (what, "twin output", j))
    o, ac, te, tr = obs.cpu().numpy(), act.cpu().numpy(), tw[2].cpu().numpy(), tw[3].cpu().numpy()
    want, p, first, after = href.launch(theta, carry, obs0, o, te, tr, mode, a.mdps[0].action_space_max)
    _same(ac, want, (what, "actions against the restatement"))
    _same(a.get_linear_memory(), after["mem"], (what, "memory after the launch"))
    seen = np.concatenate([np.asarray(obs0, F32)[None], o[:-1]], axis=0)
    return (ac, o, te, tr, seen, p, first), after


def _name_ok(env, K, plds, kernel="k_continuous_linear_rollout", **kw):
    name = env.linear_kernel_name(K, **kw)
    assert name.startswith(kernel + "<") and name.endswith(",HIST=2>"), name
    assert ("PHILOX=%d" % (env.rng == "philox")) in name, name
    assert "PLDS=0" in name or "PLDS=1" in name, name
    if plds is not None:
        assert ("PLDS=%d" % plds) in name, name
    return name


@pytest.mark.parametrize("rng", hc.RNGS)
@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_case_against_twin_restatement_and_memory(name, rng):
    c = hc.CASES[name]
    a, b = _mk(c["config"], c["kw"], rng, opts=c["opts"]), _mk(c["config"], c["kw"], rng, opts=c["opts"])
    try:
        theta = hc.theta_of(name)
        obs0 = _start(a, b, name)
        a.set_linear_policy(theta, history=2)
        assert a.linear_policy_history == 2 and tuple(a.get_linear_policy().shape) == theta.shape
        _same(a.get_linear_policy(), theta, "get_linear_policy")
        _same(a.get_linear_memory(), obs0, "the memory of a policy just set is the state")
        kname = _name_ok(a, hc.K, c["plds"])
        noise = any(c["config"].get(k) is not None for k in ("transition_noise", "reward_noise"))
        assert ("NOISE=%d" % noise) in kname, kname
        carry, launches = href.new_carry(obs0), []
        for launch in range(hc.LAUNCHES):
            out, carry = _launch_and_check(a, b, theta, carry, obs0, hc.K, (name, rng, launch), hc.mode_of(name))
            launches.append(out)
            obs0 = out[1][-1]
            _same_handles(a, b, (name, rng, launch))
        fig = hc.conditions(name, theta, launches)
        print(name, rng, kname, fig)
        hc.assert_conditions(name, fig)
        assert not (a.status() & 1).any()
    finally:
        a.close(); b.close()


def test_summary_form_against_the_full_output_twin():
    name = "d3_order2_rel20_box"
    c = hc.CASES[name]
    a, b = _mk(c["config"], c["kw"], "philox"), _mk(c["config"], c["kw"], "philox")
    try:
        theta = hc.theta_of(name)
        _start(a, b)
        a.set_linear_policy(theta, history=2)
        b.set_linear_policy(theta, history=2)
        _name_ok(a, hc.K, 1, kernel="k_continuous_linear_summary", summary=True)
        sm, want = a.episode_summary(), ref.new_summary(hc.N)
        for launch in range(hc.LAUNCHES):
            a.rollout_linear(hc.K, summary=sm)
            _, rew, term, trunc, _ = b.rollout_linear(hc.K)
            want, _ = ref.summarise(want, rew.cpu().numpy(), term.cpu().numpy(), trunc.cpu().numpy())
            _same_handles(a, b, ("summary", launch))
            _same(a.get_linear_memory(), b.get_linear_memory(), ("summary memory", launch))
        for k in ("ret", "len", "episodes", "return_sum", "length_sum"):
            _same(getattr(sm, k), want[k], ("summary", k))
        assert want["episodes"].sum() > 0
    finally:
        a.close(); b.close()


def test_shared_policy_equals_the_same_policy_broadcast_per_env():
    name = "d4_delay3_every2"
    c = hc.CASES[name]
    a, b = _mk(c["config"], c["kw"]), _mk(c["config"], c["kw"])
    try:
        th = hc.theta_of(name)[3]
        _start(a, b)
        a.set_linear_policy(th, history=2)
        b.set_linear_policy(np.ascontiguousarray(np.broadcast_to(th, (hc.N,) + th.shape)), history=2)
        assert a.get_linear_policy().shape == th.shape and b.get_linear_policy().shape == (hc.N,) + th.shape
        assert a.linear_kernel_name(hc.K) == b.linear_kernel_name(hc.K)
        for launch in range(2):
            ra, rb = a.rollout_linear(hc.K), b.rollout_linear(hc.K)
            for j, (x, y) in enumerate(zip(ra, rb)):
                _same(x, y, ("shared", launch, j))
            _same(a.get_linear_memory(), b.get_linear_memory(), ("shared memory", launch))
        _same_handles(a, b, "shared")
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("n", (1, 63, 257))
def test_small_and_ragged_env_counts(n):
    name = "d2_order2"
    c = hc.CASES[name]
    for rng in hc.RNGS:
        a, b = _mk(c["config"], c["kw"], rng, n=n), _mk(c["config"], c["kw"], rng, n=n)
        try:
            theta = hc.theta_of(name)[:n]
            obs0 = _start(a, b)
            a.set_linear_policy(theta, history=2)
            carry = href.new_carry(obs0)
            for K in (1, 7, 1):
                out, carry = _launch_and_check(a, b, theta, carry, obs0, K, (n, rng, K))
                obs0 = out[1][-1]
            _same_handles(a, b, (n, rng))
        finally:
            a.close(); b.close()


def test_set_linear_memory_then_one_step():
    name = "d3_order2_rel20_box"
    c = hc.CASES[name]
    a, b = _mk(c["config"], c["kw"]), _mk(c["config"], c["kw"])
    try:
        theta = hc.theta_of(name)
        obs0 = _start(a, b)
        a.set_linear_policy(theta, history=2)
        carry = href.new_carry(obs0)
        out, carry = _launch_and_check(a, b, theta, carry, obs0, 3, "before")      # (the step counts are no longer 0)
        obs0 = out[1][-1]
        p = np.random.default_rng(8).uniform(-5, 5, (hc.N, 3)).astype(F32)
        a.set_linear_memory(p)
        _same(a.get_linear_memory(), p, "set_linear_memory round trip")
        carry["mem"] = p.copy()
        out, carry = _launch_and_check(a, b, theta, carry, obs0, 1, "one step on a memory that was set")
        used = ~out[6][0]
        assert used.sum() > hc.N // 2 and np.array_equal(out[5][0][used], p[used])
        a.set_linear_memory(torch.from_numpy(p).to(a.device))
        for bad in (p.astype(np.float64), p[:5], p[:, :2], p.T):
            with pytest.raises(ValueError):
                a.set_linear_memory(bad)
    finally:
        a.close(); b.close()


def test_masked_reset_between_launches_needs_nothing():
    name = "d2_order2"
    c = hc.CASES[name]
    a, b = _mk(c["config"], c["kw"], "philox"), _mk(c["config"], c["kw"], "philox")
    try:
        theta = hc.theta_of(name)
        obs0 = _start(a, b)
        a.set_linear_policy(theta, history=2)
        carry = href.new_carry(obs0)
        out, carry = _launch_and_check(a, b, theta, carry, obs0, 5, "before the reset")
        mask = np.arange(hc.N) % 3 == 0
        oa, _ = a.reset(mask=torch.as_tensor(mask, device=a.device))
        ob, _ = b.reset(mask=torch.as_tensor(mask, device=b.device))
        _same(oa, ob, "masked reset")
        obs0 = oa.cpu().numpy().copy()
        steps = _steps(a)
        assert (steps[mask] == 0).all() and (steps[~mask] > 0).any()
        carry["steps"] = steps                       # the memory is left alone: the count of 0 makes p = o
        _same(a.get_linear_memory(), carry["mem"], "the reset does not touch the memory")
        out, carry = _launch_and_check(a, b, theta, carry, obs0, 5, "after the reset")
        assert out[6][0][mask].all() and np.array_equal(out[5][0][mask], obs0[mask])
        _same_handles(a, b, "masked reset")
    finally:
        a.close(); b.close()


def test_set_state_drops_the_memory():
    name = "d3_order2_rel20_box"
    c = hc.CASES[name]
    a, b = _mk(c["config"], c["kw"]), _mk(c["config"], c["kw"])
    try:
        theta = hc.theta_of(name)
        obs0 = _start(a, b)
        a.set_linear_policy(theta, history=2)
        carry = href.new_carry(obs0)
        out, carry = _launch_and_check(a, b, theta, carry, obs0, 4, "before set_state")
        st = a.get_augmented_state()
        assert not np.array_equal(carry["mem"], st["curr_state"])
        st["curr_state"] = (st["curr_state"] * F32(0.5)).astype(F32)
        st["state_derivatives"][:, 0, :] = st["curr_state"]
        a.set_augmented_state(st)
        b.set_augmented_state(st)
        _same(a.get_linear_memory(), st["curr_state"], "set_state: the memory is the state set")
        carry = dict(mem=st["curr_state"].copy(), steps=_steps(a), pending=np.zeros(hc.N, bool))
        assert (carry["steps"] > 0).any()
        _launch_and_check(a, b, theta, carry, st["curr_state"], 4, "after set_state")
        _same_handles(a, b, "set_state")
    finally:
        a.close(); b.close()


def test_history_1_after_history_2_is_todays_launch_bit_for_bit_and_back():
    name = "d4_delay3_every2"
    c = hc.CASES[name]
    a, b, f = (_mk(c["config"], c["kw"], "philox") for _ in range(3))
    try:
        theta = hc.theta_of(name)
        th1 = hc.without_v(theta)
        obs0 = _start(a, b)
        f.reset()
        a.set_linear_policy(theta, history=2)
        carry = href.new_carry(obs0)
        out, carry = _launch_and_check(a, b, theta, carry, obs0, 6, "history 2")
        f.rollout(torch.from_numpy(out[0]).to(f.device))
        # history 1 on the same handle against a handle that never had a memory
        a.set_linear_policy(th1)
        f.set_linear_policy(th1)
        assert a.linear_policy_history == 1 and tuple(a.get_linear_policy().shape) == th1.shape
        assert a.linear_kernel_name(6) == f.linear_kernel_name(6) and "HIST" not in a.linear_kernel_name(6)
        assert a.linear_kernel_name(6).startswith("k_continuous_linear_rollout<D=4,ORDER=2,PHILOX=1,NOISE=0,PLDS=")
        ra, rf = a.rollout_linear(6), f.rollout_linear(6)
        for j, (x, y) in enumerate(zip(ra, rf)):
            _same(x, y, ("history 1 against a fresh handle", j))
        b.rollout(ra[4])
        _same_handles(a, f, "history 1")
        from mdp_playground_amd._capi import MdppError
        with pytest.raises(MdppError, match="no memory"):
            a.get_linear_memory()
        # ... and back: the memory is the state again
        obs0 = ra[0][-1].cpu().numpy()
        a.set_linear_policy(theta, history=2)
        _same(a.get_linear_memory(), obs0, "back to history 2: the memory is the state")
        carry = dict(mem=obs0.copy(), steps=_steps(a), pending=np.zeros(hc.N, bool))
        _launch_and_check(a, b, theta, carry, obs0, 6, "history 2 again")
        _same_handles(a, b, "history 2 again")
    finally:
        a.close(); b.close(); f.close()


def test_v_zero_gives_the_actions_of_the_history_1_policy():
    name = "d12_order1"
    c = hc.CASES[name]
    a, b = _mk(c["config"], c["kw"]), _mk(c["config"], c["kw"])
    try:
        theta = hc.theta_of(name).copy()
        theta[:, :, 12:24] = 0.0
        _start(a, b)
        a.set_linear_policy(theta, history=2)
        b.set_linear_policy(hc.without_v(theta))
        assert a.linear_kernel_name(hc.K).endswith(",HIST=2>") and "HIST" not in b.linear_kernel_name(hc.K)
        ra, rb = a.rollout_linear(hc.K), b.rollout_linear(hc.K)
        for j, (x, y) in enumerate(zip(ra, rb)):
            _same(x, y, ("V = 0", j))
        _same_handles(a, b, "V = 0")
    finally:
        a.close(); b.close()


def test_nan_in_v_is_a_bad_action_on_exactly_that_env():
    name = "d2_order2"
    c = hc.CASES[name]
    a, b = _mk(c["config"], c["kw"]), _mk(c["config"], c["kw"])
    try:
        theta = hc.theta_of(name).copy()
        theta[70, 1, 2] = np.nan                       # V[1][0] of env 70
        obs0 = _start(a, b)
        a.set_linear_policy(theta, history=2)
        out, _ = _launch_and_check(a, b, theta, href.new_carry(obs0), obs0, 6, "nan in V")
        ac, o = out[0], out[1]
        assert np.isnan(ac[:, 70, 1]).all() and not np.isnan(np.delete(ac, 70, axis=1)).any()
        assert np.array_equal(o[:, 70], np.broadcast_to(obs0[70], o[:, 70].shape))        # the env stays
        want = np.zeros(hc.N, bool)
        want[70] = True
        for e in (a, b):
            assert np.array_equal((e.status() & 1).astype(bool), want)
        _same_handles(a, b, "nan in V")
    finally:
        a.close(); b.close()


def test_history_outside_1_and_2_raises_value_error():
    name = "d2_order2"
    c = hc.CASES[name]
    a = _mk(c["config"], c["kw"], n=16)
    try:
        th = hc.theta_of(name)[:16]
        for bad in (3, 0, -1, True, 2.5, "2"):
            with pytest.raises(ValueError):
                a.set_linear_policy(th, history=bad)
        with pytest.raises(ValueError):
            a.set_linear_policy(th)                    # [N, D, 2 D + 1] is not a history = 1 policy
        with pytest.raises(ValueError):
            a.set_linear_policy(hc.without_v(th), history=2)
        assert a.linear_policy_history == 0 and a.linear_kernel_name(3) == ""
        # the C entry point itself: an argument error
        import ctypes as C
        t = torch.from_numpy(th).to(a.device)
        assert a._lib.mdpp_set_linear_policy_history(a._h, C.c_void_p(t.data_ptr()), 1, 3, None) == -1
        assert b"history must be 1 or 2" in a._lib.mdpp_last_error(a._h)
    finally:
        a.close()


def test_captured_launch_replays_from_a_graph_against_an_eager_twin():
    """a Philox handle with a delay line in memory; the memory buffer is read and written at replay"""
    name = "d4_delay3_every2"
    c = hc.CASES[name]
    a, b = _mk(c["config"], c["kw"], "philox"), _mk(c["config"], c["kw"], "philox")
    try:
        _start(a, b)
        theta = hc.theta_of(name)
        a.set_linear_policy(theta, history=2)
        b.set_linear_policy(theta, history=2)
        K = hc.K
        out_a, out_b = a.alloc_rollout_linear(K), b.alloc_rollout_linear(K)
        a.rollout_linear(K, out_a)           # (one eager launch of the same form before the capture)
        b.rollout_linear(K, out_b)
        torch.cuda.synchronize()
        g = gr.capture(a, lambda: a.rollout_linear(K, out_a), K)
        for rep, between in enumerate((1, 2, 3)):
            g.replay()
            b.rollout_linear(K, out_b)
            torch.cuda.synchronize()
            for j, (x, y) in enumerate(zip(out_a, out_b)):
                _same(x, y, ("replay", rep, j))
            _same(a.get_linear_memory(), b.get_linear_memory(), ("replay memory", rep))
            ra, rb = a.rollout_linear(between), b.rollout_linear(between)
            for j, (x, y) in enumerate(zip(ra, rb)):
                _same(x, y, ("between", rep, j))
        _same_handles(a, b, "graph")
        assert not a.status().any()
    finally:
        a.close(); b.close()
