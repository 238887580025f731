"""Linear policy ES inside the launch (rollout_linear(K, es=); include/mdpp.h "Linear policy ES").

Every case of tests/linear_es_cases.py, on numpy and Philox streams, three launches in a row, is held after EVERY launch, bit for
bit, to:
  the twin         rollout(actions) on an identically built handle, fed the actions the ES launch returned, gives the same
                   observations, rewards and flags and leaves the same state record, streams, status words and step counter;
  the restatement  every action, the ES's nine arrays and get_linear_policy() (the candidates) equal tests/linear_es_ref.py run
                   on the launch's own observations, rewards and flags;
  the form         the kernel's name and its PLDS value.
N = 320 is five groups: one full workgroup and one with a single live wave; every lane is compared.  The conditions that keep
a pass honest (tests/test_linear_es_cases_host.py settles them on the CPU) are asserted again on what ran.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

import graph_replay_util as gr
import linear_es_cases as ec
import linear_es_ref as ler
import linear_policy_ref as ref
from test_gpu_linear_rollout import REFUSALS, _mk, _same, _same_handles

pytestmark = pytest.mark.gpu
F32 = np.float32


def _pair(name, rng, n=ec.N):
    c = ec.CASES[name]
    return _mk(c["config"], c["kw"], rng, n=n, opts=c["opts"]), _mk(c["config"], c["kw"], rng, n=n, opts=c["opts"])


def _start(name, *envs):
    """every handle reset (and, for a ``near`` case, given the same placed state); the observation every env shows"""
    outs = [e.reset()[0] for e in envs]
    for o in outs[1:]:
        _same(outs[0], o, "reset")
    obs0 = outs[0].cpu().numpy().copy()
    if ec.CASES[name]["near"]:
        st = ec.near_state(name, envs[0].get_augmented_state(), envs[0].mdps[0])
        for e in envs:
            e.set_augmented_state(st)
        obs0 = st["curr_state"].copy()
    return obs0


def _es(env, name, groups=ec.G, **over):
    """the handle's per-env layout, then the ES (which writes generation 0's candidates over it)"""
    c = ec.CASES[name]
    env.set_linear_policy(ec.theta_of(name, ec.GROUP * groups))
    kw = dict(seed=ec.SEED, episodes_per_member=c["T"], log_generations=ec.ROWS)
    kw.update(over)
    mean = kw.pop("mean", ec.mean_of(name, groups))
    return env.linear_es(mean, kw.pop("sigma", ec.sigma_of(name, groups)), kw.pop("lr", ec.lr_of(name, groups)), **kw)


def _ref_state(name, groups=ec.G, rows=ec.ROWS, mean=None, seed=ec.SEED):
    s = ler.new_state(ec.mean_of(name, groups) if mean is None else mean, ec.sigma_of(name, groups), ec.lr_of(name, groups), rows)
    return ler.init(s, seed=seed, env0=ec.OFF)


def _rule(name, **over):
    c = ec.CASES[name]
    kw = dict(seed=ec.SEED, env0=ec.OFF, T=c["T"], next_step=c["kw"].get("autoreset") == "next_step")
    kw.update(over)
    return kw


def _same_es(env, es, want, what):
    for k in ler.ARRAYS:
        _same(getattr(es, k), want[k], (what, k))
    _same(env.get_linear_policy(), want["cand"], (what, "candidates"))


def _same_objects(a, b, ea, eb, what):
    for x, y, k in zip(ea.tensors(), eb.tensors(), ler.ARRAYS):
        _same(x, y, (what, k))
    _same(a.get_linear_policy(), b.get_linear_policy(), (what, "candidates"))


def _launch_and_check(a, b, es, state, obs0, pend, K, rule, what, info=None, handles=True):
    """one ES launch on a, its twin on b, the restatement; returns (obs, ended, the state and pending after the launch)"""
    obs, rew, term, trunc, act = a.rollout_linear(K, es=es)
    tw = b.rollout(act)
    for j, (x, y) in enumerate(zip((obs, rew, term, trunc), tw)):
        _same(x, y, (what, "twin output", j))
    o = obs.cpu().numpy()
    want_act, state, pend, ended = ler.run_launch(state, obs0, o, tw[1].cpu().numpy(), tw[2].cpu().numpy(), tw[3].cpu().numpy(),
                                                  amax=a.mdps[0].action_space_max, pending=pend, info=info, **rule)
    _same(act, want_act, (what, "actions against the restatement"))
    _same_es(a, es, state, what)
    if handles:                # (status() clears the words it returns: a caller that looks at them itself compares the handles after)
        _same_handles(a, b, what)
    return o, ended, state, pend


def _name_ok(env, K, plds, summary=False):
    name = env.linear_kernel_name(K, summary=summary, es=True)
    assert name.startswith("k_continuous_es_summary<" if summary else "k_continuous_es_rollout<"), name
    assert ("PHILOX=%d" % (env.rng == "philox")) in name, name
    assert "PLDS=0" in name or "PLDS=1" in name, name
    if plds is not None:
        assert ("PLDS=%d" % plds) in name, name
    # the placement rule is the linear kernels': the same template arguments
    assert name.split("<")[1] == env.linear_kernel_name(K, summary=summary).split("<")[1]
    return name


@pytest.mark.parametrize("rng", ec.RNGS)
@pytest.mark.parametrize("name", sorted(ec.CASES))
def test_case_against_twin_and_restatement(name, rng):
    c = ec.CASES[name]
    a, b = _pair(name, rng)
    try:
        obs0 = _start(name, a, b)
        es = _es(a, name)
        kname = _name_ok(a, ec.K, c["plds"])
        noise = any(c["config"].get(k) is not None for k in ("transition_noise", "reward_noise"))
        assert ("NOISE=%d" % noise) in kname, kname
        state, pend, ended, info = _ref_state(name), None, [], ler.new_info()
        _same_es(a, es, state, (name, rng, "init"))
        for launch in range(ec.LAUNCHES):
            o, e, state, pend = _launch_and_check(a, b, es, state, obs0, pend, ec.K, _rule(name), (name, rng, launch), info=info)
            ended.append(e)
            obs0 = o[-1]
        fig = ec.figures(np.concatenate(ended), state["gen"], info)
        print(name, rng, kname, fig)
        ec.assert_figures(name, fig)
        rows, valid = es.curve()
        assert valid.tolist() == np.minimum(state["gen"], ec.ROWS).tolist() and rows.shape[0] == int(valid.max())
        _same(es.mean_theta(), np.ascontiguousarray(state["mean"].T).reshape(ec.G, c["D"], c["D"] + 1), "mean_theta")
        assert not a.status().any()
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("n, ks", ((64, (1,) * 30), (128, (1, 7, 1, 7, 7, 7))))
def test_one_and_two_groups_with_single_step_launches(n, ks):
    """K = 1: the only vote of the launch is the one in finish()"""
    name = "c_d2_n0"
    for rng in ec.RNGS:
        a, b = _pair(name, rng, n=n)
        try:
            obs0 = _start(name, a, b)
            es = _es(a, name, n // 64)
            state, pend, gens = _ref_state(name, n // 64), None, 0
            for K in ks:
                o, e, state, pend = _launch_and_check(a, b, es, state, obs0, pend, K, _rule(name), (n, rng, K))
                obs0 = o[-1]
                gens += int(e.sum()) if K == 1 else 0
            assert (state["gen"] >= 2).all()
            assert gens > 0 or n != 64                           # a generation ended in a one-step launch
        finally:
            a.close(); b.close()


@pytest.mark.parametrize("name", ("c_d2_n0", "autoreset_next_step", "cfg5_T2"))
def test_three_launches_of_37_equal_one_launch_of_111(name):
    for rng in ec.RNGS:
        a, b = _pair(name, rng)
        try:
            _start(name, a, b)
            ea, eb = _es(a, name), _es(b, name)
            parts = [a.rollout_linear(ec.K, es=ea) for _ in range(3)]
            whole = b.rollout_linear(3 * ec.K, es=eb)
            for j in range(5):
                _same(torch.cat([p[j] for p in parts]), whole[j], (name, rng, "output", j))
            _same_objects(a, b, ea, eb, (name, rng))
            _same_handles(a, b, (name, rng))
            assert int(ea.gen.min()) >= 2
        finally:
            a.close(); b.close()


def test_a_member_longer_than_the_launch_carries_over():
    name = "c_d2_n0"
    a, b = _pair(name, "numpy")
    try:
        obs0 = _start(name, a, b)
        es = _es(a, name, episodes_per_member=1000)
        state, pend = _ref_state(name), None
        cand = state["cand"].copy()
        for launch in range(2):
            o, ended, state, pend = _launch_and_check(a, b, es, state, obs0, pend, ec.K, _rule(name, T=1000), ("long member", launch))
            obs0 = o[-1]
            assert not ended.any()
            _same(a.get_linear_policy(), cand, "the candidates are unchanged")
        assert (state["eps"] >= 10).all() and (state["acc"] != 0).all() and not state["gen"].any() and not state["log_mean"].any()
    finally:
        a.close(); b.close()


def test_no_linear_lds_option_against_the_lds_form():
    name = "d4_delay3_every2_alw"
    c = ec.CASES[name]
    for rng in ec.RNGS:
        a = _mk(c["config"], c["kw"], rng, n=ec.N)
        b = _mk(c["config"], c["kw"], rng, n=ec.N, opts=("NO_LINEAR_LDS",))
        try:
            _start(name, a, b)
            ea, eb = _es(a, name), _es(b, name)
            assert "PLDS=1" in _name_ok(a, ec.K, 1) and "PLDS=0" in _name_ok(b, ec.K, 0)
            for launch in range(2):
                ra, rb = a.rollout_linear(ec.K, es=ea), b.rollout_linear(ec.K, es=eb)
                for j, (x, y) in enumerate(zip(ra, rb)):
                    _same(x, y, (rng, launch, j))
                _same_objects(a, b, ea, eb, (rng, launch))
            _same_handles(a, b, rng)
            assert int(ea.gen.min()) >= 2
        finally:
            a.close(); b.close()


def test_a_nan_mean_holds_its_group_and_no_other():
    name = "c_d2_n0"
    a, b = _pair(name, "numpy")
    try:
        mean = ec.mean_of(name).copy()
        mean[2, 1, 2] = np.nan                                          # group 2: every member's bias b[1] is NaN
        obs0 = _start(name, a, b)
        es = _es(a, name, mean=mean)
        state = _ref_state(name, mean=mean)
        o, ended, state, _ = _launch_and_check(a, b, es, state, obs0, None, ec.K, _rule(name), "nan mean", handles=False)
        want = np.zeros(ec.N, bool)
        want[128:192] = True
        for e in (a, b):
            assert np.array_equal((e.status() & 1).astype(bool), want)          # MDPP_STATUS_BAD_ACTION
        _same_handles(a, b, "nan mean")
        # the launch completed; the envs of group 2 stay where they are and are truncated at the limit with a NaN return: the
        # generation ends, the NaNs tie at the lowest rank, and the mean keeps its NaN entry (NaN + gain * S)
        assert state["gen"][2] >= 1 and np.isnan(state["fitness"][128:192]).all() and np.isnan(state["mean"][5, 2])
        assert np.isnan(state["log_mean"][0, 2]) and np.isfinite(np.delete(state["mean"], 2, axis=1)).all()
        assert (np.delete(state["gen"], 2) >= 2).all() and np.isfinite(np.delete(state["log_mean"], 2, axis=1)).all()
    finally:
        a.close(); b.close()


def test_a_member_that_never_ends_an_episode_holds_its_group_and_no_other():
    """no episode limit: a NaN candidate keeps its env in place for ever (BAD_ACTION), it never ends an episode, and its group's
    generation stands still -- the defined behaviour; the other groups go on"""
    name = "c_d2_n0"
    c = ec.CASES[name]
    kw = {k: v for k, v in c["kw"].items() if k != "max_episode_steps"}
    a, b = _mk(c["config"], kw, "philox", n=ec.N), _mk(c["config"], kw, "philox", n=ec.N)
    try:
        mean = ec.mean_of(name).copy()
        mean[:, np.arange(2), np.arange(2)] = -1.0                      # a contracting start: the other groups' envs reach the target
        mean[3, 0, 2] = np.nan
        obs0 = _start(name, a, b)
        sg = np.full(ec.G, 0.02, F32)                                   # (small: every member of the other groups still reaches the target)
        es = _es(a, name, mean=mean, sigma=sg)
        state, pend = ler.init(ler.new_state(mean, sg, ec.lr_of(name), ec.ROWS), seed=ec.SEED, env0=ec.OFF), None
        for launch in range(2):
            o, ended, state, pend = _launch_and_check(a, b, es, state, obs0, pend, ec.K, _rule(name), ("stuck", launch), handles=False)
            obs0 = o[-1]
            assert not ended[:, 3].any()
        assert state["gen"][3] == 0 and (np.delete(state["gen"], 3) >= 1).all() and not state["eps"][192:256].any()
        assert (a.status()[192:256] & 1).all()
    finally:
        a.close(); b.close()


def test_state_dict_round_trip_through_init_on_a_second_handle():
    name = "d3_order2_rel20_box_sparse"
    a, b = _pair(name, "philox")
    c2 = _mk(ec.CASES[name]["config"], ec.CASES[name]["kw"], "philox", n=ec.N, opts=ec.CASES[name]["opts"])
    try:
        _start(name, a, b, c2)
        ea, eb, e2 = _es(a, name), _es(b, name), _es(c2, name)
        for env, es in ((a, ea), (b, eb), (c2, e2)):
            env.rollout_linear(ec.K, es=es)
        assert int(ea.gen.min()) >= 1 and ea.eps.any()
        d = ea.state_dict()
        # b goes on from a fresh init of its own object; c2, another handle with the same history, from a's saved arrays in a
        # new object that was made with other values: the same search
        fresh = _es(c2, name, mean=np.zeros_like(ec.mean_of(name)), sigma=1.0, lr=0.0, seed=0, episodes_per_member=5)
        fresh.load_state_dict(d)
        c2.linear_es_init(fresh)
        b.linear_es_init(eb)
        assert not eb.eps.any() and not eb.acc.any() and not eb.ret.any()
        _same_objects(b, c2, eb, fresh, "after init")
        rb, rc = b.rollout_linear(ec.K, es=eb), c2.rollout_linear(ec.K, es=fresh)
        for j, (x, y) in enumerate(zip(rb, rc)):
            _same(x, y, ("state_dict", j))
        _same_objects(b, c2, eb, fresh, "state_dict")
        _same_handles(b, c2, "state_dict")
        assert int(fresh.gen.min()) > int(d["gen"].min())
    finally:
        a.close(); b.close(); c2.close()


SUMMARY_CASES = ("c_d2_n0", "c_d2_n0_no_lds_T2", "d3_order2_rel20_box_sparse", "d4_delay3_every2_alw", "cfg3", "cfg5_T2",
                 "autoreset_next_step", "max5_autoreset_disabled_T3")


@pytest.mark.parametrize("rng", ec.RNGS)
@pytest.mark.parametrize("name", SUMMARY_CASES)
def test_summary_form_against_the_full_output_twin(name, rng):
    c = ec.CASES[name]
    a, b = _pair(name, rng)
    try:
        _start(name, a, b)
        ea, eb = _es(a, name), _es(b, name)
        kname = _name_ok(a, ec.K, c["plds"], summary=True)
        assert kname.split("<")[1] == _name_ok(b, ec.K, c["plds"]).split("<")[1]
        s = a.episode_summary()
        want, pend = ref.new_summary(ec.N), None
        for launch in range(ec.LAUNCHES):
            assert a.rollout_linear(ec.K, summary=s, es=ea) is s
            _, rew, term, trunc, _ = b.rollout_linear(ec.K, es=eb)
            want, pend = ref.summarise(want, rew.cpu().numpy(), term.cpu().numpy(), trunc.cpu().numpy(),
                                       next_step=c["kw"].get("autoreset") == "next_step", pending=pend)
            for t, k in zip(s.tensors(), ("ret", "len", "episodes", "return_sum", "length_sum")):
                _same(t, want[k], (name, rng, launch, k))
            _same_objects(a, b, ea, eb, (name, rng, launch))
            _same_handles(a, b, (name, rng, launch))
        assert int(ea.gen.min()) >= 2 and int(want["episodes"].sum()) > 0
    finally:
        a.close(); b.close()


def test_explicit_reset_leaves_the_es_alone():
    name = "c_d2_n0"
    a, b = _pair(name, "numpy")
    try:
        _start(name, a, b)
        es = _es(a, name)
        a.rollout_linear(5, es=es)
        before = [t.clone() for t in es.tensors()]
        cand = a.get_linear_policy().clone()
        a.reset()
        for x, y, k in zip(es.tensors(), before, ler.ARRAYS):
            _same(x, y, ("reset", k))
        _same(a.get_linear_policy(), cand, "reset candidates")
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_refusals_of_the_linear_kernels_with_their_reasons(what):
    config, kw, D, reason = REFUSALS[what]
    from mdp_playground_amd.linear_es import LinearES
    env = _mk(config, kw, n=64)
    try:
        with pytest.raises(NotImplementedError, match=reason):
            env.linear_es(np.zeros((D, D + 1), F32), 0.1, 0.1, seed=1)
        es = LinearES(torch.zeros((1, D, D + 1), dtype=torch.float32, device=env.device), 0.1, 0.1, seed=1)
        with pytest.raises(NotImplementedError, match=reason):
            env.rollout_linear(3, es=es)
        assert env.linear_kernel_name(3, es=True) == ""
    finally:
        env.close()


@pytest.mark.parametrize("n", (63, 257))
def test_env_counts_that_are_no_whole_groups_are_refused(n):
    name = "c_d2_n0"
    c = ec.CASES[name]
    from mdp_playground_amd.linear_es import LinearES
    env = _mk(c["config"], c["kw"], n=n)
    try:
        env.reset()
        env.set_linear_policy(ec.theta_of(name, 320)[:n])
        assert env.linear_kernel_name(3, search=True) != "" and env.linear_kernel_name(3, es=True) == ""
        with pytest.raises(NotImplementedError, match="the ES needs whole groups of 64 envs"):
            env.linear_es(np.zeros((2, 3), F32), 0.1, 0.1, seed=1)
        es = LinearES(torch.zeros((max(n // 64, 1), 2, 3), dtype=torch.float32, device=env.device), 0.1, 0.1, seed=1)
        es.num_envs = n                                                 # (past the Python object's own check: the C side refuses)
        for t in ("acc", "ret", "fitness", "eps"):
            setattr(es, t, torch.zeros(n, dtype=getattr(es, t).dtype, device=env.device))
        t0 = gr.tick(env)
        with pytest.raises(NotImplementedError, match="the ES needs whole groups of 64 envs"):
            env.rollout_linear(3, es=es)
        with pytest.raises(NotImplementedError, match="the ES needs whole groups of 64 envs"):
            env.rollout_linear(3, summary=env.episode_summary(), es=es)
        with pytest.raises(NotImplementedError, match="the ES needs whole groups of 64 envs"):
            env.linear_es_init(es)
        assert gr.tick(env) == t0
    finally:
        env.close()


def test_refusals_of_the_es_itself():
    from mdp_playground_amd._capi import MdppError
    name = "c_d2_n0"
    c = ec.CASES[name]
    env = _mk(c["config"], c["kw"], n=64)
    try:
        env.reset()
        theta = ec.theta_of(name, 64)
        mean = ec.mean_of(name, 1)
        with pytest.raises(MdppError, match="no linear policy set"):
            env.linear_es(mean, 0.1, 0.1, seed=1)
        env.set_linear_policy(theta[0])                                 # a shared policy
        with pytest.raises(NotImplementedError, match="the search needs one parameter set per env"):
            env.linear_es(mean, 0.1, 0.1, seed=1)
        assert env.linear_kernel_name(3, es=True) == ""
        env.set_linear_policy(theta)
        es = env.linear_es(mean[0], 0.1, 0.1, seed=1, log_generations=2)           # (a shared [D, D + 1] start is broadcast)
        _same(es.mean_theta(), mean, "broadcast")
        search = env.linear_search(0.1, seed=1)
        with pytest.raises(ValueError, match="exclusive"):
            env.rollout_linear(3, search=search, es=es)
        with pytest.raises(ValueError, match="exclusive"):
            env.rollout_linear(3, summary=env.episode_summary(), search=search, es=es)
        env.set_linear_policy(theta[0])
        with pytest.raises(NotImplementedError, match="the search needs one parameter set per env"):
            env.rollout_linear(3, es=es)
        with pytest.raises(NotImplementedError, match="the search needs one parameter set per env"):
            env.rollout_linear(3, summary=env.episode_summary(), es=es)
        env.set_linear_policy(None)
        with pytest.raises(MdppError, match="no linear policy set"):
            env.rollout_linear(3, es=es)
        env.set_linear_policy(theta)
        for bad in (dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=np.nan), dict(sigma=np.ones(1, np.float64)), dict(sigma=np.ones(2, F32)),
                    dict(lr=-0.1), dict(lr=np.inf), dict(episodes_per_member=0), dict(log_generations=-1), dict(seed=-1)):
            kw = dict(dict(sigma=0.1, lr=0.1, seed=1), **bad)
            with pytest.raises(ValueError):
                env.linear_es(mean, kw.pop("sigma"), kw.pop("lr"), **kw)
        for bad_mean in (mean.astype(np.float64), np.zeros((2, 2, 3), F32), np.zeros((3, 2), F32)):
            with pytest.raises(ValueError):
                env.linear_es(bad_mean, 0.1, 0.1, seed=1)
        with pytest.raises(ValueError):
            env.rollout_linear(3, es=object())
        with pytest.raises(ValueError):
            env.rollout_linear(3, es=search)
        es.gen = es.gen.to(torch.int64)
        with pytest.raises(ValueError):
            env.rollout_linear(3, es=es)
        # the C entry points' own checks (the Python object makes them first): MDPP_EINVAL, nothing launched
        es = env.linear_es(mean, 0.1, 0.1, seed=1, log_generations=2)
        out = env.alloc_rollout_linear(3)
        ptr = [C.c_void_p(t.data_ptr()) for t in (out[4], out[0], out[1], out[2], out[3])]
        sm = [C.c_void_p(t.data_ptr()) for t in env.episode_summary().tensors()]
        before = [t.clone() for t in es.tensors()]
        t0 = gr.tick(env)
        for field, value in (("episodes_per_member", 0), ("log_rows", -1), ("mean", None), ("sigma", None), ("gain", None), ("gen", None),
                             ("acc", None), ("ret", None), ("fitness", None), ("eps", None), ("log_mean", None)):
            s = es.c_struct()
            setattr(s, field, value)
            assert env._lib.mdpp_step_n_linear_es(env._h, 3, C.byref(s), *ptr, None) == -1, field
            assert env._lib.mdpp_step_n_linear_es_summary(env._h, 3, C.byref(s), *sm, None) == -1, field
            assert env._lib.mdpp_linear_es_init(env._h, C.byref(s), None) == -1, field
        assert env._lib.mdpp_step_n_linear_es(env._h, 3, None, *ptr, None) == -1
        assert env._lib.mdpp_linear_es_init(env._h, None, None) == -1
        assert env._lib.mdpp_step_n_linear_es(env._h, 0, C.byref(es.c_struct()), *ptr, None) == -1
        s = es.c_struct()
        s.log_mean, s.log_rows = None, 0                                # a null log with M = 0 is served
        assert env._lib.mdpp_step_n_linear_es(env._h, 3, C.byref(s), *ptr, None) == 0
        torch.cuda.synchronize()
        assert gr.tick(env) == t0 + 3
        for x, y, k in zip(es.tensors(), before, ler.ARRAYS):
            if k in ("mean", "sigma", "gain", "gen", "fitness", "log_mean"):
                _same(x, y, ("three steps of a 7-step episode end no generation", k))
    finally:
        env.close()


def test_the_strategy_optimises_on_the_dense_reward():
    """linear_es_cases.OPT, settled on the oracle by tests/test_linear_es_cases_host.py: the same figures here, on Philox streams"""
    o = ec.OPT
    c = ec.lc.CASES[o["base"]]
    D = c["D"]
    kw = dict(c["kw"], max_episode_steps=o["limit"])
    a, b = _mk(c["config"], kw, "philox", n=64), _mk(c["config"], kw, "philox", n=64)
    try:
        obs0 = _start("c_d2_n0", a, b)
        a.set_linear_policy(np.zeros((64, D, D + 1), F32))
        es = a.linear_es(np.zeros((D, D + 1), F32), o["sigma"], o["lr"], seed=o["seed"], episodes_per_member=o["T"], log_generations=o["rows"])
        state = ler.init(ler.new_state(np.zeros((1, D, D + 1), F32), o["sigma"], o["lr"], o["rows"]), seed=o["seed"], env0=ec.OFF)
        rule = dict(seed=o["seed"], env0=ec.OFF, T=o["T"], next_step=False)
        _launch_and_check(a, b, es, state, obs0, None, o["steps"], rule, "optimise")
        curve, valid = es.curve()
        curve = curve[:, 0].cpu().numpy()
        print(curve.tolist())
        assert int(valid[0]) == o["rows"] and curve[-5:].mean() > curve[:5].mean()
    finally:
        a.close(); b.close()


def test_captured_launch_replays_from_a_graph_against_an_eager_twin():
    """a Philox handle with a delay line in memory; the ES's arrays and the candidates are read and written at replay"""
    name = "d4_delay3_every2_alw"
    a, b = _pair(name, "philox")
    try:
        _start(name, a, b)
        ea, eb = _es(a, name), _es(b, name)
        K = ec.K
        out_a, out_b = a.alloc_rollout_linear(K), b.alloc_rollout_linear(K)
        a.rollout_linear(K, out_a, es=ea)       # (one eager launch of the same form before the capture)
        b.rollout_linear(K, out_b, es=eb)
        torch.cuda.synchronize()
        g = gr.capture(a, lambda: a.rollout_linear(K, out_a, es=ea), K)
        for rep, between in enumerate((1, 2, 3)):
            g.replay()
            b.rollout_linear(K, out_b, es=eb)
            torch.cuda.synchronize()
            for j, (x, y) in enumerate(zip(out_a, out_b)):
                _same(x, y, ("replay", rep, j))
            ra, rb = a.rollout_linear(between, es=ea), b.rollout_linear(between, es=eb)
            for j, (x, y) in enumerate(zip(ra, rb)):
                _same(x, y, ("between", rep, j))
            _same_objects(a, b, ea, eb, ("replay", rep))
        _same_handles(a, b, "graph")
        assert int(ea.gen.min()) >= 8 and not a.status().any()
    finally:
        a.close(); b.close()
