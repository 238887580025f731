"""Closed-loop fused rollouts (RLToyVectorEnv.set_policy / rollout_policy, mdpp_discrete_policy.hip).

The policy draws from a Philox stream of its own and from none of the env's, so a closed-loop launch must leave a handle
exactly where an open-loop launch fed with the actions it returned leaves a twin: the twin's outputs, state record, env
streams and step counter are the yardstick for the step, and the action itself is checked against its definition --
    a[k][i] = min(#{ j : T[s][j] <= w >> 1 }, A - 1),   w = philox_tick_word(policy seed, env_id_offset + i, tick0 + k, 14),
s the observation before step k -- with the word from the oracle's Philox.

N = 320 envs (one full workgroup and a partial one: the i >= N guard), K = 37 steps (no multiple of 4: Philox blocks are
entered mid-way) and two launches in a row (the second starts at tick 37, word 1 of its block)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, K = 320, 37
OFF = 1000                        # env_id_offset of the replay cases
SEED = (5 << 32) + 12345          # a policy seed beyond 32 bits
POLICY_STREAM = 14

_D = dict(state_space_type="discrete", action_space_type="discrete")
CFG2 = dict(_D, state_space_size=8, action_space_size=8, delay=4, sequence_length=3, seed=0)
CASES = {
    "cfg2": (CFG2, {}),                                                     # a fast_ok handle on numpy streams
    "s50": (dict(_D, state_space_size=50, action_space_size=50, sequence_length=1, seed=0), {}),
    "rdist_delay3": (dict(_D, state_space_size=8, action_space_size=8, delay=3, sequence_length=2,
                          reward_dist=[0.5, 1.0], seed=0), {}),             # non-unit rewards: the key ring
    "cfg2_next_step": (CFG2, dict(autoreset="next_step")),
    "cfg2_disabled_max5": (CFG2, dict(autoreset="disabled", max_episode_steps=5)),
    "every3": (dict(CFG2, reward_every_n_steps=3), {}),
    "s8_obs_int32": (dict(_D, state_space_size=8, action_space_size=8, delay=0, sequence_length=1, dtype_o=np.int32,
                          seed=0), {}),                                     # 4-byte observations: OBS64=0
}


def _mk(cfg, rng, n=N, **kw):
    from mdp_playground_amd import RLToyVectorEnv
    extra = dict(rng="philox", philox_seed=77) if rng == "philox" else {}
    return RLToyVectorEnv(num_envs=n, **extra, **kw, **cfg)


def _policy(seed, S, A):
    """a stochastic policy with some exactly-zero entries"""
    r = np.random.default_rng(seed)
    p = r.random((S, A))
    p[r.random((S, A)) < 0.3] = 0.0
    p[np.arange(S), r.integers(0, A, S)] += 0.25
    return p / p.sum(axis=1, keepdims=True)


def _tick(env):
    t = C.c_uint64()
    assert env._lib.mdpp_tick(env._h, 0, C.byref(t)) == 0
    return int(t.value)


def _np(x):
    return x.cpu().numpy().copy()


_words_cache = {}


def _words(seed, off, tick0, k, n):
    from oracle import oracle as ora
    key = (seed, off, tick0, k, n)
    if key not in _words_cache:
        _words_cache[key] = np.array([[ora.philox_tick_word(seed, off + i, tick0 + t, POLICY_STREAM) for i in range(n)]
                                      for t in range(k)], dtype=np.uint32)
    return _words_cache[key]


def _assert_action_law(T, seed, off, tick0, obs_before, obs, actions):
    k, n = actions.shape
    m = _words(seed, off, tick0, k, n) >> np.uint32(1)
    states = np.concatenate([obs_before[None], obs[:-1]]).astype(np.int64)
    want = np.minimum((T[states] <= m[..., None]).sum(axis=-1), T.shape[1] - 1)
    assert np.array_equal(actions, want), np.argwhere(actions != want)[:5]


def _assert_same_outputs(got, want, what):
    for name, g, w in zip(("obs", "reward", "terminated", "truncated"), got, want):
        g, w = _np(g), _np(w)
        if name == "reward":
            g, w = g.view(np.int32), w.view(np.int32)       # bit patterns
        assert g.shape == w.shape and np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5])


def _assert_same_handles(a, b, rng):
    from mdp_playground_amd import _capi as capi
    sa, sb = a.get_augmented_state(), b.get_augmented_state()
    assert sa.keys() == sb.keys()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    if rng == "numpy":
        assert np.array_equal(a.get_rng_streams(capi.STREAM_ENV), b.get_rng_streams(capi.STREAM_ENV))
    assert not a.status().any() and not b.status().any()
    assert _tick(a) == _tick(b)


@pytest.mark.parametrize("rng", ["numpy", "philox"])
@pytest.mark.parametrize("case", list(CASES))
def test_replay_by_an_open_loop_twin_and_the_action_law(case, rng):
    cfg, kw = CASES[case]
    a, b = _mk(cfg, rng, env_id_offset=OFF, **kw), _mk(cfg, rng, env_id_offset=OFF, **kw)
    S, A = a.mdps[0].S, a.mdps[0].A
    from mdp_playground_amd.policy import policy_thresholds
    policies = [_policy(11, S, A)] * 2
    if case == "s50":            # a third launch under a deterministic policy (the integer form)
        policies.append(np.random.default_rng(12).integers(0, A, S))
    assert a.policy_kernel_name(K).startswith("k_discrete_policy_rollout<PHILOX=%d," % (rng == "philox"))
    assert ("A8=%d" % (A <= 8)) in a.policy_kernel_name(K)
    assert ("OBS64=%d" % ("dtype_o" not in cfg)) in a.policy_kernel_name(K)
    assert a._obs.dtype == (torch.int32 if "dtype_o" in cfg else torch.int64)
    obs_before = _np(a._obs)
    assert np.array_equal(obs_before, _np(b._obs))
    set_for = None
    for launch, pol in enumerate(policies):
        if pol is not set_for:
            a.set_policy(pol, seed=SEED)
            set_for = pol
        T = policy_thresholds(pol, S, A)
        tick0 = _tick(a)
        assert tick0 == launch * K
        obs, rew, term, trunc, act = a.rollout_policy(K)
        assert act.dtype == torch.int32 and tuple(act.shape) == (K, N)
        _assert_action_law(T, SEED, OFF, tick0, obs_before, _np(obs), _np(act))
        if np.issubdtype(np.asarray(pol).dtype, np.integer):
            states = np.concatenate([obs_before[None], _np(obs)[:-1]])
            assert np.array_equal(_np(act), np.asarray(pol)[states])
        if case == "cfg2" and launch == 1:       # the twin on single steps
            want = [torch.stack(x) for x in zip(*[[t.clone() for t in b.step(act[k])[:4]] for k in range(K)])]
        else:
            want = b.rollout(act)
        _assert_same_outputs((obs, rew, term, trunc), want, (case, rng, launch))
        obs_before = _np(obs)[-1]
    _assert_same_handles(a, b, rng)
    if "next_step" in case or "disabled" not in case:
        assert _np(term).any()                   # (episodes did end inside the launches: resets ran)
    a.close(); b.close()


@pytest.mark.parametrize("rng", ["numpy", "philox"])
def test_interleaved_with_steps_open_loop_rollouts_resets_and_a_new_policy(rng):
    """rollout_policy(5), step(), rollout(K = 9), set_policy(new table, new seed), rollout_policy(8), reset(mask),
    rollout_policy(6): on a fast_ok handle (cfg2 on numpy streams) the queue of start states drawn ahead changes hands in both
    directions."""
    from mdp_playground_amd.policy import policy_thresholds
    a, b = _mk(CFG2, rng), _mk(CFG2, rng)
    S = A = 8
    r = np.random.default_rng(21)
    dev = a.device

    def closed(k, T, seed, what):
        before = _np(a._obs) if a._obs_src is None else _np(a._obs_src)
        tick0 = _tick(a)
        obs, rew, term, trunc, act = a.rollout_policy(k)
        _assert_action_law(T, seed, 0, tick0, before, _np(obs), _np(act))
        _assert_same_outputs((obs, rew, term, trunc), b.rollout(act), what)

    T1 = policy_thresholds(_policy(22, S, A), S, A)
    a.set_policy(_policy(22, S, A), seed=9)
    closed(5, T1, 9, "rollout_policy(5)")
    x = torch.as_tensor(r.integers(0, A, N).astype(np.int32), device=dev)
    _assert_same_outputs(a.step(x)[:4], b.step(x)[:4], "step")
    xs = torch.as_tensor(r.integers(0, A, (9, N)).astype(np.int32), device=dev)
    _assert_same_outputs(a.rollout(xs), b.rollout(xs), "rollout(9)")
    T2 = policy_thresholds(_policy(23, S, A), S, A)
    a.set_policy(thresholds=torch.from_numpy(T2.view(np.int32)).to(dev).view(torch.uint32), seed=SEED)      # (used as given)
    closed(8, T2, SEED, "rollout_policy(8)")
    mask = torch.as_tensor(r.random(N) < 0.4, device=dev)
    oa, _ = a.reset(mask=mask)
    ob, _ = b.reset(mask=mask)
    assert torch.equal(oa, ob)
    closed(6, T2, SEED, "rollout_policy(6)")
    _assert_same_handles(a, b, rng)
    a.close(); b.close()


@pytest.mark.parametrize("rng", ["numpy", "philox"])
def test_two_shards_equal_one_env(rng):
    """320 envs in one handle against 2 x 160 at env_id_offset 0 and 160 (dist.ShardedVectorEnv's construction)."""
    pol = _policy(31, 8, 8)
    whole = _mk(CFG2, rng)
    whole.set_policy(pol, seed=SEED)
    outs = [whole.rollout_policy(K) for _ in range(2)]
    for lo in (0, N // 2):
        sh = _mk(CFG2, rng, n=N // 2, env_id_offset=lo)
        sh.set_policy(pol, seed=SEED)
        for launch in range(2):
            got = sh.rollout_policy(K)
            for g, w in zip(got, outs[launch]):
                assert torch.equal(g, w[:, lo:lo + N // 2]), (rng, lo, launch)
        sh.close()
    whole.close()


@pytest.mark.parametrize("rng", ["numpy", "philox"])
def test_a_policy_call_sent_out_in_pieces_equals_one_launch(rng):
    """LEARN_SHORT_PIECES: launches of at most 5 steps, as a call beyond the buffer descriptors' range is split.  Two calls of
    K = 37 are 8 pieces each: pieces start mid Philox block and k0 steps into the delay line (cfg2: the shift register in
    the record; rdist_delay3: the key ring in memory, read at rhead0 + k).  Outputs, actions and handles are those of the
    single launch.  (An equality test: that the option does split a call is observed by the learner's twin of this test,
    tests/test_gpu_learn_rollout.py, through SARSA's carried action -- both entry points go through one launcher.)"""
    for case in ("cfg2", "rdist_delay3"):
        cfg, kw = CASES[case]
        one, many = _mk(cfg, rng, **kw), _mk(cfg, rng, **kw)
        many.set_kernel_options("LEARN_SHORT_PIECES")
        pol = _policy(41, one.mdps[0].S, one.mdps[0].A)
        for e in (one, many):
            e.set_policy(pol, seed=SEED)
        for launch in range(2):
            want, got = one.rollout_policy(K), many.rollout_policy(K)
            _assert_same_outputs(got[:4], want[:4], (case, rng, launch))
            assert torch.equal(got[4], want[4]), (case, rng, launch)
            assert _np(want[2]).any()                # (episodes ended inside the launches: resets ran)
        _assert_same_handles(one, many, rng)
        one.close(); many.close()


_CONT = dict(state_space_type="continuous", state_space_dim=4, target_point=[0, 0, 0, 0], target_radius=0.05,
             state_space_max=10, action_space_max=1, transition_dynamics_order=1, inertia=1, time_unit=0.1,
             reward_function="move_to_a_point", seed=0)
_GRID = dict(state_space_type="grid", grid_shape=(5, 6), reward_function="move_to_a_point", make_denser=True,
             target_point=[2, 2], seed=0)
_S8 = dict(_D, state_space_size=8, action_space_size=8, delay=0, sequence_length=1, seed=0)
REFUSED = {
    "continuous": (_CONT, {}, "discrete"),
    "grid": (_GRID, {}, "discrete"),
    "irrelevant_features": (dict(_D, state_space_size=[8, 5], action_space_size=[8, 5], irrelevant_features=True, delay=0,
                                 sequence_length=1, seed=0), {}, "irrelevant"),
    "image": (dict(_S8, image_representations=True, image_width=84, image_height=84, image_transforms="shift",
                   image_sh_quant=1), {}, "image"),
    "transition_noise_0": (dict(_S8, transition_noise=0.0), {}, "transition_noise"),
    "transition_noise": (dict(_S8, transition_noise=0.1), {}, "transition_noise"),
    "reward_noise_0": (dict(_S8, reward_noise=0.0), {}, "reward_noise"),
    "reward_noise": (dict(_S8, reward_noise=0.5), {}, "reward_noise"),
    "seeds": (dict(_S8), dict(seeds=[1, 2, 3, 4]), "one shared MDP"),
    "episode_stats": (_S8, dict(episode_stats=True), "episode_stats"),
    "S300": (dict(_D, state_space_size=300, action_space_size=300, delay=0, sequence_length=1, seed=0), {}, "255 states"),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_unsupported_handles_are_refused_with_the_reason(case):
    from mdp_playground_amd import RLToyVectorEnv
    cfg, kw, reason = REFUSED[case]
    cfg = dict(cfg)
    if "seeds" in kw:
        cfg.pop("seed")
    env = RLToyVectorEnv(**({} if "seeds" in kw else {"num_envs": 64}), **kw, **cfg)
    if env.kind == "discrete":
        S, A = env.mdps[0].S, env.mdps[0].A
        with pytest.raises(NotImplementedError, match=reason):
            env.set_policy(np.zeros(S, np.int64))
        with pytest.raises(NotImplementedError, match=reason):
            env.rollout_policy(4)
        assert env.policy_kernel_name(4) == ""
    else:
        with pytest.raises(NotImplementedError, match=reason):
            env.set_policy(np.zeros(4, np.int64))
        with pytest.raises(NotImplementedError, match=reason):
            env.rollout_policy(4, out=env.alloc_rollout(4) + (torch.empty((4, 64), dtype=torch.int32, device=env.device),))
    env.close()


def test_rollout_policy_needs_a_policy():
    from mdp_playground_amd import _capi as capi
    env = _mk(CFG2, "numpy")
    with pytest.raises(capi.MdppError, match="no policy"):
        env.rollout_policy(4)
    env.set_policy(np.zeros(8, np.int64))
    env.rollout_policy(4)
    env.set_policy()                 # cleared
    with pytest.raises(capi.MdppError, match="no policy"):
        env.rollout_policy(4)
    with pytest.raises(ValueError):
        env.set_policy(np.zeros(7, np.int64))
    with pytest.raises(ValueError):
        env.set_policy(thresholds=torch.zeros((8, 8), dtype=torch.int64, device=env.device))
    assert not env.status().any()
    env.close()
