"""In-kernel tabular TD learners (RLToyVectorEnv.set_learner / rollout_learn, mdpp_discrete_learn.hip).

The learner draws from two Philox streams of its own and from none of the env's, so a learning launch must leave a handle
exactly where an open-loop launch fed with the actions it returned leaves a twin: the twin's outputs, state record, env and
space streams and step counter are the yardstick for the step.  The actions and the Q-tables are checked, bit for bit,
against tests/learner_ref.py -- a numpy restatement of the learner's semantics fed with the launch's own outputs.

N = 320 envs (one full workgroup and a partial one), K = 37 steps (no multiple of 4: Philox blocks are entered mid-way)
and two launches in a row (the second starts at tick 37; SARSA's carry is dropped between them)."""
import ctypes as C

import numpy as np
import pytest
import torch

import learner_ref as ref

pytestmark = pytest.mark.gpu

N, K = 320, 37
OFF = 1000                        # env_id_offset of the twin cases
SEED = (7 << 32) + 4321           # a learner seed beyond 32 bits
ALPHA, GAMMA, EPS = 0.3, 0.9, 0.25

_D = dict(state_space_type="discrete", action_space_type="discrete")
# MDP seed 40 for the delayed-reward shapes: the learner starts from all-zero tables, where every greedy choice is the tie's
# action 0, and under seed 0 that walk so rarely earns cfg2's delayed sequence reward that 74 steps leave the tables of 18 of
# the 320 envs non-zero (measured; 133 for rdist_delay3, 4 with autoreset disabled) -- the conditions at the end of
# test_twin_and_restatement would not hold.  Seed 40 was picked on the CPU with the restatement over seeds 0 ... 40.
CFG2 = dict(_D, state_space_size=8, action_space_size=8, delay=4, sequence_length=3, seed=40)
_S8 = dict(_D, state_space_size=8, action_space_size=8, delay=0, sequence_length=1, seed=0)
CASES = {
    "cfg2": (CFG2, {}),                                                     # a fast_ok handle on numpy streams
    "rdist_delay3": (dict(_D, state_space_size=8, action_space_size=8, delay=3, sequence_length=2,
                          reward_dist=[0.5, 1.0], seed=40), {}),            # non-unit rewards: the key ring
    "cfg2_next_step": (CFG2, dict(autoreset="next_step")),
    "cfg2_disabled_max5": (CFG2, dict(autoreset="disabled", max_episode_steps=5)),
    "s8_noise_keys_at_0": (dict(_S8, transition_noise=0.0, reward_noise=0.0), {}),      # the reference's tabular shape
    "s8_noise": (dict(_S8, transition_noise=0.1, reward_noise=0.5), {}),
    "s20": (dict(_D, state_space_size=20, action_space_size=20, delay=0, sequence_length=1, seed=0), {}),   # the global-memory form
    # beyond the issue's list: the kernel's remaining branches
    "rdist_noise": (dict(_D, state_space_size=8, action_space_size=8, delay=3, sequence_length=2, reward_dist=[0.5, 1.0],
                         transition_noise=0.1, reward_noise=0.5, seed=40), {}),          # reward noise on the key-ring path
    "s70_noise": (dict(_D, state_space_size=70, action_space_size=70, delay=0, sequence_length=1, transition_noise=0.1,
                       reward_noise=0.5, seed=0), {}),                                   # the noise cdfs (38 KiB) stay in global memory
    "s8_obs_int32": (dict(_S8, dtype_o=np.int32), {}),                                   # 4-byte observations
}
GLOBAL_FORM = ("s20", "s70_noise")


def _mk(cfg, rng, n=N, **kw):
    from mdp_playground_amd import RLToyVectorEnv
    extra = dict(rng="philox", philox_seed=77) if rng == "philox" else {}
    return RLToyVectorEnv(num_envs=n, **extra, **kw, **cfg)


def _tick(env):
    t = C.c_uint64()
    assert env._lib.mdpp_tick(env._h, 0, C.byref(t)) == 0
    return int(t.value)


def _np(x):
    return x.cpu().numpy().copy()


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def _obs_now(env):
    return _np(env._obs) if env._obs_src is None else _np(env._obs_src)


def _assert_same_outputs(got, want, what):
    for name, g, w in zip(("obs", "reward", "terminated", "truncated"), got, want):
        g, w = _np(g), _np(w)
        if name == "reward":
            g, w = _bits(g), _bits(w)
        assert g.shape == w.shape and np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5])


def _assert_same_handles(a, b, rng):
    from mdp_playground_amd import _capi as capi
    sa, sb = a.get_augmented_state(), b.get_augmented_state()
    assert sa.keys() == sb.keys()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    if rng == "numpy":
        for st in (capi.STREAM_ENV, capi.STREAM_SPACE):
            assert np.array_equal(a.get_rng_streams(st), b.get_rng_streams(st)), st
    assert not a.status().any() and not b.status().any()
    assert _tick(a) == _tick(b)


class Restated:
    """the restatement, carried from launch to launch beside a handle"""

    def __init__(self, env, algo, q0=None, off=0, seed=SEED, alpha=ALPHA, gamma=GAMMA, eps=EPS, autoreset=ref.SAME_STEP):
        m = env.mdps[0]
        self.algo, self.off, self.seed, self.alpha, self.gamma, self.eps, self.autoreset = algo, off, seed, alpha, gamma, eps, autoreset
        self.P = np.asarray(m.P)
        self.Q = np.zeros((env.num_envs, m.S, m.A), np.float32) if q0 is None else q0.copy()
        self.pending = np.zeros(env.num_envs, bool)
        self.info = {}

    def launch(self, tick0, obs_before, out):
        """the restatement's actions for the launch that returned `out`; Q and the pending flags move on"""
        obs, rew, term, trunc = (_np(x) for x in out[:4])
        k, n = obs.shape
        w_e = ref.tick_words(self.seed, self.off, tick0, k + 1, n, ref.EXPLORE_STREAM)
        w_a = ref.tick_words(self.seed, self.off, tick0, k + 1, n, ref.ACTION_STREAM)
        act, self.Q, self.pending, info = ref.run(self.algo, self.alpha, self.gamma, self.eps, self.Q, obs_before, obs, rew, term, trunc,
                                                  self.P, self.autoreset, w_e, w_a, self.pending)
        for key, v in info.items():
            self.info[key] = self.info.get(key, 0) + v
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
    assert q.dtype == np.float32 and np.array_equal(_bits(q), _bits(r.Q)), (what, "Q", np.argwhere(_bits(q) != _bits(r.Q))[:5])
    return out


@pytest.mark.parametrize("rng", ["numpy", "philox"])
@pytest.mark.parametrize("algo", ["q_learning", "sarsa"])
@pytest.mark.parametrize("case", list(CASES))
def test_twin_and_restatement(case, algo, rng):
    cfg, kw = CASES[case]
    a, b = _mk(cfg, rng, env_id_offset=OFF, **kw), _mk(cfg, rng, env_id_offset=OFF, **kw)
    noise = "transition_noise" in cfg
    name = a.learn_kernel_name(K)
    assert name == "k_discrete_learn_rollout<PHILOX=%d,NOISE=%d,UNIT=%d,QLDS=%d>" % (
        rng == "philox", noise, "reward_dist" not in cfg, case not in GLOBAL_FORM), name
    assert a._obs.dtype == (torch.int32 if "dtype_o" in cfg else torch.int64)
    a.set_learner(algo, alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=SEED)
    r = Restated(a, algo, off=OFF, autoreset=kw.get("autoreset", ref.SAME_STEP))
    assert np.array_equal(_obs_now(a), _obs_now(b))
    terminated = 0
    for launch in range(2):
        assert _tick(a) == launch * K
        out = _check_launch(a, r, K, (case, algo, rng, launch))
        _assert_same_outputs(out[:4], b.rollout(out[4]), (case, algo, rng, launch))
        terminated += int(_np(out[2]).sum())
    _assert_same_handles(a, b, rng)
    # what keeps the pass honest
    info, pairs = r.info, 2 * K * N
    nonzero_envs = int((r.Q != 0).any(axis=(1, 2)).sum())
    print(case, algo, rng, info, "terminated", terminated, "envs with non-zero Q", nonzero_envs)
    assert terminated > 0
    assert 0.15 <= info["explored"] / pairs <= 0.35, info
    assert info["greedy_ties"] > 0 and info["greedy_strict"] > 0, info
    assert nonzero_envs > N // 2
    if algo == "sarsa":
        assert info["carried"] > 0 and info["carried_differs"] > 0, info
    a.close(); b.close()


def _random_q(seed, n, S, A):
    return np.random.default_rng(seed).normal(size=(n, S, A)).astype(np.float32)


@pytest.mark.parametrize("algo", ["q_learning", "sarsa"])
def test_epsilon_0_is_greedy_from_a_given_table_and_epsilon_1_ignores_the_table(algo):
    q0 = _random_q(5, N, 8, 8)
    a = _mk(CFG2, "numpy")
    a.set_learner(algo, alpha=ALPHA, gamma=GAMMA, epsilon=0.0, seed=SEED, q=torch.as_tensor(q0, device=a.device))
    assert np.array_equal(_bits(_np(a.get_q())), _bits(q0))
    r = Restated(a, algo, q0=q0, eps=0.0)
    before = _obs_now(a)
    out = _check_launch(a, r, K, ("eps0", algo))
    assert r.info["explored"] == 0 and r.info["greedy_strict"] > 0
    assert np.array_equal(_np(out[4])[0], np.argmax(q0[np.arange(N), before], axis=1))
    a.close()
    # epsilon = 1: the actions are the explore rule's whatever Q holds
    acts = []
    for q in (None, q0):
        e = _mk(CFG2, "numpy")
        e.set_learner(algo, alpha=ALPHA, gamma=GAMMA, epsilon=1.0, seed=SEED, q=None if q is None else torch.as_tensor(q, device=e.device))
        acts.append(_np(e.rollout_learn(K)[4]))
        e.close()
    w_a = ref.tick_words(SEED, 0, 0, K + 1, N, ref.ACTION_STREAM)[:K]
    want = (w_a.astype(np.uint64) * np.uint64(8)) >> np.uint64(32)
    assert np.array_equal(acts[0], want) and np.array_equal(acts[1], want)


def test_set_learner_rates_between_launches_and_the_q_round_trip():
    from mdp_playground_amd import _capi as capi
    a = _mk(_S8, "philox")
    with pytest.raises(capi.MdppError, match="no learner"):
        a.set_learner_rates(alpha=0.5)
    a.set_learner("q_learning", alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=SEED)
    r = Restated(a, "q_learning")
    _check_launch(a, r, K, "before")
    a.set_learner_rates(alpha=0.5, epsilon=1.0)
    r.alpha, r.eps = 0.5, 1.0
    r.info = {}
    _check_launch(a, r, K, "alpha 0.5, epsilon 1")
    assert r.info["explored"] == K * N
    a.set_learner_rates(epsilon=0.0)                     # (alpha stays 0.5)
    r.eps = 0.0
    r.info = {}
    _check_launch(a, r, 6, "epsilon 0")
    assert r.info["explored"] == 0
    with pytest.raises(ValueError):
        a.set_learner_rates(alpha=0.0)
    with pytest.raises(ValueError):
        a.set_learner_rates(epsilon=1.5)
    # set_q / get_q
    q = _random_q(6, N, 8, 8)
    a.set_q(torch.as_tensor(q, device=a.device))
    assert np.array_equal(_bits(_np(a.get_q())), _bits(q))
    r.Q = q.copy()
    _check_launch(a, r, 5, "after set_q")
    for bad in (torch.zeros((N, 8, 7), device=a.device), torch.zeros((N, 8, 8), dtype=torch.float64, device=a.device),
                torch.zeros((N, 8, 8)), q):
        with pytest.raises(ValueError):
            a.set_q(bad)
        with pytest.raises(ValueError):
            a.set_learner("sarsa", alpha=ALPHA, gamma=GAMMA, epsilon=EPS, q=bad)
    for kw in (dict(alpha=0.0), dict(alpha=1.1), dict(gamma=-0.1), dict(gamma=1.5), dict(epsilon=-0.1), dict(epsilon=2.0)):
        with pytest.raises(ValueError):
            a.set_learner("sarsa", **dict(dict(alpha=ALPHA, gamma=GAMMA, epsilon=EPS), **kw))
    with pytest.raises(ValueError):
        a.set_learner("double_q_learning", alpha=ALPHA, gamma=GAMMA, epsilon=EPS)
    assert not a.status().any()
    a.close()


@pytest.mark.parametrize("rng", ["numpy", "philox"])
@pytest.mark.parametrize("algo", ["q_learning", "sarsa"])
def test_interleaved_with_policy_rollouts_open_loop_rollouts_steps_and_resets(algo, rng):
    """rollout_learn(5), step(), rollout(9), rollout_policy(8), rollout_learn(8), reset(mask), rollout_learn(6) on a fast_ok
    handle (cfg2 on numpy streams: the queue of start states drawn ahead changes hands in both directions)."""
    a, b = _mk(CFG2, rng), _mk(CFG2, rng)
    A = 8
    rs = np.random.default_rng(21)
    dev = a.device
    a.set_learner(algo, alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=SEED)
    r = Restated(a, algo)

    def learn(k, what):
        out = _check_launch(a, r, k, what)
        _assert_same_outputs(out[:4], b.rollout(out[4]), what)

    learn(5, "rollout_learn(5)")
    x = torch.as_tensor(rs.integers(0, A, N).astype(np.int32), device=dev)
    _assert_same_outputs(a.step(x)[:4], b.step(x)[:4], "step")
    xs = torch.as_tensor(rs.integers(0, A, (9, N)).astype(np.int32), device=dev)
    _assert_same_outputs(a.rollout(xs), b.rollout(xs), "rollout(9)")
    a.set_policy(rs.integers(0, A, 8), seed=3)
    out = a.rollout_policy(8)
    _assert_same_outputs(out[:4], b.rollout(out[4]), "rollout_policy(8)")
    q_before = _np(a.get_q())
    assert np.array_equal(_bits(q_before), _bits(r.Q))   # (none of these touched the tables)
    learn(8, "rollout_learn(8)")
    mask = torch.as_tensor(rs.random(N) < 0.4, device=dev)
    oa, _ = a.reset(mask=mask)
    ob, _ = b.reset(mask=mask)
    assert torch.equal(oa, ob)
    learn(6, "rollout_learn(6)")
    _assert_same_handles(a, b, rng)
    a.close(); b.close()


@pytest.mark.parametrize("rng", ["numpy", "philox"])
@pytest.mark.parametrize("algo", ["q_learning", "sarsa"])
def test_two_shards_equal_one_env(algo, rng):
    """320 envs in one handle against 2 x 160 at env_id_offset 0 and 160 (dist.ShardedVectorEnv's construction)."""
    whole = _mk(CFG2, rng)
    whole.set_learner(algo, alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=SEED)
    outs = [whole.rollout_learn(K) for _ in range(2)]
    q = whole.get_q()
    for lo in (0, N // 2):
        sh = _mk(CFG2, rng, n=N // 2, env_id_offset=lo)
        sh.set_learner(algo, alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=SEED)
        for launch in range(2):
            got = sh.rollout_learn(K)
            for g, w in zip(got, outs[launch]):
                assert torch.equal(g, w[:, lo:lo + N // 2]), (algo, rng, lo, launch)
        assert torch.equal(sh.get_q().view(torch.int32), q[lo:lo + N // 2].view(torch.int32))
        sh.close()
    whole.close()


@pytest.mark.parametrize("rng", ["numpy", "philox"])
@pytest.mark.parametrize("algo", ["q_learning", "sarsa"])
def test_a_call_sent_out_in_pieces_equals_one_launch(algo, rng):
    """LEARN_SHORT_PIECES: launches of at most 5 steps, as a call beyond the buffer descriptors' range is split; SARSA's action
    crosses the pieces, so outputs, actions and tables are those of the single launch."""
    one, many = _mk(CFG2, rng), _mk(CFG2, rng)
    many.set_kernel_options("LEARN_SHORT_PIECES")
    for e in (one, many):
        e.set_learner(algo, alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=SEED)
    r = Restated(many, algo)
    for launch in range(2):
        want = one.rollout_learn(K)
        got = _check_launch(many, r, K, (algo, rng, launch))
        for g, w in zip(got, want):
            assert torch.equal(g, w), (algo, rng, launch)
    assert torch.equal(one.get_q().view(torch.int32), many.get_q().view(torch.int32))
    if algo == "sarsa":
        assert r.info["carried_differs"] > 0
    _assert_same_handles(one, many, rng)
    one.close(); many.close()


_CONT = dict(state_space_type="continuous", state_space_dim=4, target_point=[0, 0, 0, 0], target_radius=0.05,
             state_space_max=10, action_space_max=1, transition_dynamics_order=1, inertia=1, time_unit=0.1,
             reward_function="move_to_a_point", seed=0)
_GRID = dict(state_space_type="grid", grid_shape=(5, 6), reward_function="move_to_a_point", make_denser=True,
             target_point=[2, 2], seed=0)
REFUSED = {
    "continuous": (_CONT, {}, "discrete"),
    "grid": (_GRID, {}, "discrete"),
    "irrelevant_features": (dict(_D, state_space_size=[8, 5], action_space_size=[8, 5], irrelevant_features=True, delay=0,
                                 sequence_length=1, seed=0), {}, "irrelevant"),
    "image": (dict(_S8, image_representations=True, image_width=84, image_height=84, image_transforms="shift",
                   image_sh_quant=1), {}, "image"),
    "seeds": (dict(_S8), dict(seeds=[1, 2, 3, 4]), "one shared MDP"),
    "episode_stats": (_S8, dict(episode_stats=True), "episode_stats"),
    "tables_beyond_lds": (dict(_D, state_space_size=255, action_space_size=255, delay=0, sequence_length=1, seed=0), {}, "64 KiB"),
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
    with pytest.raises(NotImplementedError, match=reason):
        env.set_learner("q_learning", alpha=ALPHA, gamma=GAMMA, epsilon=EPS)
    with pytest.raises(NotImplementedError, match=reason):
        env.set_learner("sarsa", alpha=ALPHA, gamma=GAMMA, epsilon=EPS)
    out = env.alloc_rollout(4) + (torch.empty((4, env.num_envs), dtype=torch.int32, device=env.device),)
    with pytest.raises(NotImplementedError, match=reason):
        env.rollout_learn(4, out=out)
    assert env.learn_kernel_name(4) == ""
    env.close()


def test_rollout_learn_needs_a_learner():
    from mdp_playground_amd import _capi as capi
    env = _mk(CFG2, "numpy")
    with pytest.raises(capi.MdppError, match="no learner"):
        env.rollout_learn(4)
    with pytest.raises(capi.MdppError, match="no learner"):
        env.get_q()
    env.set_learner("sarsa", alpha=ALPHA, gamma=GAMMA, epsilon=EPS)
    env.rollout_learn(4)
    env.set_learner(None)                # cleared
    with pytest.raises(capi.MdppError, match="no learner"):
        env.rollout_learn(4)
    assert not env.status().any()
    env.close()
