"""k_discrete_rollout_lean with its MDP tables built once per handle (mdpp_discrete_lean.hip k_lean_build_tables,
mdpp_capi.hip lean_tables_build) and its E lanes' first loads issued before the set-up.

A launch copies the handle's blob into LDS instead of rebuilding the tables, so what can go wrong is: a blob that does not
hold what the kernel used to build (every table-shaping parameter below), a copy that leaves part of it out (the
instantiations without an irrelevant sub-space or without reward_every_n_steps copy less), a ragged block whose spare
lanes leave after the set-up, a launch shorter than the action prefetch, a blob left behind by tables that were replaced,
and a blob built lazily inside a launch (a captured launch must not allocate or launch extras).

Every case: two launches in a row through the lean kernel against the same configuration on the single-role kernel
(set_kernel_options("NO_LEAN", "NO_PIPE")) -- obs, reward, terminated, truncated, the handle's state words and the
stream end states, bit for bit, on EVERY env -- and the first launch against the oracle, step for step.  The oracle, the
independent reference, is sampled: every 37th env (7 to 14 envs per case); the single-role kernel covers all of them."""
import dataclasses
import warnings

import numpy as np
import pytest
import torch

import graph_replay_util as gr

pytestmark = pytest.mark.gpu

BASE = dict(state_space_type="discrete", action_space_type="discrete", seed=31)

# name: (config, A, max_episode_steps, N, (K of launch 1, K of launch 2), rng, extra env keywords)
#   S, A: a generated MDP has as many states as actions (S = action_space_size * diameter), so a case with A != S takes the
#   generated MDP of S states and replaces its transition table by a random S x A one (_mdp below): S in {3, 5, 8}, A in {3, 16}.
#   N: 256 one block, 512 two, 300 a ragged second block.  K: 32 the launcher's minimum, 40 five full chunks (fewer than the
#   prefetch depth), 45 a ragged tail chunk, 72.  L 1..3 sets the reward-bit table's mask; delay, every-n and the step limit
#   select the instantiation (and every-n the rows of the reward-value table; it defaults to the sequence length).
def _sq(S, **kw):
    return dict(state_space_size=S, action_space_size=S, **kw)


CASES = {
    "s8_a16_l3_d4": (_sq(8, delay=4, sequence_length=3, reward_every_n_steps=1), 16, None, 256, (32, 45), "numpy", {}),
    "s8_a16_l3_d4_ph": (_sq(8, delay=4, sequence_length=3, reward_every_n_steps=1), 16, None, 512, (40, 72), "philox", {}),
    "s5_a3_l2_d0_ev5_max": (_sq(5, delay=0, sequence_length=2, reward_every_n_steps=5), 3, 11, 300, (45, 32), "numpy", {}),
    "s5_a3_l2_d0_ev5_max_ph": (_sq(5, delay=0, sequence_length=2, reward_every_n_steps=5), 3, 11, 300, (72, 40), "philox", {}),
    "s3_a3_l1_d4_max": (_sq(3, delay=4, sequence_length=1, terminal_state_density=0.34), 3, 7, 512, (40, 72), "numpy", {}),
    "s3_a16_l1_d0_ev5_ph": (_sq(3, delay=0, sequence_length=1, reward_every_n_steps=5, terminal_state_density=0.34), 16, None, 300,
                            (32, 45), "philox", {}),
    "s8_a3_l2_d4_ev5": (_sq(8, delay=4, sequence_length=2, reward_every_n_steps=5), 3, None, 256, (72, 40), "numpy", {}),
    "s5_a16_l3_d0_max_ph": (_sq(5, delay=0, sequence_length=3, reward_every_n_steps=1), 16, 9, 512, (45, 32), "philox", {}),
    # the other forms: their translation units include the kernel's file
    "irr_s8x5_l2_d4": (dict(state_space_size=[8, 5], action_space_size=[8, 5], irrelevant_features=True, delay=4, sequence_length=2),
                       None, None, 300, (40, 45), "numpy", {}),
    "next_s8_a3_l3_d4": (_sq(8, delay=4, sequence_length=3), 3, None, 300, (45, 32), "numpy", dict(autoreset="next_step")),
    "noise_ph": (_sq(8, delay=4, sequence_length=3, transition_noise=0.1, reward_noise=0.2), None, None, 300, (40, 45), "philox", {}),
    "noise_np": (_sq(8, delay=4, sequence_length=3, transition_noise=0.1, reward_noise=0.2), None, None, 256, (45, 72), "numpy", {}),
}
PHILOX_SEED = 5


def _mdp(config, A):
    """the generated MDP of `config`; with A given and != its S, the same MDP on a random S x A transition table (terminal
    states keep their self-loops, rl_toy_env.py:1135-1151)"""
    from mdp_playground_amd import mdp as mdp_mod
    m = mdp_mod.build_mdp(config)
    if A is None or A == m.A:
        return m
    P = np.random.default_rng([int(config["seed"]), m.S, A]).integers(0, m.S, size=(m.S, A)).astype(np.int64)
    for s in m.terminal_states:
        P[int(s), :] = int(s)
    return dataclasses.replace(m, A=A, P=P)


def _venv(cfg, A, max_steps, N, rng, extra, mdp=None, **more):
    from mdp_playground_amd import RLToyVectorEnv
    from mdp_playground_amd import mdp as mdp_mod
    kw = dict(num_envs=N, autoreset="same_step", rng=rng)
    if rng == "philox":
        kw["philox_seed"] = PHILOX_SEED
    if max_steps:
        kw["max_episode_steps"] = max_steps
    kw.update(extra)
    config = dict(BASE, **cfg)
    config.update(more)
    m = _mdp(config, A) if mdp is None else mdp
    build = mdp_mod.build_mdp
    mdp_mod.build_mdp = lambda c: m           # (the constructor of a shared-MDP env builds its MDP from the config)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return RLToyVectorEnv(**kw, **config)
    finally:
        mdp_mod.build_mdp = build


def _actions(env, K, rng):
    m, N = env.mdps[0], env.num_envs
    if env._irr:
        return np.stack([rng.integers(0, m.A, size=(K, N)), rng.integers(0, m.A_irr, size=(K, N))], axis=2).astype(np.int32)
    return rng.integers(0, m.A, size=(K, N)).astype(np.int32)


def _streams_of(env):
    from mdp_playground_amd import _capi as capi
    if env.rng != "numpy":
        return ()
    return (capi.STREAM_ENV, capi.STREAM_SPACE) + ((capi.STREAM_SPACE_IRR,) if env._irr else ())


def _assert_same_outputs(ra, rb, what):
    for j, (x, y) in enumerate(zip(ra, rb)):
        x, y = x.cpu().numpy(), y.cpu().numpy()
        assert x.shape == y.shape and x.dtype == y.dtype, (what, j)
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, "obs reward terminated truncated".split()[j])


def _assert_same_handles(a, b, what):
    sa, sb = a.get_augmented_state(), b.get_augmented_state()
    assert sa.keys() == sb.keys()
    for k in sa:
        assert np.array_equal(sa[k], sb[k], equal_nan=sa[k].dtype.kind == "f"), (what, "state", k)
    for s in _streams_of(a):
        assert np.array_equal(a.get_rng_streams(s), b.get_rng_streams(s)), (what, "stream", s)
    assert np.array_equal(a.status(), b.status()) and not a.status().any(), what


def _oracle(env, i):
    from mdp_playground_amd import _capi as capi
    from oracle import oracle as ora
    m = env.mdps[0]
    o = ora.DiscreteOracle(m.S, m.A, m.sequence_length, m.delay, m.reward_every_n_steps, m.P, m.reward_table(),
                           m.terminal_states, m.init_dist, m.transition_noise, m.reward_noise, m.reward_scale,
                           m.reward_shift, m.term_state_reward)
    if m.irrelevant:
        o.set_irrelevant(m.P_irr, m.init_dist_irr)
    if env.rng == "philox":
        o.set_philox(PHILOX_SEED, i)
    else:
        o.set_rng(env.seeded_streams[capi.STREAM_ENV][i], env.seeded_streams[capi.STREAM_SPACE][i])
        if m.irrelevant:
            o.set_rng_irr(env.seeded_streams[capi.STREAM_SPACE_IRR][i])
    return o


def _assert_first_launch_equals_oracle(env, init, acts, res, max_steps, what):
    """the reference's step() and reset() on env i's own streams, with the autoreset of the handle around them"""
    obs, rew, term, trunc = (x.cpu().numpy() for x in res)
    next_step = env.autoreset == "next_step"
    for i in range(0, env.num_envs, 37):
        o = _oracle(env, i)
        assert np.array_equal(np.asarray(o.reset()), init[i]), (what, i)
        n, pending = 0, False
        for t in range(acts.shape[0]):
            if pending:             # next-step autoreset: this call is the reset -- action ignored, reward 0, no flags
                eo, er, ed, tr = o.reset(explicit=False), 0.0, False, False
                n, pending = 0, False
            else:
                eo, er, ed = o.step(acts[t, i])
                n += 1
                tr = bool(max_steps) and n >= max_steps
                if ed or tr:
                    if next_step:
                        pending = True
                    else:
                        eo, n = o.reset(explicit=False), 0
            assert np.array_equal(np.asarray(obs[t, i]), np.asarray(eo)), (what, i, t)
            assert rew[t, i] == np.float32(er) and bool(term[t, i]) == bool(ed) and bool(trunc[t, i]) == tr, (what, i, t)


@pytest.mark.parametrize("name", sorted(CASES))
def test_lean_launches_on_prebuilt_tables_equal_the_single_role_kernel_and_the_oracle(name):
    cfg, A, max_steps, N, Ks, rng_mode, extra = CASES[name]
    a, b = _venv(cfg, A, max_steps, N, rng_mode, extra), _venv(cfg, A, max_steps, N, rng_mode, extra)
    try:
        b.set_kernel_options("NO_LEAN", "NO_PIPE")
        for K in Ks:
            assert a.rollout_kernel_name(K).startswith("k_discrete_rollout_lean<"), a.rollout_kernel_name(K)
            assert not b.rollout_kernel_name(K).startswith(("k_discrete_rollout_lean<", "k_discrete_rollout_pipe<")), b.rollout_kernel_name(K)
        init = a._obs.cpu().numpy().copy()
        assert np.array_equal(init, b._obs.cpu().numpy())
        rng, ended = np.random.default_rng(sum(name.encode())), 0
        for j, K in enumerate(Ks):
            acts = _actions(a, K, rng)
            ta = torch.as_tensor(acts, device=a.device)
            ra, rb = a.rollout(ta), b.rollout(ta)
            _assert_same_outputs(ra, rb, (name, "launch", j))
            _assert_same_handles(a, b, (name, "launch", j))
            if j == 0:
                _assert_first_launch_equals_oracle(a, init, acts, ra, max_steps, name)
            ended += sum(int(x.sum()) for x in ra[2:])
        assert ended > 0, (name, "no episode ended: the start states were not exercised")
    finally:
        a.close(); b.close()


def _replaced(a, fresh, acts, K, what):
    """`a` has run on its first tables and has just been given those of `fresh`: same streams, same reset, same launches"""
    from mdp_playground_amd import _capi as capi
    for st in (capi.STREAM_SPACE,) + ((capi.STREAM_SPACE_IRR,) if a._irr else ()):
        a._put_stream(st, fresh.seeded_streams[st])
    # (before any launch on the new tables: a lean name means the blob is there, lean_launch refuses a handle without one)
    assert a.rollout_kernel_name(K).startswith("k_discrete_rollout_lean<") and a.rollout_kernel_name(K) == fresh.rollout_kernel_name(K)
    oa, ob = a.reset(seed=99)[0], fresh.reset(seed=99)[0]
    assert torch.equal(oa, ob)
    for j in range(2):
        ra, rb = a.rollout(acts), fresh.rollout(acts)
        _assert_same_outputs(ra, rb, (what, j))
        _assert_same_handles(a, fresh, (what, j))
    return ra


def test_tables_replaced_after_creation_reach_the_lean_kernel():
    """mdpp_upload_discrete_tables on a handle that already has tables: the next lean launch runs on the new ones, like a
    fresh handle created from them (a blob left over from the first upload would step the old MDP)."""
    cfg, N, K = _sq(8, delay=2, sequence_length=2), 300, 45
    a = _venv(cfg, 5, None, N, "numpy", {})
    b = _venv(cfg, 5, None, N, "numpy", {}, seed=77)          # another MDP of the same shape
    try:
        assert not np.array_equal(a.mdps[0].P, b.mdps[0].P)
        acts = torch.as_tensor(_actions(a, K, np.random.default_rng(2)), device=a.device)
        first = tuple(x.clone() for x in a.rollout(acts))                  # (the first tables have been in use)
        a.mdps = b.mdps
        a._upload_discrete_host()
        ra = _replaced(a, b, acts, K, "replaced tables")
        assert not torch.equal(first[0], ra[0])
    finally:
        a.close(); b.close()


def test_irrelevant_tables_replaced_after_creation_reach_the_lean_kernel():
    """The same for mdpp_upload_discrete_irrelevant, which rebuilds the blob too: only the irrelevant sub-space's transition
    table changes (the blob's lds_col1), the relevant tables stay."""
    cfg = dict(state_space_size=[8, 5], action_space_size=[8, 5], irrelevant_features=True, delay=4, sequence_length=2)
    N, K = 300, 45
    a = _venv(cfg, None, None, N, "numpy", {})
    m2 = dataclasses.replace(a.mdps[0], P_irr=_mdp(dict(BASE, **cfg, seed=77), None).P_irr)
    b = _venv(cfg, None, None, N, "numpy", {}, mdp=m2)
    try:
        assert "IRR=1" in a.rollout_kernel_name(K)
        assert not np.array_equal(a.mdps[0].P_irr, m2.P_irr) and np.array_equal(a.mdps[0].P, m2.P)
        acts = torch.as_tensor(_actions(a, K, np.random.default_rng(3)), device=a.device)
        first = tuple(x.clone() for x in a.rollout(acts))
        a.mdps = [m2]
        a._upload_discrete_host()
        ra = _replaced(a, b, acts, K, "replaced irrelevant tables")
        assert not torch.equal(first[0], ra[0])
    finally:
        a.close(); b.close()


def test_lean_launch_replayed_from_a_graph_equals_the_eager_twin():
    """A lean launch captured into a HIP graph and replayed equals an eager twin.  The capture follows one eager launch (as
    for every captured call: tests/graph_replay_util.py), so by itself it could not tell a blob built lazily in that launch;
    that the blob exists right after construction is what the lean kernel name BEFORE the first launch shows -- lean_launch
    refuses a handle without one -- and the capture then holds no allocation or extra launch, which would invalidate it."""
    cfg, max_steps, N, K = _sq(8, delay=4, sequence_length=3, reward_every_n_steps=5), 13, 300, 45
    a, b = _venv(cfg, None, max_steps, N, "philox", {}), _venv(cfg, None, max_steps, N, "philox", {})
    try:
        assert a.rollout_kernel_name(K).startswith("k_discrete_rollout_lean<")          # (no launch yet: the blob exists)
        rng = np.random.default_rng(4)
        acts_a = torch.as_tensor(_actions(a, K, rng), device=a.device)
        acts_b = acts_a.clone()
        out_a, out_b = a.alloc_rollout(K), b.alloc_rollout(K)
        a.rollout(acts_a, out_a); b.rollout(acts_b, out_b)
        torch.cuda.synchronize()
        _assert_same_outputs(out_a, out_b, "warm-up")
        graph = gr.capture(a, lambda: a.rollout(acts_a, out_a), K)
        for r in range(3):
            new = torch.as_tensor(_actions(a, K, rng), device=a.device)
            acts_a.copy_(new); acts_b.copy_(new)
            graph.replay()
            b.rollout(acts_b, out_b)
            torch.cuda.synchronize()
            _assert_same_outputs(out_a, out_b, ("replay", r))
            one = torch.as_tensor(_actions(a, 1, rng)[0], device=a.device)          # (moves the counter off the multiples of K)
            for x, y in zip(a.step(one)[:4], b.step(one)[:4]):
                assert torch.equal(x, y), ("step after replay", r)
        _assert_same_handles(a, b, "graph")
        assert gr.tick(a) == gr.tick(b)
    finally:
        a.close(); b.close()
