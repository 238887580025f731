"""GPU parity of the batched post-processor (mdpp_post_*, mdp_playground_amd/post.py) — SURVEY.md §8f
rank 4 — against (1) the goldens the reference's GymEnvWrapper produced (tests/golden/w_*.npz) and (2)
the oracle on freshly seeded inputs at sizes the oracle finishes in seconds.  Bit-exact everywhere:
noisy actions, observation floats / pixels, float64 rewards, generator end states."""
import numpy as np
import pytest
import torch

import golden_util as gu
from test_post_oracle_golden import WCASES, make_post_oracle

pytestmark = pytest.mark.gpu


def _post(case, g, num_envs, **kw):
    from mdp_playground_amd.post import VectorPostProcessor
    cfg = dict(case["config"])
    args = dict(n_actions=6)
    if case["kind"] == "continuous":
        args = dict(obs_shape=g["base_obs"].shape[2:], obs_dtype=g["base_obs"].dtype)
    elif case["kind"] == "image":
        args.update(obs_shape=g["base_obs"].shape[2:])
    return VectorPostProcessor(num_envs, **args, **kw, **cfg)


def _bits(t):
    return t.cpu().numpy().tobytes()


@pytest.mark.parametrize("name", sorted(WCASES))
def test_post_vs_gym_env_wrapper_goldens(name):
    case, g = WCASES[name], gu.load(name)
    E, T = g["base_reward"].shape
    post = _post(case, g, E, seed=case["seeds"][0])
    assert np.array_equal(post.get_streams(), g["rng0"])            # the constructor's draws, :93-104
    dev = post.device
    ob0 = post.reset(torch.as_tensor(g["init_base_obs"], device=dev) if case["kind"] == "image" else None)
    if case["kind"] == "image":
        assert _bits(ob0) == g["init_obs"].tobytes()
    cur = None if case["kind"] != "image" else ob0.clone()
    for t in range(T):
        if case["kind"] != "continuous":
            a = post.actions(torch.as_tensor(g["action"][:, t].astype(np.int32), device=dev))
            assert np.array_equal(a.cpu().numpy(), g["action_env"][:, t]), (name, t)
        obs_in = None if case["kind"] == "discrete" else torch.as_tensor(np.ascontiguousarray(g["base_obs"][:, t]), device=dev)
        obs, rew = post.step(obs_in, torch.as_tensor(g["base_reward"][:, t], device=dev),
                             torch.as_tensor(g["base_done"][:, t], device=dev))
        if case["kind"] != "discrete":
            assert _bits(obs) == np.ascontiguousarray(g["obs"][:, t]).tobytes(), (name, t)
        assert np.array_equal(rew.cpu().numpy().view(np.uint64), g["reward"][:, t].view(np.uint64)), (name, t)
        ra = g["reset_after"][:, t]
        if ra.any():
            if case["kind"] == "image":
                cur = obs.clone()
                out = post.reset(torch.as_tensor(np.ascontiguousarray(g["reset_base_obs"][:, t]), device=dev), mask=ra, out=cur)
                got = out.cpu().numpy()
                assert np.array_equal(got[ra], g["reset_obs"][:, t][ra]), (name, t)
                assert np.array_equal(got[~ra], g["obs"][:, t][~ra]), (name, t)          # untouched outside the mask
            else:
                post.reset(mask=ra)
    assert np.array_equal(post.get_streams(), g["rng_end"])
    post.close()


@pytest.mark.parametrize("kind,rng", [("discrete", "numpy"), ("continuous", "numpy"), ("image", "numpy"),
                                      ("discrete", "philox"), ("continuous", "philox"), ("image", "philox")])
def test_post_fused_steps_vs_oracle_at_scale(kind, rng):
    """4 096 instances, K = 24 fused steps in one call (+ a second call: state carried), random inner-env
    outputs incl. done steps with same-step autoreset of the buffer; every 37th instance against the oracle."""
    from mdp_playground_amd.post import VectorPostProcessor
    from oracle import oracle as ora
    N, K = 4096, 24
    r = np.random.default_rng(5)
    cfg = dict(state_space_type="continuous" if kind == "continuous" else "discrete", delay=5, reward_noise=0.3,
               reward_scale=1.5, reward_shift=0.25, term_state_reward=-3.0, seed=77)
    okw = dict(state_space_type=cfg["state_space_type"], delay=5, reward_noise=0.3, reward_scale=1.5, reward_shift=0.25,
               term_state_reward=-3.0)
    args = {}
    if kind == "continuous":
        cfg["transition_noise"] = 0.2
        args = dict(obs_shape=(7,), obs_dtype=np.float32)
        okw.update(transition_noise=0.2, obs_dim=7, obs_dtype=np.float32)
        base_obs = r.normal(size=(2, K, N, 7)).astype(np.float32)
    elif kind == "image":
        cfg.update(image_transforms="shift", image_padding=5, image_sh_quant=3, transition_noise=0.3)
        args = dict(obs_shape=(10, 10, 3), n_actions=5)
        okw.update(transition_noise=0.3, n_actions=5, image_shape=(10, 10, 3), image_transforms="shift", image_padding=5,
                   image_sh_quant=3)
        base_obs = r.integers(0, 256, size=(2, K, N, 10, 10, 3)).astype(np.uint8)
    else:
        cfg["transition_noise"] = 0.3
        args = dict(n_actions=5)
        okw.update(transition_noise=0.3, n_actions=5)
        base_obs = None
    post = VectorPostProcessor(N, rng=rng, autoreset=True, env_id_offset=1000, **args, **cfg)
    dev = post.device
    base_rew = r.integers(-8, 9, size=(2, K, N)) / 4.0
    base_done = r.random((2, K, N)) < 0.08
    acts = r.integers(0, 5, size=(N,)).astype(np.int32)
    start = post.get_streams() if rng == "numpy" else None
    if kind == "image":
        first = r.integers(0, 256, size=(N, 10, 10, 3)).astype(np.uint8)
        ob0 = post.reset(torch.as_tensor(first, device=dev)).cpu().numpy()
    else:
        post.reset()
    a_env = post.actions(torch.as_tensor(acts, device=dev)).cpu().numpy() if kind != "continuous" else None
    # a second block of actions before any step: Philox streams key the action noise by the number of
    # actions() calls, so the second row is not the first row's draw again
    a_env2 = post.actions(torch.as_tensor(acts, device=dev)).cpu().numpy() if kind != "continuous" else None
    if kind != "continuous":
        assert (a_env2 != a_env).any()
    outs = []
    for c in range(2):
        oi = None if base_obs is None else torch.as_tensor(base_obs[c], device=dev)
        o, rw = post.step(oi, torch.as_tensor(base_rew[c], device=dev), torch.as_tensor(base_done[c], device=dev))
        outs.append((None if o is None else o.cpu().numpy(), rw.cpu().numpy()))
    end = post.get_streams() if rng == "numpy" else None
    for i in range(0, N, 37):
        o = ora.PostOracle(**okw)
        if rng == "numpy":
            o.set_rng(start[i])
        else:
            o.set_philox(77, 1000 + i)
        if kind == "image":
            assert np.array_equal(o.reset(first[i]), ob0[i]), i
        else:
            o.reset()
        if kind != "continuous":
            assert o.action(int(acts[i])) == int(a_env[i]), i
            assert o.action(int(acts[i])) == int(a_env2[i]), i
        for c in range(2):
            for k in range(K):
                eo, er = o.step(None if base_obs is None else base_obs[c, k, i], base_rew[c, k, i], base_done[c, k, i])
                if base_obs is not None:
                    assert np.array_equal(eo, outs[c][0][k, i]), (i, c, k)
                assert np.float64(er).view(np.uint64) == outs[c][1][k, i].view(np.uint64), (i, c, k)
                if base_done[c, k, i]:
                    import ctypes
                    ora.lib().ora_p_reset(o.h, None, None) if kind != "image" else _oracle_ring_reset(o)
        if rng == "numpy":
            assert np.array_equal(o.get_rng(), end[i]), i
    post.close()


@pytest.mark.parametrize("delay", [0, 1, 2, 3, 4, 6, 7, 8, 9, 16, 17, 40])
def test_post_reward_fifo_every_delay_vs_oracle(delay):
    """The reward FIFO of k_post_step in each of its forms -- none, the register shift with the delay as a
    compile-time constant (1..8; 8 is where numpy's pairwise flush sum starts), the LDS ring (9..16), slots in HBM --
    on 512 instances, three calls of 19, 30 and 11 fused steps with done steps (flush + same-step buffer reset), bit
    for bit against the oracle."""
    from mdp_playground_amd.post import VectorPostProcessor
    from oracle import oracle as ora
    N = 512
    r = np.random.default_rng(100 + delay)
    kw = dict(state_space_type="discrete", delay=delay, reward_scale=0.75, reward_shift=-0.125, term_state_reward=2.0)
    post = VectorPostProcessor(N, n_actions=4, autoreset=True, seed=5, **kw)
    dev = post.device
    post.reset()
    chunks = [(r.integers(-16, 17, size=(K, N)) / 8.0, r.random((K, N)) < 0.07) for K in (19, 30, 11)]   # (state carried)
    outs = [post.step(None, torch.as_tensor(rw, device=dev), torch.as_tensor(dn, device=dev))[1].cpu().numpy() for rw, dn in chunks]
    for i in range(0, N, 13):
        o = ora.PostOracle(n_actions=4, **kw)
        o.reset()
        for (rw, dn), got in zip(chunks, outs):
            for k in range(rw.shape[0]):
                _, er = o.step(None, rw[k, i], dn[k, i])
                assert np.float64(er).view(np.uint64) == got[k, i].view(np.uint64), (delay, i, k)
                if dn[k, i]:
                    ora.lib().ora_p_reset(o.h, None, None)
    post.close()


def _oracle_ring_reset(o):
    """autoreset=True refills the buffer after a done step without drawing an image (the caller resets its
    observations itself): the oracle's reset() minus its image draw."""
    w = o.get_rng()
    o.reset(np.zeros(o.shape, np.uint8))
    o.set_rng(w)


def test_post_chained_behind_the_vector_env():
    """RLToyVectorEnv (the reference's RLToyEnv, batched) -> VectorPostProcessor (its GymEnvWrapper): both on
    the device, no host round trip; sanity of shapes / dtypes and of the delay line across the chain."""
    from mdp_playground_amd import RLToyVectorEnv
    from mdp_playground_amd.post import VectorPostProcessor
    N = 512
    env = RLToyVectorEnv(num_envs=N, autoreset="disabled", state_space_type="discrete", action_space_type="discrete",
                         state_space_size=8, action_space_size=8, delay=0, sequence_length=1, reward_density=0.5, seed=3)
    post = VectorPostProcessor(N, n_actions=8, state_space_type="discrete", delay=2, reward_scale=2.0, seed=11)
    post.reset()
    rews = []
    for t in range(12):
        a = torch.randint(0, 8, (N,), device=env.device, dtype=torch.int32)
        obs, r, term, trunc, _ = env.step(post.actions(a))
        _, r2 = post.step(None, r, torch.zeros_like(term))
        rews.append((r.double().cpu().numpy(), r2.cpu().numpy()))
    for t in range(2, 12):
        assert np.array_equal(rews[t][1], rews[t - 2][0] * 2.0)
    assert (rews[0][1] == 0).all() and (rews[1][1] == 0).all()
    env.close(); post.close()


def test_episode_stats_kernel_equals_the_host_loop():
    """stats_csv.EpisodeStats on device tensors (mdpp_episode_stats: one kernel over [K, N]) against the same class on
    host tensors (plain torch ops, step by step): running returns / lengths bit-equal, counts equal, the sums of
    returns equal up to the order of a float64 summation; float32 env rewards and float64 post-processor rewards,
    one or two end-flag rows, state carried across calls, a ragged batch."""
    from mdp_playground_amd.stats_csv import EpisodeStats
    dev = torch.device("cuda", 0)
    r = np.random.default_rng(3)
    for N, K, dt in ((65536, 512, np.float32), (1000, 37, np.float64)):
        d, h = EpisodeStats(N, dev), EpisodeStats(N, "cpu")
        for call in range(2):
            rew = (r.integers(-8, 9, size=(K, N)) / 4.0).astype(dt)
            term = r.random((K, N)) < 0.03
            trunc = r.random((K, N)) < 0.01
            if call == 0:
                d.update(torch.as_tensor(rew, device=dev), torch.as_tensor(term, device=dev), torch.as_tensor(trunc, device=dev))
                h.update(torch.as_tensor(rew), torch.as_tensor(term), torch.as_tensor(trunc))
            else:
                d.update(torch.as_tensor(rew, device=dev), torch.as_tensor(term | trunc, device=dev).to(torch.uint8))
                h.update(torch.as_tensor(rew), torch.as_tensor(term | trunc))
            assert torch.equal(d.ret.cpu(), h.ret) and torch.equal(d.len.cpu(), h.len), (N, call)
            assert int(d.count.item()) == int(h.count.item()) and int(d.sum_len.item()) == int(h.sum_len.item())
            assert abs(float(d.sum_ret.item()) - float(h.sum_ret.item())) <= 1e-9 * max(1.0, abs(float(h.sum_ret.item())))
        td, th = d.pop(), h.pop()
        assert td[0] == th[0] == 2 * K * N and td[2] == th[2] and abs(td[1] - th[1]) < 1e-9
    # a single row ([N] tensors), as a step() loop would feed it
    d = EpisodeStats(256, dev)
    d.update(torch.ones(256, device=dev), torch.zeros(256, dtype=torch.bool, device=dev))
    d.update(torch.ones(256, device=dev), torch.ones(256, dtype=torch.bool, device=dev))
    assert d.pop() == (512, 2.0, 2.0)


@pytest.mark.parametrize("kind", ["discrete", "continuous"])
def test_irrelevant_toy_env_wrapper_is_two_envs_side_by_side(kind):
    """post.IrrelevantToyEnvWrapper (gym_env_wrapper.py:214-270, :378-396, :476-486): the nested toy env steps on the
    second part of every action, contributes the second part of every observation and nothing else, and is reset only
    together with the wrapped env -- against the two envs driven by hand."""
    from mdp_playground_amd import RLToyVectorEnv
    from mdp_playground_amd.post import IrrelevantToyEnvWrapper
    N, T = 256, 40
    if kind == "discrete":
        base = dict(state_space_type="discrete", action_space_type="discrete", state_space_size=8, action_space_size=8,
                    delay=1, sequence_length=2, seed=3)
        toy = dict(state_space_type="discrete", action_space_type="discrete", state_space_size=6, action_space_size=6, seed=5)
        mk_act = lambda g: torch.stack([torch.randint(0, 8, (N,), generator=g, device="cuda", dtype=torch.int32),      # noqa: E731
                                        torch.randint(0, 6, (N,), generator=g, device="cuda", dtype=torch.int32)], dim=1)
        kw = {}
    else:
        base = dict(state_space_type="continuous", state_space_dim=3, target_point=[0, 0, 0], target_radius=0.8, state_space_max=4,
                    action_space_max=1, transition_dynamics_order=1, inertia=1, time_unit=1, reward_function="move_to_a_point", seed=3)
        toy = dict(state_space_type="continuous", state_space_dim=2, target_point=[0, 0], target_radius=0.01, state_space_max=6,
                   action_space_max=1, transition_dynamics_order=2, inertia=1, time_unit=0.5, reward_function="move_to_a_point", seed=5)
        mk_act = lambda g: torch.rand((N, 5), generator=g, device="cuda") * 2 - 1      # noqa: E731
        kw = dict(env_action_dim=3)
    w = IrrelevantToyEnvWrapper(RLToyVectorEnv(num_envs=N, autoreset="disabled", **base), N, toy, state_space_type=kind,
                                autoreset=True, **kw)
    a, b = RLToyVectorEnv(num_envs=N, autoreset="disabled", **base), RLToyVectorEnv(num_envs=N, autoreset="disabled", **toy)
    o, _ = w.reset()
    assert o.shape == ((N, 2) if kind == "discrete" else (N, 5))
    a.reset(); b.reset()
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    ends = 0
    for t in range(T):
        act = mk_act(g)
        o, r, te, tr, info = w.step(act)
        if kind == "discrete":
            oa, ra, ta, _, _ = a.step(act[:, 0].contiguous()); ob = b.step(act[:, 1].contiguous())[0]
            want = torch.stack((oa, ob), dim=1)
        else:
            oa, ra, ta, _, _ = a.step(act[:, :3].contiguous()); ob = b.step(act[:, 3:].contiguous())[0]
            want = torch.cat((oa, ob), dim=1)
        assert torch.equal(info["final_obs"], want) and torch.equal(r, ra) and torch.equal(te, ta), (kind, t)
        if bool(ta.any()):
            fa, _ = a.reset(mask=ta); fb, _ = b.reset(mask=ta)
            fresh = torch.stack((fa, fb), dim=1) if kind == "discrete" else torch.cat((fa, fb), dim=1)
            want = torch.where(ta.view(-1, 1), fresh, want)
            ends += int(ta.sum())
        assert torch.equal(o, want), (kind, t)
    assert ends > 0
    w.close(); a.close(); b.close()


def _post_fuzz(n, seed):
    r = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        kind = str(r.choice(["discrete", "continuous", "image"]))
        p = dict(kind=kind, rng=str(r.choice(["numpy", "numpy", "philox"])), delay=int(r.choice([0, 1, 2, 5, 9, 33, 100])),
                 N=int(r.choice([1000, 1024, 2048 + 64, 4096])), K=int(r.choice([1, 3, 17, 40])),
                 reward_scale=float(r.choice([1.0, 1.5, -2.0])), reward_shift=float(r.choice([0.0, 0.25])),
                 term_state_reward=float(r.choice([0.0, -3.0])), p_done=float(r.choice([0.02, 0.08, 0.3])))
        rn, tn = r.choice([-1.0, 0.0, 0.3]), r.choice([-1.0, 0.0, 0.2])
        if rn >= 0:
            p["reward_noise"] = float(rn)
        if tn >= 0:
            p["transition_noise"] = float(tn)
        if kind == "continuous":
            p["obs_dim"] = int(r.choice([1, 2, 7, 12, 17]))
        elif kind == "image":
            p.update(hw=int(r.choice([6, 10, 16])), ch=int(r.choice([1, 3])), pad=int(r.choice([2, 5, 8])), shq=int(r.choice([1, 2, 3])))
        if kind != "continuous":
            p["n_actions"] = int(r.choice([2, 5, 18]))
        out.append(p)
    return out


POST_FUZZ = _post_fuzz(36, 99)


@pytest.mark.timeout(180)
@pytest.mark.parametrize("k", range(len(POST_FUZZ)))
def test_post_random_configurations_vs_oracle(k):
    """36 seeded random post-processor configurations (the GymEnvWrapper's delay line up to 100, reward noise /
    transition noise present with sigma 0 or absent, scale / shift / terminal reward, float observations of 1-17 dimensions,
    padded and shifted pictures of several sizes, 2-18 actions; ragged instance counts; K fused steps in two calls with the
    state carried), every 41st instance against the oracle: actions, observations, rewards as float64 bit patterns, end streams."""
    from mdp_playground_amd.post import VectorPostProcessor
    from oracle import oracle as ora
    p = POST_FUZZ[k]
    kind, rng, N, K = p["kind"], p["rng"], p["N"], p["K"]
    r = np.random.default_rng(300 + k)
    common = dict(delay=p["delay"], reward_scale=p["reward_scale"], reward_shift=p["reward_shift"], term_state_reward=p["term_state_reward"])
    for key in ("reward_noise", "transition_noise"):
        if key in p:
            common[key] = p[key]
    cfg = dict(common, state_space_type="continuous" if kind == "continuous" else "discrete", seed=77)
    okw = dict(common, state_space_type=cfg["state_space_type"])
    args, base_obs = {}, None
    if kind == "continuous":
        d = p["obs_dim"]
        args = dict(obs_shape=(d,), obs_dtype=np.float32)
        okw.update(obs_dim=d, obs_dtype=np.float32)
        base_obs = r.normal(size=(2, K, N, d)).astype(np.float32)
    elif kind == "image":
        shp = (p["hw"], p["hw"], p["ch"])
        cfg.update(image_transforms="shift", image_padding=p["pad"], image_sh_quant=p["shq"])
        args = dict(obs_shape=shp, n_actions=p["n_actions"])
        okw.update(n_actions=p["n_actions"], image_shape=shp, image_transforms="shift", image_padding=p["pad"], image_sh_quant=p["shq"])
        base_obs = r.integers(0, 256, size=(2, K, N) + shp).astype(np.uint8)
    else:
        args = dict(n_actions=p["n_actions"])
        okw.update(n_actions=p["n_actions"])
    # (none of _post_fuzz's combinations is among mdpp_post_create's documented refusals -- delay > 128, an odd or non-square picture,
    #  a canvas that is no multiple of 4 bytes, shift without padding, noise outside [0, 1]: a refusal here is a failure, not a skip)
    post = VectorPostProcessor(N, rng=rng, autoreset=True, env_id_offset=500, **args, **cfg)
    dev = post.device
    base_rew = r.integers(-8, 9, size=(2, K, N)) / 4.0
    base_done = r.random((2, K, N)) < p["p_done"]
    start = post.get_streams() if rng == "numpy" else None
    if kind == "image":
        first = r.integers(0, 256, size=(N,) + shp).astype(np.uint8)
        ob0 = post.reset(torch.as_tensor(first, device=dev)).cpu().numpy()
    else:
        post.reset()
    if kind != "continuous":
        acts = r.integers(0, p["n_actions"], size=(N,)).astype(np.int32)
        a_env = post.actions(torch.as_tensor(acts, device=dev)).cpu().numpy()
    outs = []
    for c in range(2):
        oi = None if base_obs is None else torch.as_tensor(base_obs[c], device=dev)
        o, rw = post.step(oi, torch.as_tensor(base_rew[c], device=dev), torch.as_tensor(base_done[c], device=dev))
        outs.append((None if o is None else o.cpu().numpy(), rw.cpu().numpy()))
    end = post.get_streams() if rng == "numpy" else None
    for i in range(1, N, 41):
        o = ora.PostOracle(**okw)
        if rng == "numpy":
            o.set_rng(start[i])
        else:
            o.set_philox(77, 500 + i)
        if kind == "image":
            assert np.array_equal(o.reset(first[i]), ob0[i]), (p, i)
        else:
            o.reset()
        if kind != "continuous":
            assert o.action(int(acts[i])) == int(a_env[i]), (p, i)
        for c in range(2):
            for t in range(K):
                eo, er = o.step(None if base_obs is None else base_obs[c, t, i], base_rew[c, t, i], base_done[c, t, i])
                if base_obs is not None:
                    assert np.array_equal(eo, outs[c][0][t, i]), (p, i, c, t)
                assert np.float64(er).view(np.uint64) == outs[c][1][t, i].view(np.uint64), (p, i, c, t, er, outs[c][1][t, i])
                if base_done[c, t, i]:
                    ora.lib().ora_p_reset(o.h, None, None) if kind != "image" else _oracle_ring_reset(o)
        if rng == "numpy":
            assert np.array_equal(o.get_rng(), end[i]), (p, i)
    post.close()
