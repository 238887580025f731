"""The post-processor's kernels (mdp_playground_amd/csrc/mdpp_post.hip) at the shapes of tests/post_shape_cases.py:
pictures of the reference's size and up to the LDS form's limit and past it, every form of the picture launch, every
ring form of the step kernel with both streams and reward noise, K around the prefetch depth, ragged instance counts,
autoreset=False with done steps inside a fused call, float observations, the action kernel's edges.

EVERY instance, every pixel and every reward (as a float64 bit pattern) is compared against the oracle
(oracle.PostOracle: plain C, one call per step; pinned without a GPU by tests/test_post_shapes_host.py and
tests/test_post_oracle_golden.py).  No tolerance anywhere; the kernel form each case runs is asserted through
VectorPostProcessor.kernel_name().  Rewards are normal draws over several orders of magnitude, not dyadic fractions: the
order of the additions in the flush on done shows in the result."""
import numpy as np
import pytest
import torch

import post_shape_cases as cases
from oracle import oracle as ora

pytestmark = pytest.mark.gpu

REWARD = dict(reward_scale=-2.0, reward_shift=0.25, term_state_reward=1.5)


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w = got.reshape(-1).view(np.uint8), want.reshape(-1).view(np.uint8)
    if not np.array_equal(g, w):
        bad = np.flatnonzero(g != w)
        at = np.unravel_index(int(bad[0]) // got.dtype.itemsize, got.shape)
        raise AssertionError(f"{what}: {bad.size} bytes differ, first at {at}: got {got[at]!r}, want {want[at]!r}")


class Twin:
    """A VectorPostProcessor and one PostOracle per instance, driven side by side; every call compares everything it
    returned.  Philox streams: the batch's three counters (steps, reset() calls, actions() calls) are kept here and
    given to an oracle before each of its calls -- a masked reset moves the batch's reset counter for everybody."""

    def __init__(self, N, rng, common, *, autoreset=True, n_actions=0, obs_dim=0, obs_dtype=None, image=None):
        from mdp_playground_amd.post import VectorPostProcessor
        self.N, self.rng, self.autoreset = N, rng, autoreset
        self.image, self.cont = image is not None, common["state_space_type"] == "continuous"
        args, okw = dict(n_actions=n_actions), dict(common, n_actions=n_actions)
        if self.cont:
            args = dict(obs_shape=(obs_dim,), obs_dtype=obs_dtype)
            okw = dict(common, obs_dim=obs_dim, obs_dtype=obs_dtype)
        if self.image:
            cfg, iokw = image
            args["obs_shape"] = iokw["image_shape"]
            okw.update(iokw)
            common = dict(common, **cfg)
        self.post = VectorPostProcessor(N, rng=rng, autoreset=autoreset, env_id_offset=cases.ENV0, seed=cases.SEED, **args, **common)
        self.dev = self.post.device
        self.oracles = [ora.PostOracle(**okw) for _ in range(N)]
        if rng == "numpy":
            for o, w in zip(self.oracles, self.post.get_streams()):
                o.set_rng(w)
        else:
            for i, o in enumerate(self.oracles):
                o.set_philox(cases.SEED, cases.ENV0 + i)
        self.tick = self.reset_tick = self.action_tick = 0

    def _sync(self, o):
        if self.rng == "philox":
            o.set_counters(self.tick, self.reset_tick, self.action_tick)

    def _dev(self, a):
        return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=self.dev)

    def reset(self, first=None, mask=None, out=None):
        """reset(); with a mask on picture handles `out` (a device tensor) holds the previous canvases."""
        prev = None if out is None else out.cpu().numpy().copy()
        got = self.post.reset(self._dev(first), mask=None if mask is None else self._dev(mask), out=out)
        want = None if prev is None else prev.copy()
        for i, o in enumerate(self.oracles):
            if mask is not None and not mask[i]:
                continue
            self._sync(o)
            canvas = o.reset(None if first is None else first[i])
            if self.image:
                if want is None:
                    want = np.empty((self.N,) + canvas.shape, np.uint8)
                    assert mask is None
                want[i] = canvas
        self.reset_tick += 1
        if self.image:
            got = got.cpu().numpy()
            _same_bits(got, want, "reset canvases")
            if prev is not None:
                return got, prev
        return got

    def actions(self, acts, n_actions):
        got = self.post.actions(self._dev(acts.astype(np.int32))).cpu().numpy()
        want = acts.astype(np.int32).copy()
        for i, o in enumerate(self.oracles):
            if 0 <= acts[i] < n_actions:                  # (out of range: passed through, nothing drawn)
                self._sync(o)
                want[i] = o.action(int(acts[i]))
        self.action_tick += 1
        _same_bits(got, want, "actions")
        return got

    def step(self, obs, rew, done):
        """One fused call: obs [K, N, ...] or None, rew float64 [K, N], done bool [K, N]."""
        K = rew.shape[0]
        o_out, r_out = self.post.step(self._dev(obs), self._dev(rew), self._dev(done))
        want_r, want_o = np.empty((K, self.N), np.float64), None
        for i, o in enumerate(self.oracles):
            self._sync(o)
            for k in range(K):
                eo, er = o.step(None if obs is None else obs[k, i], rew[k, i], done[k, i])
                want_r[k, i] = er
                if obs is not None:
                    if want_o is None:
                        want_o = np.empty((K, self.N) + eo.shape, eo.dtype)
                    want_o[k, i] = eo
                if done[k, i] and self.autoreset:
                    o.clear_ring()
        self.tick += K
        _same_bits(r_out.cpu().numpy(), want_r, f"rewards of a K={K} call")
        if obs is not None:
            got_o = o_out.cpu().numpy()
            _same_bits(got_o, want_o, f"observations of a K={K} call")
        return o_out

    def check_ring(self):
        delay = self.oracles[0].delay
        want = np.stack([o.ring() for o in self.oracles]) if delay else np.zeros((self.N, 0))
        _same_bits(self.post.reward_buffer(), want, "reward buffer")

    def check_streams(self):
        if self.rng == "numpy":
            _same_bits(self.post.get_streams(), np.stack([o.get_rng() for o in self.oracles]), "end streams")

    def close(self):
        self.post.close()


def _rewards(r, shape):
    return r.normal(size=shape) * 10.0 ** r.integers(-2, 3, size=shape)


def _dones(r, K, N, p=0.12):
    d = r.random((K, N)) < p
    d[r.integers(0, K), r.integers(0, N)] = True           # at least one, whatever the size
    return d


# ---------------------------------------------------------------------------------------------------------------
# pictures
def _picture_twin(p, rng, N=None):
    common = dict(REWARD, state_space_type="discrete", delay=p["delay"], reward_noise=0.25)
    t = Twin(p["N"] if N is None else N, rng, common, n_actions=4, image=cases.pic_config(p))
    name = t.post.kernel_name(p["K"])
    print(f"{p['name']} [{rng}]: {name}")
    assert name == cases.kernel_name(rng, p["delay"], (p["hw"], p["ch"], cases.pic_pad(p))), name
    assert name.endswith(p["form"] if p["form"] == cases.GEN else f"{cases.LDS}<LDS={p['lds']},PER_CU={p['per_cu']}>")
    return t


@pytest.mark.parametrize("name,rng", [(p["name"], rng) for p in cases.PICTURES for rng in p["rngs"]])
def test_pictures_every_instance_every_pixel_vs_oracle(name, rng):
    """reset, then two fused calls with the state carried and done steps under autoreset=True."""
    p = cases.PICTURE[name]
    N, K, shape = p["N"], p["K"], (p["hw"], p["hw"], p["ch"])
    r = np.random.default_rng(sum(map(ord, name)))
    t = _picture_twin(p, rng)
    t.reset(r.integers(0, 256, size=(N,) + shape, dtype=np.uint8))
    for call in range(2):
        obs = r.integers(0, 256, size=(K, N) + shape, dtype=np.uint8)
        done = _dones(r, K, N) if N * K > 1 else np.full((1, 1), call == 0)
        t.step(obs, _rewards(r, (K, N)), done)
    t.check_ring()
    t.check_streams()
    t.close()


@pytest.mark.parametrize("rng", cases.RNGS)
@pytest.mark.parametrize("name", cases.MASKED_RESET)
def test_masked_reset_leaves_the_other_canvases_alone(name, rng):
    """reset(mask, out=previous canvases): masked instances get the new canvas, the others keep every byte (the picture
    kernels skip them), and their streams do not move."""
    p = cases.PICTURE[name]
    N, K, shape = 33, 2, (p["hw"], p["hw"], p["ch"])
    r = np.random.default_rng(11)
    t = _picture_twin(p, rng, N=N)
    t.reset(r.integers(0, 256, size=(N,) + shape, dtype=np.uint8))
    out = t.step(r.integers(0, 256, size=(K, N) + shape, dtype=np.uint8), _rewards(r, (K, N)), _dones(r, K, N))
    mask = r.random(N) < 0.5
    mask[0], mask[-1] = True, False
    got, prev = t.reset(r.integers(0, 256, size=(N,) + shape, dtype=np.uint8), mask=mask, out=out[-1].clone())
    assert np.array_equal(got[~mask], prev[~mask]) and (got[mask] != prev[mask]).any()
    t.step(r.integers(0, 256, size=(K, N) + shape, dtype=np.uint8), _rewards(r, (K, N)), _dones(r, K, N))
    t.check_ring()
    t.check_streams()
    t.close()


# ---------------------------------------------------------------------------------------------------------------
# the step kernel
@pytest.mark.parametrize("noise", [0.3, 0.0])
@pytest.mark.parametrize("rng", cases.RNGS)
@pytest.mark.parametrize("delay", cases.RING_DELAYS)
def test_ring_forms_with_draws_vs_oracle(delay, rng, noise):
    """No FIFO, the register FIFO (1, 7, 8), the LDS ring (9, 16) and HBM slots (17, 128: the cap), each with numpy and
    Philox streams and reward noise in the same kernel (sigma 0.3, or present with sigma 0: drawn all the same)."""
    N = cases.RING_N
    common = dict(REWARD, state_space_type="discrete", delay=delay, reward_noise=noise)
    t = Twin(N, rng, common, n_actions=4)
    assert t.post.kernel_name(cases.RING_CALLS[0]) == cases.step_name(rng, delay)
    r = np.random.default_rng(1000 + delay)
    t.reset()
    if delay > 16:                       # (fill the buffer once round, so that the FIFO's front has wrapped)
        t.step(None, _rewards(r, (delay + 1, N)), np.zeros((delay + 1, N), bool))
    for K in cases.RING_CALLS:
        t.step(None, _rewards(r, (K, N)), _dones(r, K, N))
        t.check_ring()
    t.check_streams()
    t.close()


def test_delay_past_the_cap_is_refused():
    from mdp_playground_amd import _capi
    from mdp_playground_amd.post import VectorPostProcessor
    with pytest.raises(_capi.MdppError, match=cases.REFUSAL):
        VectorPostProcessor(8, n_actions=4, state_space_type="discrete", delay=cases.REFUSED_DELAY, seed=1)


@pytest.mark.parametrize("rng", cases.RNGS)
@pytest.mark.parametrize("delay", cases.K_SEQUENCE_DELAYS)
def test_fused_lengths_around_the_prefetch_depth(delay, rng):
    """K = 1, 7, 8, 9, 15, 16, 17 on one handle in sequence (8 and 16: no tail; 7 and 15: the longest tail), done flags
    on the first and the last row of every call."""
    N = 257
    t = Twin(N, rng, dict(REWARD, state_space_type="discrete", delay=delay, reward_noise=0.3), n_actions=4)
    assert t.post.kernel_name(8) == cases.step_name(rng, delay)
    r = np.random.default_rng(delay)
    t.reset()
    for n, K in enumerate(cases.K_SEQUENCE):
        done = _dones(r, K, N, 0.05)
        done[0, n::5] = True
        done[K - 1, (n + 2)::7] = True
        t.step(None, _rewards(r, (K, N)), done)
        t.check_ring()
    t.check_streams()
    t.close()


@pytest.mark.parametrize("rng", cases.RNGS)
@pytest.mark.parametrize("kind", ["discrete", "continuous"])
@pytest.mark.parametrize("N", cases.N_CASES)
def test_every_instance_at_ragged_counts(N, kind, rng):
    """One lane, one short of / exactly / one past a wave and a workgroup, and 1000 (a ragged last workgroup), with the
    LDS ring (discrete) and observation noise (continuous)."""
    r = np.random.default_rng(N)
    K = 9
    if kind == "discrete":
        t = Twin(N, rng, dict(REWARD, state_space_type="discrete", delay=9, reward_noise=0.3, transition_noise=0.25), n_actions=5)
    else:
        t = Twin(N, rng, dict(REWARD, state_space_type="continuous", delay=2, reward_noise=0.3, transition_noise=0.2),
                 obs_dim=3, obs_dtype=np.float32)
    t.reset()
    for call in range(2):
        if kind == "discrete":
            t.actions(r.integers(0, 5, size=N), 5)
        obs = None if kind == "discrete" else r.normal(size=(K, N, 3)).astype(np.float32)
        t.step(obs, _rewards(r, (K, N)), _dones(r, K, N))
    t.check_ring()
    t.check_streams()
    t.close()


@pytest.mark.parametrize("rng", cases.RNGS)
@pytest.mark.parametrize("delay", cases.NO_AUTORESET_DELAYS)
def test_no_autoreset_keeps_the_ring_through_done_steps(delay, rng):
    """autoreset=False: done steps in the middle of a fused call flush the buffer's sum and leave the buffer as it is
    (the oracle is simply not reset); then reset(mask = the last row's dones), then another fused call."""
    N, K = 257, 17
    t = Twin(N, rng, dict(REWARD, state_space_type="discrete", delay=delay, reward_noise=0.3), autoreset=False, n_actions=4)
    assert t.post.kernel_name(K) == cases.step_name(rng, delay)
    r = np.random.default_rng(50 + delay)
    t.reset()
    t.step(None, _rewards(r, (delay + 2, N)), np.zeros((delay + 2, N), bool))      # a full buffer
    done = np.zeros((K, N), bool)
    done[3:13] = r.random((10, N)) < 0.2
    done[K - 1] = r.random(N) < 0.3
    assert done[3:13].any() and done[K - 1].any() and not done[K - 1].all()
    t.step(None, _rewards(r, (K, N)), done)
    t.check_ring()
    assert t.post.reward_buffer()[done[3:13].any(axis=0) & ~done[K - 1]].any()   # (not emptied by a done step)
    t.reset(mask=done[K - 1])
    t.check_ring()
    t.step(None, _rewards(r, (9, N)), _dones(r, 9, N))
    t.check_ring()
    t.check_streams()
    t.close()


@pytest.mark.parametrize("rng", cases.RNGS)
@pytest.mark.parametrize("noise", cases.CONT_NOISES)
@pytest.mark.parametrize("dim", cases.CONT_DIMS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_continuous_observations_every_instance(dtype, dim, noise, rng):
    N, K = 257, 9
    common = dict(REWARD, state_space_type="continuous", delay=3, reward_noise=0.3)
    if noise is not None:
        common["transition_noise"] = noise
    t = Twin(N, rng, common, obs_dim=dim, obs_dtype=dtype)
    r = np.random.default_rng(dim)
    t.reset()
    for call in range(2):
        t.step((r.normal(size=(K, N, dim)) * 3.0).astype(dtype), _rewards(r, (K, N)), _dones(r, K, N))
    t.check_ring()
    t.check_streams()
    t.close()


# ---------------------------------------------------------------------------------------------------------------
# the action kernel
@pytest.mark.parametrize("rng", cases.RNGS)
@pytest.mark.parametrize("noise", cases.ACTION_NOISES)
@pytest.mark.parametrize("n", cases.ACTION_COUNTS)
def test_action_noise_edges(n, noise, rng):
    """2 to 300 actions; noise 0.0 (identity, streams unmoved), 0.25, 1.0 (never the given action); two actions() calls
    before a step and one between two steps; out-of-range actions in a few lanes come back unchanged and draw nothing."""
    N, K = 257, 2
    t = Twin(N, rng, dict(REWARD, state_space_type="discrete", delay=1, reward_noise=0.3, transition_noise=noise), n_actions=n)
    r = np.random.default_rng(n)
    odd = np.array([3, 64, 200, 256])                       # lanes with out-of-range actions
    t.reset()

    def acts():
        a = r.integers(0, n, size=N)
        a[odd] = [-1, n, n, -1]
        return a
    before = t.post.get_streams() if rng == "numpy" else None
    a0 = acts()
    got = t.actions(a0, n)
    inside = np.ones(N, bool)
    inside[odd] = False
    assert np.array_equal(got[odd], a0[odd])
    if noise == 0.0:
        assert np.array_equal(got, a0)
    if noise == 1.0:
        assert (got[inside] != a0[inside]).all()
    if rng == "numpy":
        moved = (t.post.get_streams() != before).any(axis=1)
        assert not moved[odd].any() and moved[inside].all() == (noise != 0.0) and moved[inside].any() == (noise != 0.0)
    second = t.actions(a0, n)                               # the same actions again: other draws
    if noise == 0.25 and n > 2:
        assert (second != got).any()
    t.step(None, _rewards(r, (K, N)), _dones(r, K, N))
    t.actions(acts(), n)
    t.step(None, _rewards(r, (K, N)), _dones(r, K, N))
    t.check_streams()
    t.close()
