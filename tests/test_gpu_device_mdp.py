"""Per-env discrete MDPs generated on the device (mdpp_generate.hip via RLToyVectorEnv(seeds=...)) against the host
builder mdp.build_mdp, the reference's goldens, and host-built handles: tables, seed dicts, streams and behaviour."""
import warnings

import numpy as np
import pytest
import torch

import gen_configs as gc
import golden_util as gu
from mdp_playground_amd import _capi as capi
from mdp_playground_amd import mdp

pytestmark = pytest.mark.gpu

BASE = dict(state_space_type="discrete", action_space_type="discrete")
CFG2 = dict(BASE, state_space_size=8, action_space_size=8, delay=4, sequence_length=3)
S50 = dict(BASE, state_space_size=50, action_space_size=50, sequence_length=1)
CONFIGS = {
    "cfg2": CFG2,
    "l1": dict(BASE, action_space_size=8, sequence_length=1),
    "l2_rep": dict(BASE, action_space_size=8, sequence_length=2, repeats_in_sequences=True),
    "l3": dict(BASE, action_space_size=8, sequence_length=3, reward_density=0.1),
    "l4_rep": dict(BASE, action_space_size=8, sequence_length=4, repeats_in_sequences=True),
    "l4": dict(BASE, action_space_size=8, sequence_length=4),
    "denser": dict(BASE, action_space_size=8, sequence_length=3, make_denser=True),
    "rdist_l1": dict(BASE, action_space_size=8, sequence_length=1, reward_density=1.0, reward_dist=[0.5, 1.0]),
    "rdist_l3_d2": dict(BASE, action_space_size=5, diameter=2, sequence_length=3, reward_dist=[0.1, 1.0]),
    "diam2": dict(BASE, action_space_size=4, diameter=2, sequence_length=2),
    "diam3_rep": dict(BASE, action_space_size=4, diameter=3, sequence_length=3, repeats_in_sequences=True),
    "not_maxc": dict(BASE, action_space_size=8, diameter=2, maximally_connected=False, sequence_length=2),
    "s50": S50,
    "s255": dict(BASE, action_space_size=255, sequence_length=1, reward_density=0.1),
    "image": dict(BASE, action_space_size=8, sequence_length=2, image_representations=True, image_width=32,
                  image_height=32),
    "noise": dict(BASE, action_space_size=8, sequence_length=2, transition_noise=0.1, reward_noise=0.5),
}


def _seeds(n, salt=0):
    r = np.random.default_rng(1234 + salt)
    fixed = [0, 1, 2 ** 32 + 3, 2 ** 32 + 77, 2 ** 62 + 5, 2 ** 62 + 11, 5874934615388537134, 2 ** 64 - 1]
    rest = [int(x) for x in r.integers(0, 2 ** 63, size=n - len(fixed) - n // 4, dtype=np.uint64)]
    small = [int(x) for x in r.integers(0, 2 ** 32, size=n // 4, dtype=np.uint64)]
    return fixed + rest + small


def _build(cfg, s):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return mdp.build_mdp({**cfg, "seed": s})


def _venv(**kw):
    from mdp_playground_amd import RLToyVectorEnv
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return RLToyVectorEnv(**kw)


def _check_env(env, cfg, seeds, idx):
    """Env i's tables, seed dict and streams on the device equal build_mdp({**cfg, "seed": seeds[i]}) for i in idx."""
    tabs = env.get_mdp_tables()
    sd = env.get_seed_dicts()
    # (what the device held right after generation, read back by the constructor before its reset drew from it)
    streams = env.seeded_streams
    image = cfg.get("image_representations", False)
    assert set(streams) == {capi.STREAM_ENV, capi.STREAM_SPACE} | ({capi.STREAM_IMAGE} if image else set())
    for i in idx:
        m = _build(cfg, seeds[i])
        assert np.array_equal(tabs["P"][i], m.P), i
        if m.S ** m.sequence_length > gc.DENSE_KEYS:      # key by key: no dense host table of every env
            gc.assert_reward_row(m, rbits=tabs["rbits"][i] if "rbits" in tabs else None,
                                 rtable=tabs["rtable"][i] if "rtable" in tabs else None, tag=i)
        else:
            t = m.reward_table()
            if "rbits" in tabs:
                assert np.array_equal(tabs["rbits"][i], np.packbits((t != 0).astype(np.uint8), bitorder="little")), i
            else:
                assert np.array_equal(tabs["rtable"][i], t), i
        assert np.array_equal(tabs["is_term"][i], m.is_terminal_table()), i
        assert np.array_equal(tabs["init_cdf"][i], m.init_cdf()), i
        assert sd[i].tolist() == [seeds[i]] + [m.seed_dict[k] for k in mdp._SEED_KEYS], i
        assert np.array_equal(streams[capi.STREAM_ENV][i], mdp.pcg64_words(mdp.new_generator(seeds[i]))), i
        # (the device keeps no buffered half-word for the space stream: mdpp_seed_streams drops it as well)
        assert np.array_equal(streams[capi.STREAM_SPACE][i][:4], m.space_rng_words[:4]), i
        if image:
            assert np.array_equal(streams[capi.STREAM_IMAGE][i],
                                  mdp.pcg64_words(mdp.new_generator(m.seed_dict["image_representations"]))), i


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_device_tables_and_streams_equal_host_builder(name):
    cfg = CONFIGS[name]
    seeds = _seeds(1024, salt=len(name))
    env = _venv(seeds=seeds, autoreset="same_step", **cfg)
    assert env.tables_built_on == "device"
    _check_env(env, cfg, seeds, range(len(seeds)))
    # the space stream is only drawn from by transition noise: untouched by the constructor's reset
    assert np.array_equal(env.seeded_streams[capi.STREAM_SPACE], env.get_rng_streams(capi.STREAM_SPACE))
    assert int(env.status().sum()) == 0
    env.close()


def _covered_goldens():
    out = []
    for name in gu.DISCRETE + gu.IMAGE:
        seeds = gu.CASES[name]["seeds"]
        if seeds == [None] or None in seeds:
            continue
        if mdp.device_coverage(gu.CASES[name]["config"], seeds)[0]:
            out.append(name)
    return out


COVERED_GOLDENS = _covered_goldens()


def test_some_goldens_are_covered():
    assert len(COVERED_GOLDENS) >= 20, COVERED_GOLDENS


@pytest.mark.parametrize("name", COVERED_GOLDENS)
def test_device_tables_equal_reference_golden(name):
    g = gu.load(name)
    cfg = dict(gu.CASES[name]["config"])
    seeds = gu.CASES[name]["seeds"]
    env = _venv(seeds=seeds, autoreset="disabled", **cfg)
    assert env.tables_built_on == "device"
    tabs = env.get_mdp_tables()
    S, L = env._cfg.S, env._cfg.L
    for e in range(len(seeds)):
        assert np.array_equal(tabs["P"][e], g["P"][e]), e
        keys = [int(sum(int(x) * S ** (L - 1 - j) for j, x in enumerate(k))) for k in g[f"rew_keys_{e}"]]
        vals = [float(v) for v in g[f"rew_vals_{e}"]]
        if "rbits" in tabs:
            bits = np.unpackbits(tabs["rbits"][e], bitorder="little")[:S ** L]
            assert sorted(np.flatnonzero(bits).tolist()) == sorted(keys), e
        else:
            rt = tabs["rtable"][e]
            assert sorted(np.flatnonzero(rt).tolist()) == sorted(k for k, v in zip(keys, vals) if v != 0.0), e
            assert all(rt[k] == v for k, v in zip(keys, vals)), e
        assert np.array_equal(env.seeded_streams[capi.STREAM_SPACE][e][:4], g["rng_space"][e][:4]), e
    env.close()


def _host_twin(cfg, seeds, **kw):
    return _venv(seeds=seeds, mdps=[_build(cfg, s) for s in seeds], **kw, **cfg)


@pytest.mark.parametrize("rng", ["numpy", "philox"])
@pytest.mark.parametrize("autoreset", ["same_step", "next_step", "disabled"])
@pytest.mark.parametrize("name", ["cfg2", "noise", "s50", "rdist_l1", "diam2"])
def test_device_built_handle_behaves_like_host_built(name, autoreset, rng):
    _compare_with_host_twin(CONFIGS[name], autoreset, rng)


def _compare_with_host_twin(cfg, autoreset, rng):
    """A device-built handle and a host-built one of the same seeds select the same kernels and behave the same."""
    N = 256
    seeds = _seeds(N, salt=7)
    kw = dict(autoreset=autoreset, rng=rng, max_episode_steps=30)
    dev = _venv(seeds=seeds, **kw, **cfg)
    host = _host_twin(cfg, seeds, **kw)
    assert dev.tables_built_on == "device" and host.tables_built_on == "host"
    for K in (64, 1, 8):
        assert dev.rollout_kernel_name(K) == host.rollout_kernel_name(K), K
    A = dev.mdps[0].A
    r = np.random.default_rng(3)
    acts = torch.as_tensor(r.integers(0, A, size=(64, N)).astype(np.int32), device=dev.device)
    a = [x.cpu().numpy() for x in dev.rollout(acts)]
    b = [x.cpu().numpy() for x in host.rollout(acts)]
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    for _ in range(20):
        at = torch.as_tensor(r.integers(0, A, size=N).astype(np.int32), device=dev.device)
        a = [x.cpu().numpy() for x in dev.step(at)[:4]]
        b = [x.cpu().numpy() for x in host.step(at)[:4]]
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    if rng == "numpy":
        oa, _ = dev.reset(seed=123)
        ob, _ = host.reset(seed=123)
        assert np.array_equal(oa.cpu().numpy(), ob.cpu().numpy())
        for st in (capi.STREAM_ENV, capi.STREAM_SPACE):
            assert np.array_equal(dev.get_rng_streams(st)[:, :4], host.get_rng_streams(st)[:, :4]), st
        assert np.array_equal(dev.seeded_streams[capi.STREAM_ENV], host.seeded_streams[capi.STREAM_ENV])
        assert dev.seed(2 ** 40) == 2 ** 40 and host.seed(2 ** 40) == 2 ** 40
        assert np.array_equal(dev.get_rng_streams(capi.STREAM_ENV), host.get_rng_streams(capi.STREAM_ENV))
    sa, sb = dev.get_augmented_state(), host.get_augmented_state()
    assert sa.keys() == sb.keys()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    assert np.array_equal(dev.get_seed_dicts(), host.get_seed_dicts())
    for k in ("P", "is_term", "init_cdf"):
        assert np.array_equal(dev.get_mdp_tables()[k], host.get_mdp_tables()[k]), k
    assert int(dev.status().sum()) == 0 and int(host.status().sum()) == 0
    dev.close()
    host.close()


# L = 5 and the long kernel (L 8 ... 15), several independent sets without maximal connection, the largest state
# space with transition noise, no terminal states
TWINS = {
    "l5": dict(BASE, action_space_size=8, sequence_length=5, reward_density=0.01),
    "l8_rep_rdist": dict(BASE, action_space_size=4, sequence_length=8, repeats_in_sequences=True, reward_density=0.01,
                         terminal_state_density=0, reward_dist=[0.25, 1.0]),
    "l12_rep": dict(BASE, action_space_size=3, sequence_length=12, repeats_in_sequences=True, reward_density=0.001,
                    terminal_state_density=0),
    "l15_rep": dict(BASE, action_space_size=2, sequence_length=15, repeats_in_sequences=True, reward_density=0.01),
    "diam3_not_maxc": dict(BASE, action_space_size=5, diameter=3, maximally_connected=False, sequence_length=3,
                           reward_dist=[0.2, 1.0]),
    "s255_noise": dict(BASE, action_space_size=255, sequence_length=1, reward_density=0.1, transition_noise=0.1),
    "no_term": dict(BASE, action_space_size=8, sequence_length=3, terminal_state_density=0, reward_density=0.1),
}


@pytest.mark.parametrize("rng", ["numpy", "philox"])
@pytest.mark.parametrize("name", sorted(TWINS))
def test_device_built_handle_behaves_like_host_built_beyond_the_short_kernels(name, rng):
    cfg = TWINS[name]
    assert mdp.device_coverage(cfg, [0])[0]
    _compare_with_host_twin(cfg, "same_step", rng)


def _device_family():
    """The Floyd edges and every fifth config of the family, each with 64 ... 512 seeds: cheap host builds get more,
    and no config's tables take much more than 1 GiB."""
    fam = gc.family()
    out = []
    for i, (name, cfg) in enumerate(fam[:len(gc.FLOYD_EDGES)] + fam[len(gc.FLOYD_EDGES)::5]):
        p = mdp.device_gen_params(cfg)
        r = np.random.default_rng(i)
        cheap = p["diameter"] * p["n_sel"] * p["L"] + p["S"] * p["A"] <= 4000
        N = int(np.exp(r.uniform(np.log(64), np.log(513)))) if cheap else 64
        keys = p["S"] ** p["L"]
        per_env = (keys + 7) // 8 if p["unit_rewards"] else 8 * keys
        out.append((name, cfg, max(64, min(N, (1 << 30) // per_env))))
    return out


DEVICE_FAMILY = _device_family()


@pytest.mark.parametrize("name, cfg, N", DEVICE_FAMILY, ids=[f[0] for f in DEVICE_FAMILY])
def test_device_tables_equal_host_builder_on_the_config_family(name, cfg, N):
    seeds = _seeds(N, salt=sum(map(ord, name)))
    env = _venv(seeds=seeds, autoreset="same_step", **cfg)
    assert env.tables_built_on == "device"
    _check_env(env, cfg, seeds, range(N))
    assert int(env.status().sum()) == 0
    env.close()


def _launches(cfg, N):
    per_env = 8 * mdp.device_gen_params(cfg)["scratch_words"]
    chunk = min(N, max(1, mdp.DEVICE_SCRATCH_CAP // per_env))
    return chunk, -(-N // chunk)


def test_device_generation_in_several_launches():
    # 2 028 120 B of scratch per env: 132 envs a launch, 400 envs in launches of 132 + 132 + 132 + 4
    cfg = dict(BASE, action_space_size=64, sequence_length=4, terminal_state_density=0, reward_density=0.001)
    N = 400
    chunk, launches = _launches(cfg, N)
    assert launches >= 3 and N % chunk != 0, (chunk, launches)
    seeds = _seeds(N, salt=11)
    env = _venv(seeds=seeds, autoreset="same_step", **cfg)
    assert env.tables_built_on == "device"
    edges = {k for c in range(launches) for k in (c * chunk, min(N, (c + 1) * chunk) - 1)}
    others = set(np.random.default_rng(2).choice(N, size=16, replace=False).tolist())
    _check_env(env, cfg, seeds, sorted(edges | others))
    assert int(env.status().sum()) == 0
    env.close()


def test_device_generation_one_env_per_launch():
    # 194 MB of scratch per env (a bitset of 200 * 199 * 198 * 197 sequence numbers): every launch holds one env; the
    # reward bits are 200 MB an env, compared key by key
    cfg = dict(BASE, action_space_size=200, sequence_length=4, terminal_state_density=0, reward_density=1e-6)
    N = 3
    assert 8 * mdp.device_gen_params(cfg)["scratch_words"] > mdp.DEVICE_SCRATCH_CAP // 2
    assert _launches(cfg, N) == (1, N)
    seeds = [0, 2 ** 64 - 1, 5874934615388537134]
    env = _venv(seeds=seeds, autoreset="same_step", **cfg)
    assert env.tables_built_on == "device"
    _check_env(env, cfg, seeds, range(N))
    assert int(env.status().sum()) == 0
    env.close()


@pytest.mark.parametrize("name", ["cfg2", "s50"])
def test_device_generation_at_full_size(name):
    cfg = CONFIGS[name]
    N = 65536
    seeds = list(range(10 ** 6, 10 ** 6 + N))
    env = _venv(seeds=seeds, autoreset="same_step", **cfg)
    assert env.tables_built_on == "device"
    idx = sorted(set(np.random.default_rng(5).choice(N, size=2048, replace=False).tolist()) | {0, N - 1})
    _check_env(env, cfg, seeds, idx)
    acts = torch.zeros((8, N), dtype=torch.int32, device=env.device)
    env.rollout(acts)
    assert int(env.status().sum()) == 0
    env.close()


def test_uncovered_config_keeps_host_path_and_lazy_mdps_match():
    irr = dict(BASE, action_space_size=[8, 4], state_space_size=[8, 4], irrelevant_features=True, sequence_length=2)
    env = _venv(seeds=[3, 4, 5], **irr)
    assert env.tables_built_on == "host"
    assert isinstance(env.mdps, list) and env.mdps[1].P_irr is not None
    env.close()
    seeds = _seeds(512, salt=3)
    env = _venv(seeds=seeds, **CFG2)
    assert env.tables_built_on == "device"
    assert len(env.mdps) == len(seeds)
    for i in (0, 1, 7, 100, 511, -1):
        m, h = env.mdps[i], _build(CFG2, seeds[i])
        assert np.array_equal(m.P, h.P) and m.rewardable_sequences == h.rewardable_sequences
        assert np.array_equal(m.space_rng_words, h.space_rng_words) and m.seed_dict == h.seed_dict
    with pytest.raises(IndexError):
        env.mdps[len(seeds)]
    with pytest.raises(AttributeError):
        env.tables_built_on = "host"
    env.close()
