"""The reference's own experiment configurations AT SCALE (tests/golden_sweep/cases.json, tools/refgen/gen_sweep.py).

The goldens of the sweep step ONE env per configuration: they pin the arithmetic, on the general kernels (a handful of envs
never selects a specialised one).  A user who switches runs thousands of envs of one MDP -- and then the dispatcher picks
k_discrete_rollout_lean / _quiet / _fast, k_continuous_rollout_fast, k_image_obs_fast / _wide, the one-launch kernels of
mdpp_step ... by the configuration's shape.  Here every configuration of the sweep is run as ONE shared MDP over 1 024 envs
(256 with pictures) on the default dispatch and, beside it, with every specialisation switched off (all MDPP_OPT_NO_* bits:
the general kernels the goldens pin): two fused rollouts, single steps, a rollout again -- every output of every env and
every stream's end state, bit for bit."""
import os

import numpy as np
import pytest
import torch

import golden_util as gu
from test_gpu_boundary import _rand_actions
from test_gpu_parity import _venv

pytestmark = pytest.mark.gpu

SWEEP = sorted(k for k in gu.CASES if "_x" in k and k.rsplit("_x", 1)[-1].isdigit())
KERNELS = {}


def _refused_like_the_reference(cfg, e, seeds=None):
    """A configuration refused at construction: the host restatement of the reference's generator (the MDP and, with pictures,
    the picture templates) refuses it with the same exception -- the library declines nothing the reference accepts."""
    from mdp_playground_amd import image_obs, mdp
    import warnings
    with warnings.catch_warnings(), pytest.raises(type(e)):
        warnings.simplefilter("ignore")
        for c in ([dict(cfg, seed=x) for x in seeds] if seeds is not None else [cfg]):
            m = mdp.build_mdp(c)
            if m.kind == "discrete" and m.image is not None:
                image_obs.build_templates(max(m.S, m.S_irr) if m.irrelevant else m.S, m.image)


def _same(x, y):
    return torch.equal(x.view(torch.int32) if x.dtype.is_floating_point else x, y.view(torch.int32) if y.dtype.is_floating_point else y)


@pytest.mark.parametrize("rng", ["numpy", "philox", "numpy-next_step", "numpy-disabled-timelimit", "numpy-ragged"])
@pytest.mark.parametrize("name", SWEEP)
def test_sweep_config_at_scale_specialised_equals_general(name, rng):
    from mdp_playground_amd import _capi as capi
    cfg = gu.case_config(name)
    image = bool(cfg.get("image_representations"))
    N, F = (256, 24) if image else (1024, 48)
    if "ragged" in rng:                         # (not whole workgroups, a short rollout: the kernels without producer waves)
        N, F = (250, 9) if image else (1000, 9)
    kw = dict(rng="philox", philox_seed=5) if rng == "philox" else {}
    # (gymnasium's next-step autoreset; no autoreset under a TimeLimit of 9 steps: the kernels' other episode-end forms)
    mode = dict(autoreset="next_step") if "next" in rng else dict(autoreset="disabled", max_episode_steps=9) if "disabled" in rng else dict(autoreset="same_step")
    a = _venv(num_envs=N, **mode, **kw, **cfg)
    b = _venv(num_envs=N, **mode, **kw, **cfg)
    b.set_kernel_options(*capi.OPTIONS)
    KERNELS[(name, rng)] = (a.rollout_kernel_name(F), a.rollout_kernel_name(1), b.rollout_kernel_name(F))
    g = np.random.default_rng(11)
    for piece in range(2):
        acts = torch.as_tensor(_rand_actions(a, F, g), device=a.device)
        ra, rb = a.rollout(acts), b.rollout(acts)
        torch.cuda.synchronize()
        assert all(_same(x, y) for x, y in zip(ra, rb)), (name, rng, "rollout", piece, KERNELS[(name, rng)])
        for t in range(6):
            sa, sb = a.step(acts[t]), b.step(acts[t])
            assert all(_same(x, y) for x, y in zip(sa[:4], sb[:4])), (name, rng, "step", piece, t, KERNELS[(name, rng)])
    assert np.array_equal(a.status(), b.status())
    if rng != "philox":
        streams = [capi.STREAM_ENV, capi.STREAM_SPACE] + ([capi.STREAM_IMAGE] if image and a.kind == "discrete" else [])
        for s in streams:
            assert np.array_equal(a.get_rng_streams(s), b.get_rng_streams(s)), (name, s)
    a.close(); b.close()


def test_sweep_selects_the_specialised_kernels():
    """(runs after the cases above) what the dispatcher chose for the reference's configurations: most of them leave the
    general kernels, and every family of specialised kernel is reached by some experiment of the reference."""
    if sum(1 for k in KERNELS if k[1] == "numpy") < len(SWEEP):
        pytest.skip("needs the parametrised cases of this module to have run")
    fused = {k: v[0].split("<")[0] for k, v in KERNELS.items() if k[1] == "numpy"}
    single = {k: v[1].split("<")[0] for k, v in KERNELS.items() if k[1] == "numpy"}
    general = {k: v[2].split("<")[0] for k, v in KERNELS.items() if k[1] == "numpy"}
    assert set(general.values()) <= {"k_discrete_step", "k_continuous_step", "k_image_obs"}, set(general.values())
    special = [k for k in fused if fused[k] != general[k]]
    assert len(special) >= 0.9 * len(fused), (len(special), len(fused))
    fam = set(fused.values()) | set(single.values())
    # (k_discrete_step1, the narrow one-step kernel, is not among them: every discrete experiment file passes reward_noise: 0,
    #  for which the reference still draws rng.normal(0, 0) per step -- rl_toy_env.py:398-403, :1982 -- so the kernels WITH reward
    #  noise are what the reference's sweeps select: lean / quiet <RN=1>, k_discrete_step1w<...,RN=1>, continuous NOISE=1)
    for want in ("k_discrete_rollout_lean", "k_discrete_rollout_quiet", "k_continuous_rollout_fast", "k_image_obs_fast", "k_image_obs_wide",
                 "k_discrete_step1w", "k_continuous_step1", "k_image_step1"):
        assert want in fam, (want, sorted(fam))
    assert all("RN=1" in v[0] for k, v in KERNELS.items() if k[1] == "numpy" and k[0].startswith("d_") and "rollout" in v[0])
    assert all(v[0].startswith("k_continuous_rollout_fast<") for k, v in KERNELS.items() if k[0].startswith("c_") and k[1] in ("numpy", "philox")), "order 3 included (round 5)"
    # (next-step autoreset with noise on numpy streams stays on the general continuous kernel by design: mdpp_capi.hip next_ok)


@pytest.mark.parametrize("rng", ["numpy", "philox"])
@pytest.mark.parametrize("shape", ["s40_l3_unit", "s32_l2_rdist", "s48_l2_unit", "s30_l2_rdist_delay"])
def test_wide_one_step_kernel_without_a_noise_key_at_blob_sizes_past_8_kib(shape, rng):
    """k_discrete_step1w without noise stages 8 rounds of 1 KiB, the upload accepted table blobs of up to
    12 KiB for every handle -- a noise-free handle with a 9-12 KiB blob (S = A = 40, sequence_length 3; S = A = 32,
    sequence_length 2 with reward_dist) read the tail of its reward table and its bucket table from unwritten LDS.  No
    experiment file of the reference has such a shape (they all pass a reward_noise key), so the sweep above never met it.
    mdpp_step() of these shapes against the general kernel, every env, every output, and the streams' end states."""
    from mdp_playground_amd import _capi as capi
    cfg = dict(state_space_type="discrete", action_space_type="discrete", reward_density=0.25, terminal_state_density=0.25,
               make_denser=False, completely_connected=True, repeats_in_sequences=False, generate_random_mdp=True, seed=3)
    cfg.update({"s40_l3_unit": dict(state_space_size=40, action_space_size=40, sequence_length=3, delay=1, reward_density=0.05),
                "s32_l2_rdist": dict(state_space_size=32, action_space_size=32, sequence_length=2, delay=0, reward_dist=[0.01, 1]),
                "s48_l2_unit": dict(state_space_size=48, action_space_size=48, sequence_length=2, delay=2),
                "s30_l2_rdist_delay": dict(state_space_size=30, action_space_size=30, sequence_length=2, delay=3,
                                           reward_dist=[0.01, 1])}[shape])
    kw = dict(rng="philox", philox_seed=9) if rng == "philox" else {}
    N = 1024
    a = _venv(num_envs=N, autoreset="same_step", **kw, **cfg)
    b = _venv(num_envs=N, autoreset="same_step", **kw, **cfg)
    b.set_kernel_options(*capi.OPTIONS)
    assert b.rollout_kernel_name(1).startswith("k_discrete_step<")
    g = np.random.default_rng(5)
    acts = torch.as_tensor(_rand_actions(a, 200, g), device=a.device)
    for t in range(200):
        sa, sb = a.step(acts[t]), b.step(acts[t])
        assert all(_same(x, y) for x, y in zip(sa[:4], sb[:4])), (shape, rng, t, a.rollout_kernel_name(1))
    ra, rb = a.rollout(acts[:40]), b.rollout(acts[:40])
    assert all(_same(x, y) for x, y in zip(ra, rb))
    assert np.array_equal(a.status(), b.status()) and not a.status().any()
    if rng == "numpy":
        for s in (capi.STREAM_ENV, capi.STREAM_SPACE):
            assert np.array_equal(a.get_rng_streams(s), b.get_rng_streams(s))
    a.close(); b.close()


@pytest.mark.parametrize("shape", ["d_s8_rn0", "d_s8_delay_evn_pn", "d_s50_rn0", "d_s24_rdist_rn0", "c_d2_n0", "c_d4_order2_pn0", "c_d2_rn0_only"])
def test_sigma_zero_noise_keys_advance_only_equals_values_formed(shape):
    """Round 6: every experiment file of the reference passes its noise keys with sigma 0, and the reference
    still draws rng.normal(0, 0) per step (rl_toy_env.py:398-403, :1682-1691, :1980-1987) -- the draw's VALUE is multiplied by 0
    (numpy: 0.0 + 0.0 z = +0.0 whatever z is), only the stream's advance is left.  The default dispatch makes the ziggurat's
    accept decisions alone (lean Z0, quiet's skip draw, the continuous walker without its normals ring); MDPP_OPT_NO_SIGMA0
    forms every value as before.  16 384 envs, rollouts of 96 + 40 steps and single steps: every output of every env bit for
    bit, and the end states of the env and space streams (how many words every draw consumed, wedge and tail paths included)."""
    from mdp_playground_amd import _capi as capi
    D = dict(state_space_type="discrete", action_space_type="discrete", reward_density=0.25, terminal_state_density=0.25,
             make_denser=False, completely_connected=True, generate_random_mdp=True, repeats_in_sequences=False, seed=0)
    C = dict(state_space_type="continuous", action_space_type="continuous", inertia=1, state_space_max=10, action_space_max=1,
             target_radius=0.5, make_denser=True, reward_function="move_to_a_point", action_loss_weight=0.01, delay=0, seed=0)
    cfg = {"d_s8_rn0": dict(D, state_space_size=8, action_space_size=8, delay=0, sequence_length=1, transition_noise=0, reward_noise=0),
           "d_s8_delay_evn_pn": dict(D, state_space_size=8, action_space_size=8, delay=3, sequence_length=2, reward_every_n_steps=2,
                                     transition_noise=0.1, reward_noise=0, reward_scale=2.5, reward_shift=-0.5),
           "d_s50_rn0": dict(D, state_space_size=50, action_space_size=50, delay=1, sequence_length=1, transition_noise=0, reward_noise=0),
           "d_s24_rdist_rn0": dict(D, state_space_size=24, action_space_size=24, delay=0, sequence_length=1, reward_dist=[0.01, 1],
                                   reward_noise=0),
           "c_d2_n0": dict(C, state_space_dim=2, action_space_dim=2, transition_dynamics_order=1, time_unit=1.0, target_point=[0, 0],
                           transition_noise=0, reward_noise=0),
           "c_d4_order2_pn0": dict(C, state_space_dim=4, action_space_dim=4, transition_dynamics_order=2, time_unit=0.1,
                                   target_point=[0, 0, 0, 0], transition_noise=0),
           "c_d2_rn0_only": dict(C, state_space_dim=2, action_space_dim=2, transition_dynamics_order=1, time_unit=1.0,
                                 target_point=[1, -1], reward_noise=0, make_denser=False)}[shape]
    N = 16384
    a = _venv(num_envs=N, autoreset="same_step", **cfg)
    b = _venv(num_envs=N, autoreset="same_step", **cfg)
    b.set_kernel_options("NO_SIGMA0")
    name = a.rollout_kernel_name(96)
    if shape.startswith("d_s8") or shape in ("c_d2_n0", "c_d2_rn0_only"):
        assert "Z0=1" in name and "Z0" not in b.rollout_kernel_name(96), name
        assert name.startswith("k_discrete_rollout_lean<" if shape[0] == "d" else "k_continuous_rollout_fast<D=2,"), name
    g = np.random.default_rng(23)
    for piece, F in enumerate((96, 40)):
        acts = torch.as_tensor(_rand_actions(a, F, g), device=a.device)
        ra, rb = a.rollout(acts), b.rollout(acts)
        torch.cuda.synchronize()
        assert all(_same(x, y) for x, y in zip(ra, rb)), (shape, "rollout", piece, name)
        for t in range(4):
            sa, sb = a.step(acts[t]), b.step(acts[t])
            assert all(_same(x, y) for x, y in zip(sa[:4], sb[:4])), (shape, "step", piece, t)
    assert np.array_equal(a.status(), b.status()) and not a.status().any()
    for s in (capi.STREAM_ENV, capi.STREAM_SPACE):
        assert np.array_equal(a.get_rng_streams(s), b.get_rng_streams(s)), (shape, s)
    a.close(); b.close()


def _fuzz_configs(n, seed):
    """Seeded random discrete / continuous configurations around the dispatch conditions of this round's kernel forms (SF: L = 1,
    same-step autoreset, no step limit, every-step pay; XR: reward noise alone; Z0: sigma 0; PE: seeds=[...])."""
    r = np.random.default_rng(seed)
    out = []
    for k in range(n):
        if r.random() < 0.7:
            S = int(r.choice([4, 8, 8, 12, 16, 24, 50, 130]))
            A = int(r.choice([S, max(2, S // 2), min(S, 8)]))
            L = int(r.choice([1, 1, 1, 2, 3]))
            L = 1 if S > 24 else min(L, 2) if S > 12 else L            # (the host generator enumerates S^L sequences, like the reference)
            cfg = dict(state_space_type="discrete", action_space_type="discrete", state_space_size=S, action_space_size=A,
                       sequence_length=L, delay=int(r.choice([0, 0, 1, 2, 5])), reward_density=float(r.choice([0.1, 0.25, 0.5])),
                       terminal_state_density=float(r.choice([0.1, 0.25])), make_denser=bool(r.random() < 0.2),
                       completely_connected=True, generate_random_mdp=True, repeats_in_sequences=False, seed=int(r.integers(1000)))
            if A != S:
                cfg["completely_connected"] = False
            if r.random() < 0.5:
                cfg["reward_noise"] = float(r.choice([0.0, 0.0, 0.3]))
            if r.random() < 0.25:
                cfg["transition_noise"] = float(r.choice([0.0, 0.1]))
            if r.random() < 0.2:
                cfg["reward_every_n_steps"] = int(r.choice([1, 2, L]))
            if r.random() < 0.2:
                cfg["reward_dist"] = [0.01, 1]
            if r.random() < 0.3:
                cfg.update(reward_scale=float(r.choice([1.0, 2.5, -1.5])), reward_shift=float(r.choice([0.0, -0.5])),
                           term_state_reward=float(r.choice([0.0, 1.0])))
        else:
            D = int(r.choice([2, 2, 4, 8, 12]))
            cfg = dict(state_space_type="continuous", action_space_type="continuous", state_space_dim=D, action_space_dim=D,
                       transition_dynamics_order=int(r.choice([1, 1, 2])), inertia=float(r.choice([1.0, 2.0, 3.0])),
                       time_unit=float(r.choice([1.0, 0.1])), state_space_max=10, action_space_max=1, target_point=[0.0] * D,
                       target_radius=float(r.choice([0.5, 2.0])), make_denser=bool(r.random() < 0.7), reward_function="move_to_a_point",
                       delay=int(r.choice([0, 0, 2])), seed=int(r.integers(1000)))
            if r.random() < 0.6:
                cfg["transition_noise"] = float(r.choice([0.0, 0.0, 0.05]))
            if r.random() < 0.6:
                cfg["reward_noise"] = float(r.choice([0.0, 0.0, 0.1]))
        mode = r.choice(["same_step", "same_step", "same_step", "disabled", "next_step", "timelimit"])
        per_env = cfg["state_space_type"] == "discrete" and cfg["state_space_size"] <= 16 and r.random() < 0.3
        out.append((cfg, str(mode), per_env))
    return out


def _same_calls_as_general_kernels(env, cfg, kw, seed, scale=1.0):
    """_check_vs_oracle's calls (a rollout of 72, three single steps, a rollout of 40) on `env` and on a twin handle with every
    specialisation switched off (the general kernels the goldens pin): every output of every env and the status words equal."""
    from mdp_playground_amd import _capi as capi
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        twin = _venv(num_envs=env.num_envs, env_id_offset=env.env_id_offset, **kw, **cfg)
    twin.set_kernel_options(*capi.OPTIONS)
    assert _same(env._obs, twin._obs)
    g = np.random.default_rng(seed)
    for K in (72, 1, 1, 1, 40):
        acts = _rand_actions(env, K, g)
        if scale != 1.0:
            acts = (acts * np.float32(scale)).astype(np.float32)
        at = torch.as_tensor(acts, device=env.device)
        if K == 1:
            ra, rb = env.step(at[0])[:4], twin.step(at[0])[:4]
        else:
            ra, rb = env.rollout(at), twin.rollout(at)
        torch.cuda.synchronize()
        assert all(_same(x, y) for x, y in zip(ra, rb)), (cfg, kw, K, env.rollout_kernel_name(K), twin.rollout_kernel_name(K))
    assert np.array_equal(env.status(), twin.status())
    twin.close()


def _check_vs_oracle(env, k, cfg, mode, kw, seed, scale=1.0, stride=37, calls=(72, 1, 1, 1, 40), flags=None):
    """A fused rollout of 72 steps, three single steps, a rollout of 40 on `env` (or the rollout lengths `calls`: 1 = a single
    step); every `stride`-th env stepped through its own oracle (stride 1: every env).  `flags`, a list, receives (K, the
    [K, N] terminated | truncated flags of every env) per call."""
    from mdp_playground_amd import _capi as capi
    from test_gpu_parity import _oracle_for
    N = env.num_envs
    stride = int(os.environ.get("MDPP_FUZZ_STRIDE", stride))        # (exploration: MDPP_FUZZ_STRIDE=1 -- every lane of every wave)
    auto = kw["autoreset"] == "same_step"
    nextm = kw["autoreset"] == "next_step"        # gymnasium >= 1.0: the call after an episode's last step IS that env's reset()
    philox = env.rng == "philox"
    if philox and nextm:     # (Philox streams are keyed by the BATCH's tick, which also advances on an env's reset call: this per-env loop does not model that)
        return _same_calls_as_general_kernels(env, cfg, kw, seed, scale)
    horizon = kw.get("max_episode_steps", 0)
    disc = env.kind == "discrete"
    init = env._obs.cpu().numpy().copy()
    sample = list(range(3 if stride > 1 else 0, N, stride))
    oracles = []
    for i in sample:
        o = _oracle_for(env, i)
        if philox:       # the build's own counter-based streams, keyed by (seed, global env id): the oracle's C restatement of them
            o.set_philox(int(env._cfg.philox_seed), env.env_id_offset + i)
        else:
            o.set_rng(env.seeded_streams[0][i], env.seeded_streams[1][i])
            if disc and env._irr:
                o.set_rng_irr(env.seeded_streams[capi.STREAM_SPACE_IRR][i])
        assert np.array_equal(np.asarray(o.reset()), init[i]), (k, i)
        oracles.append([o, 0, False])
    g = np.random.default_rng(seed)
    for K in calls:
        acts = _rand_actions(env, K, g)
        if scale != 1.0:
            acts = (acts * np.float32(scale)).astype(np.float32)
        at = torch.as_tensor(acts, device=env.device)
        if K == 1:
            o1, r1, t1, tr1, _ = env.step(at[0])
            obs, rew, term, trunc = (x[None].cpu().numpy() for x in (o1, r1, t1, tr1))
        else:
            obs, rew, term, trunc = (x.cpu().numpy() for x in env.rollout(at))
        if flags is not None:
            flags.append((K, term.astype(bool) | trunc.astype(bool)))
        ends = None if philox else (env.get_rng_streams(capi.STREAM_ENV), env.get_rng_streams(capi.STREAM_SPACE))
        for (o, i), rec in zip(zip([x[0] for x in oracles], sample), oracles):
            for t in range(K):
                if nextm and rec[2]:             # (ignores the action, returns the first observation, reward 0, no flags; draws nothing else)
                    st, rr, d, tr = o.reset(), 0.0, False, False
                    rec[1], rec[2] = 0, False
                    assert not term[t, i] and not trunc[t, i] and rew[t, i] == 0.0, (k, cfg, mode, K, i, t)
                    assert np.array_equal(np.asarray(obs[t, i]).view(np.uint32 if not disc else obs.dtype),
                                          np.asarray(st, dtype=obs.dtype).view(np.uint32 if not disc else obs.dtype)), (k, cfg, mode, K, i, t, "reset call")
                    continue
                if disc:
                    st, rr, d = o.step(acts[t, i])
                else:
                    st, rr, _, d = o.step(acts[t, i])
                rec[1] += 1
                tr = bool(horizon) and rec[1] >= horizon
                if nextm:
                    rec[2] = d or tr
                assert d == bool(term[t, i]) and tr == bool(trunc[t, i]), (k, cfg, mode, K, i, t, env.rollout_kernel_name(K))
                if disc and not philox:
                    assert np.float32(rr) == rew[t, i], (k, cfg, mode, K, i, t, rr, rew[t, i], env.rollout_kernel_name(K))
                else:       # (the line reward: the upstream tolerance -- LAPACK's float32 SVD is not a function of its inputs alone)
                    tol = 1e-5 if isinstance(cfg, dict) and cfg.get("reward_function") == "move_along_a_line" else 1e-6
                    assert abs(float(np.float32(rr)) - float(rew[t, i])) <= tol * max(1.0, abs(rr)), (k, cfg, mode, K, i, t, rr, rew[t, i])
                if auto and (d or tr):
                    st = o.reset(explicit=False)
                    rec[1] = 0
                assert np.array_equal(np.asarray(obs[t, i]).view(np.uint32 if not disc else obs.dtype),
                                      np.asarray(st, dtype=obs.dtype).view(np.uint32 if not disc else obs.dtype)), (k, cfg, mode, K, i, t, env.rollout_kernel_name(K))
            if philox:
                continue
            ge, gs = o.get_rng()
            assert np.array_equal(ge[:4], ends[0][i][:4]) and np.array_equal(gs[:4], ends[1][i][:4]), (k, cfg, mode, K, i, env.rollout_kernel_name(K))
            if disc and env._irr:
                assert np.array_equal(o.get_rng_irr()[:4], env.get_rng_streams(capi.STREAM_SPACE_IRR)[i][:4]), (k, cfg, mode, K, i)


# (env counts: fewer than 8 workgroups, exactly 8 and a multiple of 8 -- the XCD-contiguous block order is on for those only --, 9
#  workgroups, a ragged last workgroup)
_FUZZ_SIZES = tuple(int(x) for x in os.environ["MDPP_FUZZ_SIZES"].split(",")) if "MDPP_FUZZ_SIZES" in os.environ else \
    (1024, 2048, 1000, 4096, 2304, 2048 + 77)
FUZZ = _fuzz_configs(48, 20261004) + _fuzz_configs(96, 777) if "MDPP_FUZZ_SEEDS" not in os.environ else \
    sum((_fuzz_configs(160, int(x)) for x in os.environ["MDPP_FUZZ_SEEDS"].split(",")), [])


@pytest.mark.timeout(120)
@pytest.mark.parametrize("k", range(len(FUZZ)))
def test_random_configurations_specialised_equals_general(k):
    """Round 6: 144 seeded random configurations around the new dispatch conditions (SF / XR / Z0 / PE and their refusals: S = 130,
    L > 1, a step limit, next-step autoreset, transition noise beside reward noise, one MDP per env), each as 1 024 envs on the
    default dispatch beside a handle with every specialisation switched off (the general kernels the goldens pin): two fused
    rollouts of different lengths, single steps in between, every output of every env and both streams' end states.
    (Found with it: a continuous next-step handle with transition noise alone on numpy streams was dispatched to the fused kernel,
    whose walker draws during the reset call -- mdpp_capi.hip `next_ok` tested the discrete field of the config.)"""
    from mdp_playground_amd import _capi as capi
    import warnings
    cfg, mode, per_env = FUZZ[k]
    N = _FUZZ_SIZES[(7 * k + 3) % len(_FUZZ_SIZES)]
    kw = dict(autoreset="same_step")
    if mode == "disabled":
        kw = dict(autoreset="disabled")
    elif mode == "next_step":
        kw = dict(autoreset="next_step")
    elif mode == "timelimit":
        kw = dict(autoreset="same_step", max_episode_steps=11)
    nkw = dict(seeds=list(range(7, 7 + N))) if per_env else dict(num_envs=N)
    cfg = dict(cfg)
    if per_env:
        cfg.pop("seed", None)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            a = _venv(**nkw, **kw, **cfg)
        except (NotImplementedError, ValueError, AssertionError, IndexError, KeyError) as e:      # (a combination the host generator refuses, like the reference: e.g. reward_dist + make_denser, IndexError in both)
            return _refused_like_the_reference(cfg, e, nkw.get("seeds"))
        b = _venv(**nkw, **kw, **cfg)
    b.set_kernel_options(*capi.OPTIONS)
    g = np.random.default_rng(100 + k)
    names = (a.rollout_kernel_name(72), b.rollout_kernel_name(72))
    for piece, F in enumerate((72, 40)):
        acts = torch.as_tensor(_rand_actions(a, F, g), device=a.device)
        ra, rb = a.rollout(acts), b.rollout(acts)
        torch.cuda.synchronize()
        assert all(_same(x, y) for x, y in zip(ra, rb)), (k, cfg, mode, per_env, "rollout", piece, names)
        for t in range(3):
            sa, sb = a.step(acts[t]), b.step(acts[t])
            assert all(_same(x, y) for x, y in zip(sa[:4], sb[:4])), (k, cfg, mode, per_env, "step", piece, t, names)
    assert np.array_equal(a.status(), b.status()), (k, names)
    assert not (a.status() & 0x80000000).any()
    for s in (capi.STREAM_ENV, capi.STREAM_SPACE):
        assert np.array_equal(a.get_rng_streams(s), b.get_rng_streams(s)), (k, cfg, mode, per_env, s, names)
    a.close(); b.close()


@pytest.mark.timeout(180)
@pytest.mark.parametrize("k", range(len(FUZZ)))
def test_random_configurations_default_dispatch_vs_oracle(k):
    """The same random configurations on the DEFAULT dispatch (whatever specialised kernel the library picks: lean Z0, quiet SF /
    XR / PE, the continuous fast kernels ...) against the ORACLE: 512 envs, a fused rollout of 72 steps, three single steps, a rollout
    of 40; every 37th env stepped through its own oracle -- observations and flags bit for bit, rewards as float32 bit patterns
    (continuous float64-path rewards within 1e-6 relative), and both streams' end states after every call."""
    from mdp_playground_amd import _capi as capi
    from test_gpu_parity import _oracle_for
    import warnings
    cfg, mode, per_env = FUZZ[k]
    N = 512
    kw = dict(autoreset="same_step")
    if mode == "disabled":
        kw = dict(autoreset="disabled")
    elif mode == "next_step":
        kw = dict(autoreset="next_step")
    elif mode == "timelimit":
        kw = dict(autoreset="same_step", max_episode_steps=11)
    nkw = dict(seeds=list(range(7, 7 + N))) if per_env else dict(num_envs=N)
    cfg = dict(cfg)
    if per_env:
        cfg.pop("seed", None)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            env = _venv(**nkw, **kw, **cfg)
        except (NotImplementedError, ValueError, AssertionError, IndexError, KeyError) as e:
            return _refused_like_the_reference(cfg, e, nkw.get("seeds"))
    _check_vs_oracle(env, k, cfg, mode, kw, 500 + k)
    assert not (env.status() & 0x80000000).any()
    env.close()


def _fuzz_wide(n, seed):
    """Seeded random configurations of the WIDENED rows: discrete irrelevant features, diameter > 1, repeats
    in sequences, custom P / R matrices, polygon pictures with random transform subsets; continuous relevant subsets, action
    loss, terminal boxes, order 3, the line reward, rendered pictures; grids with and without pictures."""
    r = np.random.default_rng(seed)
    out = []
    for k in range(n):
        fam = str(r.choice(["d_irr", "d_diam", "d_rep", "d_custom", "d_image", "c_wide", "c_wide", "c_line", "c_image", "grid", "grid_image"]))
        base_d = dict(state_space_type="discrete", action_space_type="discrete", delay=int(r.choice([0, 0, 1, 3])),
                      sequence_length=int(r.choice([1, 1, 2, 3])), reward_density=float(r.choice([0.1, 0.25, 0.5])),
                      terminal_state_density=float(r.choice([0.1, 0.25])), seed=int(r.integers(1000)))
        if fam == "d_irr":
            S, S2 = int(r.choice([4, 8, 12])), int(r.choice([3, 5, 10, 16]))
            cfg = dict(base_d, state_space_size=[S, S2], action_space_size=[S, int(r.choice([S2, max(2, S2 // 2)]))], irrelevant_features=True)
        elif fam == "d_diam":
            d = int(r.choice([2, 3]))
            A = int(r.choice([3, 4, 6]))
            cfg = dict(base_d, diameter=d, action_space_size=A, state_space_size=A * d * int(r.choice([1, 1, 2])) if r.random() < 0.5 else A * d,
                       terminal_state_density=float(r.choice([0.25, 0.34])))
        elif fam == "d_rep":
            S = int(r.choice([4, 6, 8]))
            cfg = dict(base_d, state_space_size=S, action_space_size=S, repeats_in_sequences=True, sequence_length=int(r.choice([2, 3, 4])),
                       reward_density=float(r.choice([0.02, 0.05, 0.2])))
        elif fam == "d_custom":
            S, A = int(r.choice([5, 8, 12, 20])), int(r.choice([3, 5, 8]))
            cfg = dict(state_space_type="discrete", action_space_type="discrete", use_custom_mdp=True, state_space_size=S, action_space_size=A,
                       transition_function=r.integers(0, S, size=(S, A)).tolist(), reward_function=np.round(r.normal(size=(S, A)), 3).tolist(),
                       terminal_states=sorted(int(x) for x in r.choice(S, size=max(1, S // 5), replace=False)), delay=int(r.choice([0, 1, 3])),
                       seed=int(r.integers(1000)))
            if r.random() < 0.5 or S != A:          # (without it the reference sizes the default by A and reset() raises, rl_toy_env.py:1003-1018)
                cfg["init_state_dist"] = [0.0 if s in cfg["terminal_states"] else 1.0 / (S - len(cfg["terminal_states"])) for s in range(S)]
        elif fam == "d_image":
            S = int(r.choice([4, 8, 8, 12]))
            W = int(r.choice([32, 64, 84, 100]))
            tr = [t for t in ("shift", "scale", "flip", "rotate") if r.random() < 0.5]
            cfg = dict(base_d, state_space_size=S, action_space_size=S, image_representations=True, image_width=W, image_height=W,
                       image_transforms=",".join(tr) if tr else "none", image_sh_quant=int(r.choice([1, 2, 5])), image_ro_quant=int(r.choice([1, 3, 30])))
            if "scale" in tr:
                cfg["image_scale_range"] = (0.5, float(r.choice([1.0, 1.5])))
        elif fam in ("c_wide", "c_line", "c_image"):
            D = int(r.choice([2, 3, 4, 6, 8, 14]))
            nrel = int(r.integers(2, D + 1))
            rel = sorted(int(x) for x in r.choice(D, size=nrel, replace=False))
            cfg = dict(state_space_type="continuous", action_space_type="continuous", state_space_dim=D, action_space_dim=D,
                       transition_dynamics_order=int(r.choice([1, 1, 2, 3])), inertia=float(r.choice([1.0, 2.0])), time_unit=float(r.choice([1.0, 0.5, 0.1])),
                       state_space_max=float(r.choice([4, 6, 10])), action_space_max=1, delay=int(r.choice([0, 0, 1, 2])), seed=int(r.integers(1000)),
                       reward_scale=float(r.choice([1.0, 1.5])), reward_shift=float(r.choice([0.0, 0.5])))
            if nrel < D:
                cfg.update(relevant_indices=rel, irrelevant_features=True)
            if fam == "c_line":
                cfg.update(reward_function="move_along_a_line", sequence_length=int(r.choice([2, 3, 5, 10, 20])))
            else:
                cfg.update(reward_function="move_to_a_point", target_point=[float(x) for x in np.round(r.uniform(-1, 1, nrel), 2)],
                           target_radius=float(r.choice([0.3, 1.0])), make_denser=bool(r.random() < 0.6))
                if r.random() < 0.5:
                    cfg["action_loss_weight"] = float(r.choice([0.01, 0.5]))
            if r.random() < 0.5:
                cfg.update(terminal_states=[[float(x) for x in np.round(r.uniform(-3, 3, nrel), 1)] for _ in range(int(r.integers(1, 5)))],
                           term_state_edge=float(r.choice([0.5, 1.5])), term_state_reward=float(r.choice([0.0, -1.0])))
            if r.random() < 0.5:
                cfg["transition_noise"] = float(r.choice([0.0, 0.05]))
            if r.random() < 0.5:
                cfg["reward_noise"] = float(r.choice([0.0, 0.1]))
            if fam == "c_image":
                W = int(r.choice([32, 48, 84]))
                cfg.update(image_representations=True, image_width=W, image_height=W, state_space_dim=2, action_space_dim=2,
                           target_point=[0.5, -0.5], reward_function="move_to_a_point")
                cfg.pop("relevant_indices", None); cfg.pop("irrelevant_features", None)
                if "terminal_states" in cfg:
                    cfg["terminal_states"] = [t[:2] if len(t) >= 2 else [t[0], 0.0] for t in cfg["terminal_states"]]
        else:
            G = [int(r.integers(3, 10)), int(r.integers(3, 10))]
            cfg = dict(state_space_type="grid", grid_shape=G, reward_function="move_to_a_point", make_denser=bool(r.random() < 0.5),
                       target_point=[int(r.integers(0, G[0])), int(r.integers(0, G[1]))], seed=int(r.integers(1000)))
            if r.random() < 0.5:
                cfg["terminal_states"] = [[int(r.integers(0, G[0])), int(r.integers(0, G[1]))] for _ in range(int(r.integers(1, 3)))]
            if r.random() < 0.5:
                cfg["transition_noise"] = float(r.choice([0.0, 0.2]))
            if r.random() < 0.5:
                cfg["reward_noise"] = float(r.choice([0.0, 0.1]))
            if r.random() < 0.3:
                cfg["irrelevant_features"] = True
            if fam == "grid_image":
                W = int(r.choice([40, 64, 84]))
                cfg.update(image_representations=True, image_width=W, image_height=W)
        if cfg["state_space_type"] == "discrete" and fam != "d_custom":
            if r.random() < 0.4:
                cfg["reward_noise"] = float(r.choice([0.0, 0.3]))
            if r.random() < 0.3:
                cfg["transition_noise"] = float(r.choice([0.0, 0.15]))
            if r.random() < 0.3:
                cfg.update(reward_scale=float(r.choice([2.5, -1.5])), reward_shift=float(r.choice([0.0, -0.5])), term_state_reward=float(r.choice([0.0, 1.0])))
        mode = str(r.choice(["same_step", "same_step", "same_step", "disabled", "next_step", "timelimit"]))
        rng = str(r.choice(["numpy", "numpy", "philox"]))
        ragged = bool(r.random() < 0.25)
        out.append((fam, cfg, mode, rng, ragged))
    return out


def _fuzz_more(n, seed):
    """A third seeded family, the corners the two above leave out: unbounded state / action boxes (the reset then draws normals,
    rl_toy_env.py:2286), order 4, every-n / delay / terminal reward on continuous envs, pictures WITH an irrelevant sub-space, large
    discrete tables (S up to 1 000, S^L up to 531 441 keys, sequence_length up to 12), grids up to 30 x 40 cells."""
    r = np.random.default_rng(seed)
    out = []
    for k in range(n):
        fam = str(r.choice(["c_unb", "c_order4", "c_evn", "d_image_irr", "d_big", "d_big", "grid_big"]))
        if fam in ("c_unb", "c_order4", "c_evn"):
            D = int(r.choice([2, 3, 4, 6]))
            cfg = dict(state_space_type="continuous", action_space_type="continuous", state_space_dim=D, action_space_dim=D,
                       transition_dynamics_order=int(r.choice([1, 2])), inertia=float(r.choice([1.0, 0.5, 4.0])), time_unit=float(r.choice([1.0, 0.25, 0.01])),
                       state_space_max=float(r.choice([3, 10])), action_space_max=float(r.choice([1, 0.5, 2])), delay=int(r.choice([0, 1, 4])),
                       reward_function="move_to_a_point", target_point=[float(x) for x in np.round(r.uniform(-1, 1, D), 2)],
                       target_radius=float(r.choice([0.2, 1.0])), make_denser=bool(r.random() < 0.5), seed=int(r.integers(1000)))
            if fam == "c_unb":
                if r.random() < 0.7:
                    cfg.pop("state_space_max")
                if r.random() < 0.5:
                    cfg.pop("action_space_max")
            elif fam == "c_order4":
                cfg["transition_dynamics_order"] = int(r.choice([3, 4]))
            else:
                cfg.update(reward_every_n_steps=int(r.choice([2, 3])), term_state_reward=float(r.choice([-1.0, 2.0])),
                           reward_scale=float(r.choice([1.0, -0.5])), reward_shift=float(r.choice([0.0, 1.0])),
                           terminal_states=[[float(x) for x in np.round(r.uniform(-2, 2, D), 1)]], term_state_edge=1.0)
            if r.random() < 0.5:
                cfg["transition_noise"] = float(r.choice([0.0, 0.02]))
            if r.random() < 0.5:
                cfg["reward_noise"] = float(r.choice([0.0, 0.5]))
        elif fam == "d_image_irr":
            S, S2 = int(r.choice([4, 8])), int(r.choice([3, 6, 11]))
            W = int(r.choice([32, 64, 84]))
            tr = [t for t in ("shift", "scale", "flip", "rotate") if r.random() < 0.5]
            cfg = dict(state_space_type="discrete", action_space_type="discrete", state_space_size=[S, S2], action_space_size=[S, S2],
                       irrelevant_features=True, delay=int(r.choice([0, 2])), sequence_length=int(r.choice([1, 2])), seed=int(r.integers(1000)),
                       image_representations=True, image_width=W, image_height=W, image_transforms=",".join(tr) if tr else "none",
                       image_sh_quant=int(r.choice([1, 3, 4])), image_ro_quant=int(r.choice([1, 7])))
            if "scale" in tr:
                cfg["image_scale_range"] = (0.5, 1.5)
        elif fam == "d_big":
            # (S > 255: k_discrete_step_wide; L > 7: k_discrete_step_long -- with repeats, the no-repeats generator needs L <= non-terminal states)
            S, L = [(100, 1), (200, 1), (255, 1), (30, 3), (8, 5), (4, 7), (16, 3), (60, 2), (300, 1), (1000, 1), (300, 2), (4, 9), (3, 12), (256, 1)][int(r.integers(14))]
            cfg = dict(state_space_type="discrete", action_space_type="discrete", state_space_size=S, action_space_size=S, sequence_length=L,
                       delay=int(r.choice([0, 1, 7])), reward_density=float(r.choice([0.05, 0.25])), terminal_state_density=float(r.choice([0.05, 0.25])),
                       make_denser=bool(r.random() < 0.2), seed=int(r.integers(1000)))
            if r.random() < 0.5:
                cfg["reward_noise"] = float(r.choice([0.0, 0.2]))
            if r.random() < 0.3:
                cfg["transition_noise"] = float(r.choice([0.0, 0.05]))
            if r.random() < 0.3:
                cfg["reward_dist"] = [0.01, 1]
            if L > 7:
                cfg["repeats_in_sequences"] = True
        else:
            G = [int(r.integers(10, 31)), int(r.integers(10, 41))]
            cfg = dict(state_space_type="grid", grid_shape=G, reward_function="move_to_a_point", make_denser=bool(r.random() < 0.5),
                       target_point=[int(r.integers(0, G[0])), int(r.integers(0, G[1]))], seed=int(r.integers(1000)),
                       terminal_states=[[int(r.integers(0, G[0])), int(r.integers(0, G[1]))] for _ in range(int(r.integers(0, 4)))])
            if r.random() < 0.5:
                cfg["transition_noise"] = float(r.choice([0.0, 0.3]))
            if r.random() < 0.5:
                cfg["reward_noise"] = float(r.choice([0.0, 0.2]))
            if r.random() < 0.5:
                cfg.update(image_representations=True, image_width=100, image_height=100)
        mode = str(r.choice(["same_step", "same_step", "same_step", "disabled", "next_step", "timelimit"]))
        out.append((fam, cfg, mode, str(r.choice(["numpy", "numpy", "philox"])), bool(r.random() < 0.25)))
    return out


# (MDPP_FUZZ_WIDE_SEEDS=1,2,3 in the environment: an exploration run over other seeds -- tools/fuzz_wide.sh)
FUZZ_WIDE = sum((_fuzz_wide(160, int(x)) for x in os.environ.get("MDPP_FUZZ_WIDE_SEEDS", "606").split(",")), []) + \
    sum((_fuzz_more(64, int(x)) for x in os.environ.get("MDPP_FUZZ_MORE_SEEDS", "17").split(",")), [])


@pytest.mark.timeout(180)
@pytest.mark.parametrize("k", range(len(FUZZ_WIDE)))
def test_random_widened_configurations_specialised_equals_general(k):
    """160 seeded random configurations of the widened rows (irrelevant features, diameter, repeats, custom matrices, polygon
    pictures with random transform subsets, relevant subsets / action loss / terminal boxes / order 3 / line reward / rendered
    pictures, grids), random autoreset mode, random stream kind, a third of them on a ragged batch: default dispatch beside the
    general kernels the goldens pin, every output of every env and every stream's end state.  Actions of the continuous
    families reach 5 % past the action box (the reference's "stay" branch, rl_toy_env.py:1671-1679)."""
    from mdp_playground_amd import _capi as capi
    import warnings
    fam, cfg, mode, rng, ragged = FUZZ_WIDE[k]
    image = bool(cfg.get("image_representations"))
    N, F = (256, 20) if image else (_FUZZ_SIZES[(7 * k + 3) % len(_FUZZ_SIZES)], 48)
    if ragged:
        N, F = (250, 9) if image else (1000, 11)
    kw = dict(autoreset="same_step")
    if mode == "disabled":
        kw = dict(autoreset="disabled")
    elif mode == "next_step":
        kw = dict(autoreset="next_step")
    elif mode == "timelimit":
        kw = dict(autoreset="same_step", max_episode_steps=7)
    if rng == "philox":
        kw.update(rng="philox", philox_seed=77)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            a = _venv(num_envs=N, **kw, **cfg)
        except (NotImplementedError, ValueError, AssertionError, IndexError, KeyError, TypeError) as e:
            return _refused_like_the_reference(cfg, e)
        b = _venv(num_envs=N, **kw, **cfg)
    b.set_kernel_options(*capi.OPTIONS)
    names = (a.rollout_kernel_name(F), a.rollout_kernel_name(1), b.rollout_kernel_name(F))
    g = np.random.default_rng(900 + k)
    for piece in range(2):
        acts = _rand_actions(a, F, g)
        if a.kind == "continuous":
            acts = (acts * np.float32(1.05)).astype(np.float32)
        acts = torch.as_tensor(acts, device=a.device)
        ra, rb = a.rollout(acts), b.rollout(acts)
        torch.cuda.synchronize()
        assert all(_same(x, y) for x, y in zip(ra, rb)), (k, fam, cfg, mode, rng, N, "rollout", piece, names)
        for t in range(4):
            sa, sb = a.step(acts[t]), b.step(acts[t])
            assert all(_same(x, y) for x, y in zip(sa[:4], sb[:4])), (k, fam, cfg, mode, rng, N, "step", piece, t, names)
    assert np.array_equal(a.status(), b.status()), (k, names)
    assert not (a.status() & 0x80000000).any()
    if rng != "philox":
        streams = [capi.STREAM_ENV, capi.STREAM_SPACE] + ([capi.STREAM_IMAGE] if image and a.kind == "discrete" else []) \
            + ([capi.STREAM_SPACE_IRR] if a.kind == "discrete" and a._irr else [])
        for s in streams:
            assert np.array_equal(a.get_rng_streams(s), b.get_rng_streams(s)), (k, fam, cfg, mode, s, names)
    a.close(); b.close()


@pytest.mark.timeout(180)
@pytest.mark.parametrize("k", [k for k in range(len(FUZZ_WIDE)) if FUZZ_WIDE[k][0] in ("d_irr", "d_diam", "d_rep", "d_custom", "c_wide", "c_line", "c_unb", "c_order4", "c_evn", "d_big")
                               ])
def test_random_widened_configurations_default_dispatch_vs_oracle(k):
    """The widened random configurations without pictures, on numpy streams, against the ORACLE on the default dispatch: 512 envs
    (500 on the ragged ones), every 29th env through its own oracle instance -- observations and flags bit for bit, discrete
    rewards as float32 bit patterns, continuous float64-path rewards within 1e-6 relative, every stream's end state after every
    call.  (Found with it: state_space_dim > 12 with transition_dynamics_order 3 / 4 passed mdpp_create and was refused by the
    reset launch -- no kernel of that shape was instantiated.)"""
    import warnings
    fam, cfg, mode, rng, ragged = FUZZ_WIDE[k]
    N = 500 if ragged else 512
    kw = dict(autoreset="same_step")
    if mode == "disabled":
        kw = dict(autoreset="disabled")
    elif mode == "next_step":
        kw = dict(autoreset="next_step")
    elif mode == "timelimit":
        kw = dict(autoreset="same_step", max_episode_steps=7)
    if rng == "philox":
        kw.update(rng="philox", philox_seed=77)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            env = _venv(num_envs=N, **kw, **cfg)
        except (NotImplementedError, ValueError, AssertionError, IndexError, KeyError, TypeError) as e:
            return _refused_like_the_reference(cfg, e)
    _check_vs_oracle(env, k, cfg, mode, kw, 1500 + k, scale=1.05 if env.kind == "continuous" else 1.0, stride=29)
    assert not (env.status() & 0x80000000).any()
    env.close()


_OPS_CASES = [("d", k) for k in range(0, len(FUZZ), 4)] + [("w", k) for k in range(1, len(FUZZ_WIDE), 3)]


@pytest.mark.timeout(240)
@pytest.mark.parametrize("fam,k", _OPS_CASES)
def test_random_operation_sequences_specialised_equals_general(fam, k):
    """Every fourth / third configuration of the two random families under a random SEQUENCE of calls instead of the fixed
    rollout-steps-rollout: fused rollouts of 1 / 2 / 7 / 33 / 130 / 257 steps, runs of single steps, reset() of everything, reset(mask=...)
    of a random third, seed(), a HIP graph of 2-5 captured single steps replayed twice, and a get_augmented_state() -> set_augmented_state() round trip on the specialised handle alone
    (which must change nothing).  After every call: every output of every env against the general kernels; at the end every
    stream's state and the status words."""
    from mdp_playground_amd import _capi as capi
    import warnings
    if fam == "d":
        cfg, mode, per_env = FUZZ[k]
        rng, image = "numpy", False
        N = _FUZZ_SIZES[(5 * k + 1) % len(_FUZZ_SIZES)]
    else:
        _, cfg, mode, rng, ragged = FUZZ_WIDE[k]
        per_env = False
        image = bool(cfg.get("image_representations"))
        N = (250 if ragged else 256) if image else _FUZZ_SIZES[(5 * k + 1) % len(_FUZZ_SIZES)]
    kw = dict(autoreset="same_step")
    if mode == "disabled":
        kw = dict(autoreset="disabled")
    elif mode == "next_step":
        kw = dict(autoreset="next_step")
    elif mode == "timelimit":
        kw = dict(autoreset="same_step", max_episode_steps=9)
    if rng == "philox":
        kw.update(rng="philox", philox_seed=31)
    nkw = dict(seeds=list(range(3, 3 + N))) if per_env else dict(num_envs=N)
    cfg = dict(cfg)
    if per_env:
        cfg.pop("seed", None)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            a = _venv(**nkw, **kw, **cfg)
        except (NotImplementedError, ValueError, AssertionError, IndexError, KeyError, TypeError) as e:
            return _refused_like_the_reference(cfg, e, nkw.get("seeds"))
        b = _venv(**nkw, **kw, **cfg)
    b.set_kernel_options(*capi.OPTIONS)
    g = np.random.default_rng(4000 + k)
    scale = np.float32(1.05) if a.kind == "continuous" else None
    log = []
    for _ in range(9):
        op = str(g.choice(["rollout", "rollout", "rollout", "steps", "reset", "reset_mask", "seed", "state", "graph"]))
        if op == "rollout":
            F = int(g.choice([1, 2, 7, 33, 130, 257] if not image else [1, 2, 7, 19]))
            log.append((op, F))
            acts = _rand_actions(a, F, g)
            acts = torch.as_tensor(acts if scale is None else (acts * scale).astype(np.float32), device=a.device)
            ra, rb = a.rollout(acts), b.rollout(acts)
            torch.cuda.synchronize()
            assert all(_same(x, y) for x, y in zip(ra, rb)), (log, a.rollout_kernel_name(F), fam, k, mode, rng, N, cfg)
        elif op == "steps":
            n = int(g.integers(1, 6))
            log.append((op, n))
            acts = _rand_actions(a, n, g)
            acts = torch.as_tensor(acts if scale is None else (acts * scale).astype(np.float32), device=a.device)
            for t in range(n):
                sa, sb = a.step(acts[t]), b.step(acts[t])
                assert all(_same(x, y) for x, y in zip(sa[:4], sb[:4])), (log, t, a.rollout_kernel_name(1), fam, k, mode, rng, N, cfg)
        elif op in ("reset", "reset_mask"):
            mask = None if op == "reset" else torch.as_tensor(g.random(N) < 0.33)
            log.append((op,))
            oa, ob = a.reset(mask=mask)[0], b.reset(mask=mask)[0]
            assert _same(oa, ob), (log, fam, k, mode, rng, N, cfg)
        elif op == "seed":
            if rng == "philox":
                continue
            sd = int(g.integers(1 << 30))
            log.append((op, sd))
            a.seed(sd); b.seed(sd)
        elif op == "graph":
            # a HIP graph of K captured mdpp_step launches on the specialised handle, replayed twice (new actions written into its
            # action tensor in between), against 2 K step() calls of the general handle
            K = int(g.integers(2, 6))
            acts = _rand_actions(a, 2 * K, g)
            acts = torch.as_tensor(acts if scale is None else (acts * scale).astype(np.float32), device=a.device)
            try:
                sg = a.step_graph(acts[:K].clone())
            except capi.MdppError as e:
                assert "does not replay exactly" in str(e), e
                continue
            log.append((op, K))
            for half in range(2):
                sg.actions.copy_(acts[half * K:(half + 1) * K])
                sg.replay()
                torch.cuda.synchronize()
                for t in range(K):
                    sb = b.step(acts[half * K + t])
                    got = (sg.obs[t], sg.reward[t], sg.terminated[t], sg.truncated[t])
                    assert all(_same(x, y) for x, y in zip(got, sb[:4])), (log, half, t, [bool(_same(x, y)) for x, y in zip(got, sb[:4])], a.rollout_kernel_name(1), fam, k, mode, rng, N, cfg)
            del sg
        else:
            log.append((op,))
            a.set_augmented_state(a.get_augmented_state())
    assert np.array_equal(a.status(), b.status()), (fam, k, log)
    assert not (a.status() & 0x80000000).any()
    if rng != "philox":
        streams = [capi.STREAM_ENV, capi.STREAM_SPACE] + ([capi.STREAM_IMAGE] if image and a.kind == "discrete" else []) \
            + ([capi.STREAM_SPACE_IRR] if a.kind == "discrete" and a._irr else []) + ([capi.STREAM_ACTION] if a.kind == "grid" else [])
        for s in streams:
            assert np.array_equal(a.get_rng_streams(s), b.get_rng_streams(s)), (fam, k, cfg, mode, s, log)
    a.close(); b.close()


@pytest.mark.timeout(180)
@pytest.mark.parametrize("name", [n for n in SWEEP if not gu.CASES[n]["config"].get("image_representations")])
def test_sweep_config_at_scale_default_dispatch_vs_oracle(name):
    """VERDICT r5 (weak 1): the specialised-equals-general comparison above is a self-comparison, and the sweep's goldens step one env
    through the general kernels.  Here every configuration of the reference's experiment files without pictures runs 512 envs of one
    MDP on the DEFAULT dispatch (lean / quiet / fast kernels: whatever a user gets) against the ORACLE: a fused rollout of 72 steps,
    three single steps, a rollout of 40, every 37th env through its own oracle instance from the uploaded streams on -- observations
    and flags bit for bit, rewards as float32 bit patterns (continuous: within 1e-6 relative of the float64 path), both streams'
    end states after every call."""
    import warnings
    cfg = gu.case_config(name)
    kw = dict(autoreset="same_step")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = _venv(num_envs=512, **kw, **cfg)
    _check_vs_oracle(env, name, cfg, "same_step", kw, 77)
    assert not (env.status() & 0x80000000).any()
    env.close()


_PICTURE_CASES = [("sweep", n) for n in SWEEP if gu.CASES[n]["config"].get("image_representations")] + \
                 [("fuzz", k) for k in range(len(FUZZ_WIDE)) if FUZZ_WIDE[k][0] == "d_image"]      # (d_image_irr: test_gpu_parity.py's i_irr cases)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("src,key", _PICTURE_CASES)
def test_pictures_of_fused_rollouts_vs_oracle(src, key):
    """The pictures of the FUSED rollout kernels (k_image_obs_fast / _wide / the general renderer, whatever the dispatch picks) for
    every picture configuration of the reference's experiment files and of the widened random family, against the oracle's draw +
    Pillow-exact rotation restatement: 256 envs without autoreset (no terminal pictures in between: the image stream advances by
    one observation per step), a twin handle without pictures supplies the states; every 5th env, every step, every pixel, and
    the image stream's end state.  (The single-step kernels against the oracle: test_gpu_parity.py test_image_batch_vs_oracle.)"""
    from test_image_oracle import _render
    from mdp_playground_amd import _capi as capi, image_obs, mdp
    import warnings
    cfg = gu.case_config(key) if src == "sweep" else dict(FUZZ_WIDE[key][1])
    N, T = 256, 14
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            env = _venv(num_envs=N, autoreset="disabled", **cfg)
        except (NotImplementedError, ValueError, AssertionError, IndexError, KeyError, TypeError) as e:
            return _refused_like_the_reference(cfg, e)
        twin = _venv(num_envs=N, autoreset="disabled", **{k: v for k, v in cfg.items() if not k.startswith("image_")})
        m = mdp.build_mdp(cfg)
    tpl = image_obs.build_templates(m.S, m.image)
    words = env.get_rng_streams(capi.STREAM_IMAGE).copy()
    acts = torch.as_tensor(_rand_actions(env, T, np.random.default_rng(8)), device=env.device)
    obs, rew, term, trunc = env.rollout(acts)
    sobs, srew, sterm, _ = twin.rollout(acts)
    assert torch.equal(term, sterm) and torch.equal(rew, srew)
    obs, st = obs.cpu().numpy(), sobs.cpu().numpy()
    for i in range(2, N, 5):
        for t in range(T):
            assert np.array_equal(_render(m.image, tpl, int(st[t, i]), words[i]), obs[t, i]), (src, key, t, i, env.rollout_kernel_name(T))
    end = env.get_rng_streams(capi.STREAM_IMAGE)
    assert all(np.array_equal(words[i][:4], end[i][:4]) for i in range(2, N, 5))
    env.close(); twin.close()


_SHARD_CASES = [("d", k) for k in range(2, len(FUZZ), 5)] + [("w", k) for k in range(0, len(FUZZ_WIDE), 4)]


@pytest.mark.timeout(240)
@pytest.mark.parametrize("fam,k", _SHARD_CASES)
def test_random_configurations_two_unequal_shards_equal_one_batch(fam, k):
    """envs are sharded contiguously and every stream is keyed by the GLOBAL env id, so a run's results do not depend on
    how many devices it was split over.  Every fifth / fourth configuration of the two random families as ONE batch of N envs beside
    two handles of 3 N / 8 and 5 N / 8 envs with env_id_offset 0 and 3 N / 8 (different grid sizes, the second shard not starting
    on a workgroup boundary of the whole batch): a rollout, single steps, a rollout -- every output of every env of the two shards
    equal to the whole batch's rows, on the default dispatch."""
    import warnings
    if fam == "d":
        cfg, mode, per_env = FUZZ[k]
        rng, image = "numpy" if k % 2 else "philox", False
    else:
        _, cfg, mode, rng, _ = FUZZ_WIDE[k]
        per_env = False
        image = bool(cfg.get("image_representations"))
    N = 256 if image else 2048
    cut = 3 * N // 8
    kw = dict(autoreset="same_step")
    if mode == "disabled":
        kw = dict(autoreset="disabled")
    elif mode == "next_step":
        kw = dict(autoreset="next_step")
    elif mode == "timelimit":
        kw = dict(autoreset="same_step", max_episode_steps=9)
    if rng == "philox":
        kw.update(rng="philox", philox_seed=31)
    cfg = dict(cfg)
    if per_env:
        cfg.pop("seed", None)
    seeds = list(range(3, 3 + N))

    def make(lo, hi):
        nkw = dict(seeds=seeds[lo:hi]) if per_env else dict(num_envs=hi - lo)
        return _venv(env_id_offset=lo, **nkw, **kw, **cfg)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            whole = make(0, N)
        except (NotImplementedError, ValueError, AssertionError, IndexError, KeyError, TypeError) as e:
            return _refused_like_the_reference(cfg, e, seeds if per_env else None)
        parts = [(0, cut, make(0, cut)), (cut, N, make(cut, N))]
    g = np.random.default_rng(7000 + k)
    assert all(_same(whole._obs[lo:hi], p._obs) for lo, hi, p in parts), (fam, k, "initial observations")
    for piece, F in enumerate((40, 1, 1, 23)):
        acts = _rand_actions(whole, F, g)
        if whole.kind == "continuous":
            acts = (acts * np.float32(1.05)).astype(np.float32)
        acts = torch.as_tensor(acts, device=whole.device)
        if F == 1:
            rw = [x[None] for x in whole.step(acts[0])[:4]]
            rp = [[x[None] for x in p.step(acts[0, lo:hi].contiguous())[:4]] for lo, hi, p in parts]
        else:
            rw = whole.rollout(acts)
            rp = [p.rollout(acts[:, lo:hi].contiguous()) for lo, hi, p in parts]
        torch.cuda.synchronize()
        for (lo, hi, p), r in zip(parts, rp):
            assert all(_same(x[:, lo:hi].contiguous(), y) for x, y in zip(rw, r)), (piece, F, lo, hi, fam, k, mode, rng, whole.rollout_kernel_name(F),
                                                                                    p.rollout_kernel_name(F), cfg)
    st = whole.status()                   # (sticky bits, cleared by the call: read once)
    for lo, hi, p in parts:
        assert np.array_equal(st[lo:hi], p.status()), (fam, k, lo, hi)
        p.close()
    whole.close()


@pytest.mark.timeout(240)
@pytest.mark.parametrize("mode", ["same_step", "next_step", "timelimit"])
@pytest.mark.parametrize("shape", ["s300", "s1000_noise", "s400_l2_rdist", "s300_diam50", "s2000_evn", "s256", "s700_l3_custom_pn", "s300_irr_noise"])
def test_state_spaces_beyond_255_states_vs_oracle(shape, mode):
    """Round 6 (VERDICT r5 missing 5): the reference has no limit on state_space_size (rl_toy_env.py:1050-1151); the device's tables
    and history held states as bytes.  S = 256 ... 65 535 now run on k_discrete_step_wide (16-bit table entries, eight 16-bit history
    fields -- mdpp_discrete_wide.hip; reference goldens d_s300_noise, d_s300_diam50_l2).  Here 512 envs of one MDP against the
    ORACLE, every 37th env, a rollout of 72, single steps, a rollout of 40 -- both noises, delays, sequence_length 2 / 3, reward_dist,
    diameter 50, every-n, a custom P / R matrix pair, the three episode-end modes; then a state round trip into a fresh handle."""
    import warnings
    D = dict(state_space_type="discrete", action_space_type="discrete", reward_density=0.25, terminal_state_density=0.1, seed=5)
    r = np.random.default_rng(3)
    cfg = {"s300": dict(D, state_space_size=300, action_space_size=300, sequence_length=1, delay=0),
           "s256": dict(D, state_space_size=256, action_space_size=256, sequence_length=1, delay=3, reward_noise=0.0),
           "s1000_noise": dict(D, state_space_size=1000, action_space_size=1000, sequence_length=1, delay=2, reward_noise=0.3, transition_noise=0.1,
                               reward_scale=2.0, reward_shift=-0.5, term_state_reward=-1.0),
           "s400_l2_rdist": dict(D, state_space_size=400, action_space_size=400, sequence_length=2, delay=1, reward_density=0.01, reward_dist=[0.01, 1]),
           "s300_diam50": dict(D, state_space_size=300, action_space_size=6, diameter=50, sequence_length=2, delay=0, terminal_state_density=0.34),
           "s300_irr_noise": dict(D, state_space_size=[300, 7], action_space_size=[300, 5], irrelevant_features=True, sequence_length=2, delay=1,
                                  transition_noise=0.1, reward_noise=0.1),
           "s2000_evn": dict(D, state_space_size=2000, action_space_size=2000, sequence_length=1, delay=5, reward_every_n_steps=3, transition_noise=0.0),
           "s700_l3_custom_pn": dict(state_space_type="discrete", action_space_type="discrete", use_custom_mdp=True, state_space_size=700, action_space_size=9,
                                     transition_function=r.integers(0, 700, size=(700, 9)).tolist(), reward_function=np.round(r.normal(size=(700, 9)), 3).tolist(),
                                     terminal_states=[5, 77, 699], init_state_dist=[1.0 / 700] * 700, delay=1, transition_noise=0.05, seed=5)}[shape]
    kw = dict(autoreset="same_step")
    if mode == "next_step":
        kw = dict(autoreset="next_step")
    elif mode == "timelimit":
        kw = dict(autoreset="same_step", max_episode_steps=9)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = _venv(num_envs=512, **kw, **cfg)
    assert env.rollout_kernel_name(72).startswith("k_discrete_step_wide<") and env.rollout_kernel_name(1).startswith("k_discrete_step_wide<")
    _check_vs_oracle(env, shape, cfg, mode, kw, 99)
    # state round trip into a fresh handle: the same next outputs (streams copied too)
    from mdp_playground_amd import _capi as capi
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        twin = _venv(num_envs=512, **kw, **cfg)
    twin.set_augmented_state(env.get_augmented_state())
    for sidx in (capi.STREAM_ENV, capi.STREAM_SPACE) + ((capi.STREAM_SPACE_IRR,) if env._irr else ()):
        twin._put_stream(sidx, env.get_rng_streams(sidx))
    g = np.random.default_rng(8)
    acts = torch.as_tensor(_rand_actions(env, 24, g), device=env.device)
    ra, rb = env.rollout(acts), twin.rollout(acts)
    assert all(_same(x, y) for x, y in zip(ra, rb)), (shape, mode)
    # a captured graph of three single steps on one handle, three step() calls on the other
    try:
        sg = env.step_graph(acts[:3].clone())
    except capi.MdppError as e:
        assert "does not replay exactly" in str(e)
        sg = None
    if sg is not None:
        sg.replay()
        torch.cuda.synchronize()
        for t in range(3):
            sb = twin.step(acts[t])
            assert all(_same(x, y) for x, y in zip((sg.obs[t], sg.reward[t], sg.terminated[t], sg.truncated[t]), sb[:4])), (shape, mode, "graph", t)
    assert not (env.status() & 0x80000000).any()
    env.close(); twin.close()


@pytest.mark.timeout(240)
@pytest.mark.parametrize("mode", ["same_step", "timelimit", "disabled"])
@pytest.mark.parametrize("shape", ["l9_s4_repeats", "l8_s5_rdist", "l15_s3", "l8_s4_noise_delay", "l8_s4_irr"])
def test_sequence_lengths_beyond_7_vs_oracle(shape, mode):
    """Round 6 (VERDICT r5 missing 5): sequence_length 8 ... 15 on k_discrete_step_long (a history of sixteen byte fields --
    mdpp_discrete_long.hip; reference goldens d_l9_repeats, d_l8_s5).  512 envs of one MDP against the ORACLE, every 37th env,
    rollouts and single steps -- repeats, reward_dist, both noises with a delay, L = 15 (3^15 = 14 348 907 sequence keys); then a
    state round trip into a fresh handle.  (The key space stays dense: S^L < 4e9.)"""
    import warnings
    from mdp_playground_amd import _capi as capi
    D = dict(state_space_type="discrete", action_space_type="discrete", terminal_state_density=0.25, seed=7)
    cfg = {"l9_s4_repeats": dict(D, state_space_size=4, action_space_size=4, sequence_length=9, repeats_in_sequences=True, reward_density=0.3, delay=2),
           "l8_s5_rdist": dict(D, state_space_size=5, action_space_size=5, sequence_length=8, repeats_in_sequences=True, reward_density=0.5, delay=0,
                               reward_dist=[0.01, 1]),
           "l15_s3": dict(D, state_space_size=3, action_space_size=3, sequence_length=15, repeats_in_sequences=True, reward_density=0.4, delay=1,
                          terminal_state_density=0.34),
           "l8_s4_irr": dict(D, state_space_size=[4, 6], action_space_size=[4, 3], irrelevant_features=True, sequence_length=8, repeats_in_sequences=True,
                             reward_density=0.5, delay=1, transition_noise=0.1),
           "l8_s4_noise_delay": dict(D, state_space_size=4, action_space_size=4, sequence_length=8, repeats_in_sequences=True, reward_density=0.5, delay=5,
                                     reward_noise=0.2, transition_noise=0.1, reward_scale=-1.5, reward_every_n_steps=2)}[shape]
    kw = dict(autoreset="same_step")
    if mode == "disabled":
        kw = dict(autoreset="disabled")
    elif mode == "timelimit":
        kw = dict(autoreset="same_step", max_episode_steps=23)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            env = _venv(num_envs=512, **kw, **cfg)
        except AssertionError as e:            # (a shape the reference's generator refuses: say so)
            pytest.skip(f"refused at construction: {str(e)[:100]}")
    assert env.rollout_kernel_name(72).startswith("k_discrete_step_long<") and env.rollout_kernel_name(1).startswith("k_discrete_step_long<")
    _check_vs_oracle(env, shape, cfg, mode, kw, 91)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        twin = _venv(num_envs=512, **kw, **cfg)
    twin.set_augmented_state(env.get_augmented_state())
    for sidx in (capi.STREAM_ENV, capi.STREAM_SPACE) + ((capi.STREAM_SPACE_IRR,) if env._irr else ()):
        twin._put_stream(sidx, env.get_rng_streams(sidx))
    acts = torch.as_tensor(_rand_actions(env, 40, np.random.default_rng(8)), device=env.device)
    ra, rb = env.rollout(acts), twin.rollout(acts)
    assert all(_same(x, y) for x, y in zip(ra, rb)), (shape, mode)
    # a captured graph of three single steps on one handle, three step() calls on the other
    try:
        sg = env.step_graph(acts[:3].clone())
    except capi.MdppError as e:
        assert "does not replay exactly" in str(e)
        sg = None
    if sg is not None:
        sg.replay()
        torch.cuda.synchronize()
        for t in range(3):
            sb = twin.step(acts[t])
            assert all(_same(x, y) for x, y in zip((sg.obs[t], sg.reward[t], sg.terminated[t], sg.truncated[t]), sb[:4])), (shape, mode, "graph", t)
    assert not (env.status() & 0x80000000).any()
    env.close(); twin.close()


@pytest.mark.parametrize("shape", ["s1000_both_noises", "l9_s4_both_noises"])
def test_wide_and_long_handles_on_philox_streams_vs_oracle(shape):
    """The wide / long kernels on the build's own Philox streams (transition noise by one word of the tick -- a multiply-shift over
    S - 1 states, here S = 1 000 --, reward noise, resets keyed by the tick) against the oracle's C restatement of those streams:
    1 024 envs, a rollout of 64 with same-step autoreset then 8 single steps, every 11th env."""
    from test_gpu_parity import _oracle_for
    import warnings
    D = dict(state_space_type="discrete", action_space_type="discrete", reward_density=0.25, terminal_state_density=0.1, seed=11)
    cfg = {"s1000_both_noises": dict(D, state_space_size=1000, action_space_size=1000, sequence_length=1, delay=2, transition_noise=0.2, reward_noise=0.3,
                                     reward_scale=1.5),
           "l9_s4_both_noises": dict(D, state_space_size=4, action_space_size=4, sequence_length=9, repeats_in_sequences=True, delay=1,
                                     terminal_state_density=0.25, transition_noise=0.2, reward_noise=0.3)}[shape]
    N, T, T1 = 1024, 64, 8
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = _venv(num_envs=N, autoreset="same_step", rng="philox", philox_seed=99, **cfg)
    assert env.rollout_kernel_name(T).startswith("k_discrete_step_wide<PHILOX=1" if shape[0] == "s" else "k_discrete_step_long<PHILOX=1")
    A = cfg["action_space_size"]
    acts = np.random.default_rng(6).integers(0, A, size=(T + T1, N)).astype(np.int32)
    init = env._obs.cpu().numpy().copy()
    obs, rew, term, trunc = env.rollout(torch.as_tensor(acts[:T], device=env.device))
    obs, rew, term = obs.cpu().numpy(), rew.cpu().numpy(), term.cpu().numpy()
    single = []
    for t in range(T, T + T1):
        o1, r1, d1, _, _ = env.step(torch.as_tensor(acts[t], device=env.device))
        single.append((o1.cpu().numpy().copy(), r1.cpu().numpy().copy(), d1.cpu().numpy().copy()))
    for i in range(0, N, 11):
        o = _oracle_for(env, i)
        o.set_philox(99, i)
        assert o.reset() == int(init[i])
        eo, er, ed, ero = o.rollout(acts[:, i], None)
        exp = eo.copy()
        exp[ed] = ero[ed]
        assert np.array_equal(obs[:, i], exp[:T]) and np.array_equal(term[:, i], ed[:T]), i
        assert np.allclose(rew[:, i], er[:T].astype(np.float32), rtol=1e-6, atol=1e-6), i
        for k, (o1, r1, d1) in enumerate(single):
            assert o1[i] == exp[T + k] and d1[i] == ed[T + k] and np.allclose(r1[i], np.float32(er[T + k]), rtol=1e-6, atol=1e-6), (i, k)
    env.close()


@pytest.mark.parametrize("order,D,horizon", [(3, 14, 7), (4, 14, 0), (3, 20, 0), (4, 20, 7), (2, 30, 7)])
def test_general_continuous_kernel_beyond_12_dimensions_on_philox_streams_vs_oracle(order, D, horizon):
    """Found by the random configurations on Philox streams against the oracle (not by specialised-equals-general: both sides were
    this kernel): k_continuous_step<DMAX=32, OMAX=4, PHILOX> -- 3 KB of scratch per lane -- ended episodes that had not ended, in
    lanes 43-60 of a wave, whenever another lane of the wave ran the in-step reset.  The compiler parks spilled SGPRs in the lanes of
    a VGPR, and where that VGPR is itself spilled inside divergent control flow the inactive lanes' values are lost; the general
    kernels' translation units now spill SGPRs to memory (build.py SPILL_SAFE).  512 envs, every 29th through its own oracle
    (env 119 = lane 55 among them), same-step autoreset with and without a step limit."""
    import warnings
    cfg = dict(state_space_type="continuous", action_space_type="continuous", state_space_dim=D, action_space_dim=D, transition_dynamics_order=order,
               inertia=2.0, time_unit=1.0, state_space_max=6.0, action_space_max=1, delay=1, seed=249, reward_scale=1.0, reward_shift=0.5,
               relevant_indices=[2, 9, 10], irrelevant_features=True, reward_function="move_to_a_point", target_point=[-0.44, -0.53, -0.57],
               target_radius=1.0, make_denser=True, action_loss_weight=0.5)
    kw = dict(autoreset="same_step", rng="philox", philox_seed=77)
    if horizon:
        kw["max_episode_steps"] = horizon
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = _venv(num_envs=512, **kw, **cfg)
    assert env.rollout_kernel_name(72).startswith("k_continuous_step<DMAX=32,")
    _check_vs_oracle(env, (order, D), cfg, "timelimit" if horizon else "same_step", kw, 1509, scale=1.05, stride=29)
    env.close()


_EVERY_LANE = {
    # (kernels of the hot translation units that have VGPR scratch: docs/round6.md section 10)
    "lean_philox_irr": (dict(state_space_type="discrete", action_space_type="discrete", state_space_size=[8, 5], action_space_size=[8, 5], irrelevant_features=True,
                             delay=2, sequence_length=2, seed=5), dict(autoreset="same_step", rng="philox", philox_seed=9), "k_discrete_rollout_lean<"),
    "lean_philox_irr_limit": (dict(state_space_type="discrete", action_space_type="discrete", state_space_size=[8, 5], action_space_size=[8, 5], irrelevant_features=True,
                                   delay=0, sequence_length=3, seed=6), dict(autoreset="same_step", rng="philox", philox_seed=9, max_episode_steps=7), "k_discrete_rollout_lean<"),
    "lean_numpy_both_noises": (dict(state_space_type="discrete", action_space_type="discrete", state_space_size=8, action_space_size=8, delay=4, sequence_length=3,
                                    transition_noise=0.1, reward_noise=0.3, seed=0), dict(autoreset="same_step"), "k_discrete_rollout_lean<"),
    "lean_numpy_both_noises_limit": (dict(state_space_type="discrete", action_space_type="discrete", state_space_size=8, action_space_size=8, delay=2, sequence_length=2,
                                          transition_noise=0.2, reward_noise=0.3, reward_every_n_steps=1, seed=1), dict(autoreset="same_step", max_episode_steps=7), "k_discrete_rollout_lean<"),
    "lean_numpy_rn_only_off": (dict(state_space_type="discrete", action_space_type="discrete", state_space_size=8, action_space_size=8, delay=0, sequence_length=1,
                                    reward_noise=0.5, seed=2), dict(autoreset="disabled"), "k_discrete_rollout_"),
    "lean_numpy_pn_only": (dict(state_space_type="discrete", action_space_type="discrete", state_space_size=6, action_space_size=6, delay=1, sequence_length=3,
                                transition_noise=0.3, seed=3), dict(autoreset="same_step"), "k_discrete_rollout_"),   # (S = 6: the noise thresholds are not row-independent -> quiet)
    "lean_next_irr": (dict(state_space_type="discrete", action_space_type="discrete", state_space_size=[8, 6], action_space_size=[8, 6], irrelevant_features=True,
                           delay=1, sequence_length=2, seed=7), dict(autoreset="next_step", max_episode_steps=9), "k_discrete_rollout_lean<"),
    "quiet_philox_noise": (dict(state_space_type="discrete", action_space_type="discrete", state_space_size=20, action_space_size=20, delay=3, sequence_length=2,
                                transition_noise=0.1, reward_noise=0.2, seed=8), dict(autoreset="same_step", rng="philox", philox_seed=9), "k_discrete_rollout_quiet<"),
    "cfast_philox_noise": (dict(state_space_type="continuous", action_space_type="continuous", state_space_dim=12, action_space_dim=12, relevant_indices=[0, 1, 2, 3],
                                irrelevant_features=True, target_point=[0, 0, 0, 0], target_radius=1.0, state_space_max=1, action_space_max=1,
                                transition_dynamics_order=2, inertia=1, time_unit=1.0, make_denser=True, reward_function="move_to_a_point",
                                transition_noise=0.05, reward_noise=0.05, seed=0), dict(autoreset="same_step", rng="philox", philox_seed=9, max_episode_steps=11), "k_continuous_rollout_fast<"),
    "cfast_d2_sigma0": (dict(state_space_type="continuous", action_space_type="continuous", state_space_dim=2, action_space_dim=2, target_point=[0, 0], target_radius=0.5,
                             state_space_max=10, action_space_max=1, transition_dynamics_order=1, inertia=1, time_unit=1.0, make_denser=True,
                             reward_function="move_to_a_point", transition_noise=0, reward_noise=0, seed=0), dict(autoreset="same_step", max_episode_steps=13), "k_continuous_rollout_fast<"),
    "cfast_d4_order2_both": (dict(state_space_type="continuous", action_space_type="continuous", state_space_dim=4, action_space_dim=4, target_point=[0, 0, 0, 0], target_radius=0.5,
                                  state_space_max=5, action_space_max=1, transition_dynamics_order=2, inertia=2, time_unit=0.5, make_denser=False, delay=2,
                                  reward_function="move_to_a_point", transition_noise=0.05, reward_noise=0.1, seed=1), dict(autoreset="same_step", max_episode_steps=9), "k_continuous_rollout_fast<"),
    "cfast_d8_order3_pn": (dict(state_space_type="continuous", action_space_type="continuous", state_space_dim=8, action_space_dim=8, relevant_indices=[0, 1, 2, 3], irrelevant_features=True,
                                target_point=[0, 0, 0, 0], target_radius=1.0, state_space_max=4, action_space_max=1, transition_dynamics_order=3, inertia=1, time_unit=0.5,
                                make_denser=True, reward_function="move_to_a_point", transition_noise=0.02, seed=2), dict(autoreset="same_step"), "k_continuous_step<DMAX=12,OMAX=4"),   # (general kernel, 36 B of scratch)
    "cfast_numpy_noise_limit": (dict(state_space_type="continuous", action_space_type="continuous", state_space_dim=12, action_space_dim=12, relevant_indices=[0, 1, 2, 3],
                                     irrelevant_features=True, target_point=[0, 0, 0, 0], target_radius=1.0, state_space_max=1, action_space_max=1,
                                     transition_dynamics_order=1, inertia=1, time_unit=1.0, make_denser=True, reward_function="move_to_a_point",
                                     transition_noise=0.05, seed=0), dict(autoreset="same_step", max_episode_steps=9), "k_continuous_rollout_fast<"),
}


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", sorted(_EVERY_LANE))
def test_rollout_kernels_with_register_spills_every_lane_vs_oracle(name):
    """docs/round6.md section 10: the compiler parks spilled SGPRs in VGPR lanes, and a kernel that also spills VGPRs inside divergent control
    flow can lose them -- in particular lanes.  The hand-tuned rollout kernels keep that spilling (it is what makes cfg2 110 us instead of
    157); those of their instantiations that HAVE VGPR scratch are compared here with the oracle on EVERY lane: 512 envs = 8 full
    waves, rollouts with in-step resets (a step limit where episodes would otherwise be long), single steps, both stream kinds.
    The k_continuous_rollout_fast cases also prove that resets diverge inside waves (a target radius large against the state
    space: episodes end at per-env times), the hazard's trigger; every such kernel has its own case in test_gpu_spill_lanes.py."""
    import warnings
    import spill_exposed as sx
    cfg, kw, kernel = _EVERY_LANE[name]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = _venv(num_envs=512, **kw, **cfg)
    assert env.rollout_kernel_name(72).startswith(kernel), env.rollout_kernel_name(72)
    mode = "next_step" if kw["autoreset"] == "next_step" else "timelimit" if kw.get("max_episode_steps") else "same_step"
    ends = []
    _check_vs_oracle(env, name, cfg, mode, kw, 321, stride=1, flags=ends)
    assert not (env.status() & 0x80000000).any()
    env.close()
    if name in ("cfast_philox_noise", "cfast_numpy_noise_limit"):
        sx.assert_resets_diverge(ends, single=False)
