"""The linear policy ES without a GPU: the numpy restatement (tests/linear_es_ref.py) against values worked by hand, and the
interface -- header text, bindings, stream id, build table, the Python object's argument checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import linear_es_ref as ler
from mdp_playground_amd import _capi, build

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mdpp_linear_es_init", "mdpp_step_n_linear_es", "mdpp_step_n_linear_es_summary", "mdpp_linear_es_kernel_name")


def _z(value=0.0):
    """a normals function that hands out `value` for every entry (a callable (env, tick, n) -> array works too) and records
    the keys it was asked for"""
    asked = []

    def normals(seed, env, tick, n):
        asked.append((seed, env, tick, n))
        return np.asarray(value(env, tick, n) if callable(value) else np.full(n, value), F32)
    normals.asked = asked
    return normals


def test_average_ranks_for_ties():
    acc = np.arange(64, dtype=np.float64)
    assert ler.ranks(acc).tolist() == [2 * m - 63 for m in range(64)]
    acc[1] = 0.0                                   # members 0 and 1 tie below everyone: 2 * 0 + 1 - 63 each
    r = ler.ranks(acc)
    assert r[0] == r[1] == -62 and r[2] == -59 and r[63] == 63 and r.sum() == 0
    acc[:] = 7.5                                   # all equal: 2 * 0 + 63 - 63 = 0
    assert ler.ranks(acc).tolist() == [0] * 64


def test_all_equal_scores_leave_the_mean_bit_unchanged():
    rng = np.random.default_rng(0)
    mean = rng.standard_normal(6).astype(F32)
    z0 = rng.standard_normal((32, 6)).astype(F32)
    out = ler.move_mean(mean, F32(0.37), ler.ranks(np.full(64, -3.25)), z0)
    assert np.array_equal(out.view(np.uint32), mean.view(np.uint32))
    # ... and a tie inside a pair cancels: only pair 5 differs from the rest, with equal scores for its two members
    acc = np.zeros(64)
    acc[10] = acc[11] = 9.0
    r = ler.ranks(acc)
    assert r[10] == r[11] == 2 * 62 + 1 - 63 and (np.delete(r, [10, 11]) == 61 - 63).all()
    z0[:] = 0
    z0[5] = 1.0                                    # only pair 5 has a perturbation: +r z and -r z cancel exactly
    assert np.array_equal(ler.move_mean(mean, F32(0.37), r, z0).view(np.uint32), mean.view(np.uint32))


def test_nan_ranks_lowest_and_ties_with_minus_infinity():
    acc = np.arange(64, dtype=np.float64)
    acc[5] = np.nan
    r = ler.ranks(acc)
    assert r[5] == -63 and r[0] == -61 and r[4] == -53 and r[6] == -51 and r[63] == 63
    acc[9] = -np.inf                               # the NaN's key is -inf: the two tie at the bottom
    r = ler.ranks(acc)
    assert r[5] == r[9] == -62 and r[0] == -59


def test_butterfly_order_is_not_left_to_right():
    v = np.zeros(64, F32)
    v[0], v[2], v[3] = 2.0 ** 24, 1.0, 1.0
    left = F32(0)
    for x in v:
        left = F32(left + x)
    assert left == F32(2.0 ** 24)                  # 2^24 + 1 rounds back to 2^24, twice
    b = ler.butterfly(v)
    assert b.dtype == F32 and (b == F32(2.0 ** 24 + 2)).all()     # lanes 2 and 3 meet first: 2^24 + 2 is exact
    assert np.array_equal(b.view(np.uint32), np.full(64, b[0]).view(np.uint32))
    d = ler.butterfly(np.arange(64, dtype=np.float64))
    assert d.dtype == np.float64 and (d == 2016.0).all()


def test_no_fused_multiply_add_in_the_mean_or_the_candidates():
    # gain = S = 1 + 2^-12: the product 1 + 2^-11 + 2^-24 rounds to 1 + 2^-11 and mean = -(1 + 2^-11) makes the sum 0;
    # fma(gain, S, mean) keeps the 2^-24
    w = F32(1 + 2.0 ** -12)
    b = F32(-(1 + 2.0 ** -11))
    r = np.zeros(64, np.int64)
    r[0] = 1
    z0 = np.zeros((32, 1), F32)
    z0[0] = w                                      # S = 1 * w + 0 + ... = w
    assert ler.move_mean([b], w, r, z0).tolist() == [0.0]
    assert ler.move_mean([b], w, r, z0, fma=True).tolist() == [2.0 ** -24]
    r[0], r[1] = 0, 1                              # the odd member: v = 1 * (-z0)
    assert ler.move_mean([b], w, r, z0).tolist() == [float(F32(b - F32(w * w)))]
    # sigma = z = 1 + 2^-12 likewise: mu + t == 0 for the even member, mu - t for the odd one
    z1 = np.zeros((32, 1), F32)
    z1[0] = w
    c = ler.candidates([b], w, z1)
    assert c.shape == (64, 1) and c[0, 0] == 0.0 and c[1, 0] == F32(2) * b and (c[2:, 0] == b).all()
    assert ler.candidates([b], w, z1, fma=True)[0, 0] == F32(2.0 ** -24)


def test_gain_is_lr_over_sigma_times_4032_in_float32():
    sg, lr = F32(0.3), F32(0.7)
    assert ler.gain_of(sg, lr) == F32(lr / F32(sg * F32(4032)))
    assert ler.gain_of(F32(0.5), F32(0)) == 0 and ler.gain_of(np.asarray([1, 2], F32), np.asarray([4032, 4032], F32)).tolist() == [1.0, 0.5]


def _launch(s, reward, term, T=1, next_step=False, pending=None, z=None, info=None):
    K, N = reward.shape
    obs = np.zeros((K, N, 1), F32)
    z = z or _z(0.0)
    out = ler.run_launch(s, np.zeros((N, 1), F32), obs, reward.astype(F32), term.astype(np.uint8), np.zeros((K, N), np.uint8),
                         seed=9, env0=1000, T=T, amax=1.0, next_step=next_step, pending=pending, normals=z, info=info)
    return out + (z,)


def _fresh(mean=0.25, sigma=0.5, lr=0.125, rows=3):
    s = ler.new_state(np.asarray([[[0.0, mean]]], F32), sigma, lr, rows)
    return ler.init(s, seed=9, env0=1000, normals=_z(0.0))


def test_init_draws_the_pairs_from_the_even_members_stream_at_tick_gen():
    s = ler.new_state(np.asarray([[[1.0, 0.25]]], F32), 0.5, 0.125)
    s["gen"][0] = 3
    s["eps"][:] = 7
    s["acc"][:] = 1.0
    z = _z(lambda env, tick, n: [env - 1000, 1.0][:n])
    ler.init(s, seed=9, env0=1000, normals=z)
    assert z.asked == [(9, 1000 + 2 * p, 3, 2) for p in range(32)]
    assert s["cand"][4].reshape(-1).tolist() == [1.0 + 0.5 * 4, 0.75] and s["cand"][5].reshape(-1).tolist() == [1.0 - 0.5 * 4, -0.25]
    assert not s["eps"].any() and not s["acc"].any() and s["gen"][0] == 3


def test_waiting_after_a_generation_that_ends_on_a_reset_call():
    """next-step autoreset, T = 1.  Step 0: every env but env 1 ends its episode (reward 1).  Step 1: their reset call -- not
    counted, reward 100 ignored -- while env 1 ends (5 + 2): the generation ends at this step.  Env 1's step ended an
    episode: it counts from its next episode at once (eps = 0); the others were in a reset call: they wait (eps = -1)."""
    s = _fresh()
    rw = np.zeros((5, 64))
    te = np.zeros((5, 64))
    rw[0], te[0] = 1.0, 1
    rw[0, 1], te[0, 1] = 5.0, 0
    rw[1] = 100.0
    rw[1, 1], te[1, 1] = 2.0, 1
    rw[2] = 3.0                                     # the others' new episode: waiting, not counted; env 1: its reset call
    rw[3] = 4.0
    te[3, 0] = 1                                    # env 0's episode ends: eps -1 -> 0, nothing is added
    rw[4] = 8.0                                     # (env 0: its reset call)
    info = ler.new_info()
    act, s2, pend, ended, z = _launch(s, rw, te, next_step=True, info=info)
    assert ended[:, 0].tolist() == [False, True, False, False, False]
    assert s2["fitness"][1] == 7.0 and (np.delete(s2["fitness"], 1) == 1.0).all()
    assert s2["log_mean"][0, 0] == (63 * 1.0 + 7.0) / 64 and s2["gen"][0] == 1
    assert s2["eps"][1] == 0 and s2["eps"][0] == 0 and (s2["eps"][2:] == -1).all()
    assert s2["ret"][1] == 4.0 + 8.0                # steps 3 and 4 (step 2 was env 1's reset call)
    assert s2["ret"][0] == 0.0 and not s2["ret"][2:].any() and not s2["acc"].any()
    assert pend.tolist() == [False] * 64            # (env 0's reset call was step 4)
    # the keys: tick gen = 0 and tick gen + 1 = 1 of the even members' streams, E = 2 normals each
    assert z.asked == [(9, 1000 + 2 * p, 0, 2) for p in range(32)] + [(9, 1000 + 2 * p, 1, 2) for p in range(32)]
    # waiting env steps: steps 2 and 3, all but env 1 (63 each); step 4, envs 2 .. 63 (env 0 counts again, in its reset call)
    assert info["waiting"] == 63 + 63 + 62 and info["spare"] == 0 and info["non_ties"] == 1 and info["ties"] == 1
    assert s["gen"][0] == 0                         # the input state is left alone


def test_spare_episodes_are_ignored_and_a_member_that_ends_at_the_generation_end_counts_on():
    """same-step autoreset, T = 1.  Env 0 is done after step 0 (reward 1); its episode of steps 1-2 (reward 50 + 50) is spare.
    At step 2 everyone ends: the generation ends, env 0's fitness is still 1, and every member -- env 0 too, whose spare
    episode ended there -- starts counting at once."""
    s = _fresh()
    rw = np.zeros((4, 64))
    te = np.zeros((4, 64))
    rw[0, 0], te[0, 0] = 1.0, 1
    rw[1:3, 0] = 50.0
    rw[0:3, 1:] = 2.0
    te[2] = 1
    rw[3] = 0.5
    info = ler.new_info()
    act, s2, _, ended, _ = _launch(s, rw, te, info=info)
    assert ended[:, 0].tolist() == [False, False, True, False]
    assert s2["fitness"][0] == 1.0 and (s2["fitness"][1:] == 6.0).all()
    assert (s2["eps"] == 0).all() and (s2["ret"] == 0.5).all() and info["spare"] == 2 and info["waiting"] == 0
    # ranks: env 0 lowest (-63), the 63 others tie at 2 * 1 + 62 - 63 = 1; with z = 0 the mean stays and the candidates are the mean
    assert np.array_equal(s2["mean"], s["mean"]) and (s2["cand"][:, 0, 1] == F32(0.25)).all()
    assert (act[:, :, 0] == F32(0.25)).all()


def test_the_mean_moves_by_gain_times_the_rank_weighted_sum_and_the_new_candidates_act_at_once():
    # D = 1, mean b = 0.25, sigma = 0.5, lr = 0.125: gain = 0.125 / (0.5 * 4032).  z0 = 1 for pair 0 and 0 elsewhere; member 0
    # scores 63 (r = 63), member 1 scores 0 with the rest tied at 0 (r = 2 * 0 + 62 - 63 = -1 each): S = 63 * 1 + (-1) * (-1) = 64
    s = ler.new_state(np.asarray([[[0.0, 0.25]]], F32), 0.5, 0.125, 2)
    z = _z(lambda env, tick, n: np.full(n, 1.0 if env == 1000 and tick == 0 else (2.0 if tick == 1 else 0.0)))
    ler.init(s, seed=9, env0=1000, normals=z)
    assert s["cand"][0, 0].tolist() == [0.5, 0.75] and s["cand"][1, 0].tolist() == [-0.5, -0.25] and (s["cand"][2:, 0, 1] == 0.25).all()
    rw = np.zeros((2, 64))
    te = np.zeros((2, 64))
    rw[0, 0] = 63.0
    te[0] = 1
    act, s2, _, ended, _ = _launch(s, rw, te, z=z)
    gain = ler.gain_of(F32(0.5), F32(0.125))
    mu = F32(F32(0.25) + F32(gain * F32(64)))
    assert ended[:, 0].tolist() == [True, False] and s2["mean"][1, 0] == mu and s2["mean"][0, 0] == F32(gain * F32(64))
    assert s2["cand"][6, 0, 1] == F32(mu + F32(1.0)) and s2["cand"][7, 0, 1] == F32(mu - F32(1.0))       # sigma * z1 = 0.5 * 2
    assert act[0, 0, 0] == F32(0.75) and act[1, 0, 0] == F32(1.0) and act[1, 7, 0] == F32(mu - F32(1.0))   # (clipped at amax = 1)
    assert s2["log_mean"][0, 0] == 63.0 / 64 and s2["log_mean"][1, 0] == 0.0


def test_a_nan_member_holds_its_group_and_no_other():
    s = ler.new_state(np.zeros((2, 1, 2), F32), 0.5, 0.125)
    ler.init(s, seed=9, env0=1000, normals=_z(0.0))
    rw = np.ones((3, 128))
    te = np.ones((3, 128))
    te[:, 70] = 0                                   # env 70 (group 1) never ends an episode
    _, s2, _, ended, _ = _launch(s, rw, te)
    assert ended[:, 0].all() and not ended[:, 1].any() and s2["gen"].tolist() == [3, 0]
    assert s2["eps"][70] == 0 and (np.delete(s2["eps"][64:], 6) == 1).all()


def test_the_normals_are_the_oracles_philox_stream_19():
    from oracle import oracle as ora
    z = ler._normals(5, 1002, 2, 7)
    assert z.dtype == F32 and np.array_equal(z, ora.philox_normals(5, 1002, 2, 19, 1, 7)[0].astype(F32))
    assert not np.array_equal(z, ora.philox_normals(5, 1002, 2, 18, 1, 7)[0].astype(F32)) and ler.STREAM == 19


def test_header_binding_and_stream_id():
    src = open(os.path.join(ROOT, "include", "mdpp.h")).read()
    for name in NEW:
        assert name in _capi.EXPORTS, name
        assert re.search(r"\b%s\s*\(mdpp_env \*h" % name, src), name
    assert re.search(r"#define\s+MDPP_ABI_VERSION\s+8\b", src) and _capi.MDPP_ABI_VERSION == 8
    for text in ("Linear policy ES", "the ES needs whole groups of 64 envs", "stream id 19", "k_m = isnan(acc) ? -inf : acc",
                 "rank2_m = 2 #{j : k_j < k_m} + #{j != m : k_j == k_m}", "r_m = rank2_m - 63",
                 "v = v + shfl_xor(v, 1 << k)", "mu = mean[e][g] + gain[g] * S", "t = sigma[g] * z1[e]",
                 "cand_m[e] = s_m > 0 ? mu + t : mu - t", "env_id_offset + 64g + 2p", "lr / (sigma * 4032)",
                 "A linear policy ES (mdpp_step_n_linear_es / _summary)"):
        assert text in src, text
    internal = open(os.path.join(build.CSRC, "mdpp_internal.hpp")).read()
    assert re.search(r"kPhiloxLinearEsStream\s*=\s*19\b", internal) and re.search(r"kPhiloxLinearSearchStream\s*=\s*18\b", internal)
    assert sorted(_capi.OPTIONS.values()) == [1 << k for k in range(24)]                    # no new option bit
    m = re.search(r"typedef struct mdpp_linear_es \{(.*?)\} mdpp_linear_es;", src, re.S)
    fields = [f.strip().lstrip("*") for decl in m.group(1).split(";") if decl.strip() for f in decl.strip().split(None, 1)[1].split(",")]
    assert fields == [f for f, _ in _capi.MdppLinearEs._fields_]
    assert fields[:9] == list(ler.ARRAYS)
    assert C.sizeof(_capi.MdppLinearEs) == 9 * 8 + 8 + 4 + 4


def test_build_table_has_both_units_with_default_flags():
    for u in ("mdpp_continuous_es.hip", "mdpp_continuous_summary_es.hip"):
        assert u in build.SOURCES and u not in build.EXTRA_FLAGS
        assert "mdpp_continuous_closed.hpp" in build.INCLUDED_SOURCES[u]
        assert os.path.exists(os.path.join(build.CSRC, u))
    assert "mdpp_continuous_es.hip" in build.INCLUDED_SOURCES["mdpp_continuous_summary_es.hip"]
    assert len(set(build.SOURCES)) == len(build.SOURCES)
    unit = open(os.path.join(build.CSRC, "mdpp_continuous_es.hip")).read()
    # the cross-lane work: ballots and shuffles; no LDS traffic of its own, no barrier, no inline assembly
    assert "__all(" in unit and "__shfl(" in unit and unit.count("__shfl_xor(") == 2
    assert "__syncthreads" not in unit and "asm" not in unit and "atomic" not in unit.replace("no atomics", "")
    body = open(os.path.join(build.CSRC, "mdpp_continuous_closed.hpp")).read()
    assert body.count("agent.observe(rw, done || truncated);") == 1 and "vote" not in body     # the shared step has no new hook


def test_built_library_exports_the_entry_points_and_refuses_a_null_handle():
    lib = _capi.load()
    assert len(lib.mdpp_step_n_linear_es.argtypes) == 9 and len(lib.mdpp_step_n_linear_es_summary.argtypes) == 9
    assert len(lib.mdpp_linear_es_kernel_name.argtypes) == 3 and len(lib.mdpp_linear_es_init.argtypes) == 3
    buf = (C.c_float * 8)()
    p = C.cast(buf, C.c_void_p)
    s = _capi.MdppLinearEs()
    assert lib.mdpp_linear_es_init(None, C.byref(s), None) == -1
    assert lib.mdpp_step_n_linear_es(None, 1, C.byref(s), p, p, p, p, p, None) == -1
    assert lib.mdpp_step_n_linear_es_summary(None, 1, C.byref(s), p, p, p, p, p, None) == -1
    assert lib.mdpp_linear_es_kernel_name(None, 1, 0) == b""


def test_python_object_checks_its_arguments_before_any_device_work():
    import torch
    from mdp_playground_amd.linear_es import LinearES
    th = torch.zeros((3, 2, 3), dtype=torch.float32)
    th[:, 0, 2] = torch.arange(3)
    s = LinearES(th, 0.25, 0.5, seed=3, episodes_per_member=2, log_generations=4)
    assert (s.groups, s.num_envs, s.D) == (3, 192, 2)
    assert tuple(s.mean.shape) == (6, 3) and s.mean[2].tolist() == [0, 1, 2] and torch.equal(s.mean_theta(), th)
    assert s.sigma.tolist() == [0.25] * 3 and s.gen.dtype == torch.int32 and tuple(s.log_mean.shape) == (4, 3)
    assert s.gain.numpy().tolist() == [float(ler.gain_of(F32(0.25), F32(0.5)))] * 3
    assert tuple(s.acc.shape) == tuple(s.fitness.shape) == tuple(s.eps.shape) == (192,) and s.fitness.dtype == torch.float64
    c = s.c_struct()
    assert (c.mean, c.eps, c.log_mean, c.seed, c.episodes_per_member, c.log_rows) == (s.mean.data_ptr(), s.eps.data_ptr(), s.log_mean.data_ptr(), 3, 2, 4)
    assert LinearES(th, 0.25, 0.5, seed=3).c_struct().log_mean is None           # M = 0: a null pointer
    s.check(192, 2, th.device, "t")
    with pytest.raises(ValueError):
        s.check(128, 2, th.device, "t")
    s.gen[:] = torch.tensor([2, 0, 9], dtype=torch.int32)
    rows, valid = s.curve()
    assert tuple(rows.shape) == (4, 3) and valid.tolist() == [2, 0, 4]
    d = s.state_dict()
    s2 = LinearES(torch.ones((3, 2, 3), dtype=torch.float32), 1.0, 1.0, seed=0, log_generations=4)
    s2.load_state_dict(d)
    assert all(torch.equal(x, y) for x, y in zip(s.tensors(), s2.tensors())) and (s2.seed, s2.episodes_per_member) == (3, 2)
    sg = np.asarray([0.5, 1, 2], F32)
    es = LinearES(th, sg, np.asarray([0, 1, 2], F32), seed=1)
    assert es.sigma.tolist() == sg.tolist() and es.gain.numpy().tolist() == ler.gain_of(sg, np.asarray([0, 1, 2], F32)).tolist()
    for bad in (dict(sigma=0.0), dict(sigma=-0.1), dict(sigma=np.nan), dict(sigma=np.inf), dict(sigma=sg.astype(np.float64)),
                dict(sigma=sg[:2]), dict(sigma=np.asarray([1, 0, 1], F32)), dict(lr=-0.5), dict(lr=np.inf), dict(lr=np.nan),
                dict(lr=np.asarray([1, -1, 1], F32)), dict(episodes_per_member=0), dict(episodes_per_member=1.5),
                dict(log_generations=-1), dict(seed=-1), dict(seed=2 ** 64)):
        kw = dict(dict(sigma=0.1, lr=0.1, seed=1), **bad)
        with pytest.raises(ValueError):
            LinearES(th, kw.pop("sigma"), kw.pop("lr"), **kw)
    for bad_theta in (th.double(), th[:, :, :2], th[0], th.numpy()):
        with pytest.raises(ValueError):
            LinearES(bad_theta, 0.1, 0.1, seed=1)
