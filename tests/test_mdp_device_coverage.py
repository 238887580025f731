"""Which per-env discrete configs the device generator covers (mdp.device_coverage), and the parameters it is handed
(mdp.device_gen_params) against what mdp.build_mdp itself uses, on every discrete golden case (no GPU)."""
import warnings

import numpy as np
import pytest

import golden_util as gu
from mdp_playground_amd import mdp

BASE = dict(state_space_type="discrete", action_space_type="discrete")


class _Recorder:
    """Stands in for the env generator inside _rewardable_sequences: records every choice() call."""

    def __init__(self, rng, calls):
        self._rng, self._calls = rng, calls

    def choice(self, a, size=None, replace=True, p=None):
        self._calls.append((int(a), int(size), replace, p))
        return self._rng.choice(a, size=size, replace=replace, p=p)


def _build_recording(cfg, monkeypatch):
    calls = []
    orig = mdp._rewardable_sequences
    monkeypatch.setattr(mdp, "_rewardable_sequences", lambda rng, *a: orig(_Recorder(rng, calls), *a))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = mdp.build_mdp(cfg)
    monkeypatch.setattr(mdp, "_rewardable_sequences", orig)
    return m, calls


def _discrete_cases():
    return [n for n in gu.DISCRETE + gu.IMAGE + gu.IRRELEVANT if gu.CASES[n]["seeds"] not in ([None],)]


COVERED = [n for n in _discrete_cases() if mdp.device_coverage(gu.CASES[n]["config"], gu.CASES[n]["seeds"])[0]]


@pytest.mark.parametrize("name", COVERED)
def test_params_equal_what_the_host_builder_uses(name, monkeypatch):
    cfg = dict(gu.CASES[name]["config"])
    seeds = gu.CASES[name]["seeds"]
    p = mdp.device_gen_params(cfg)
    for s in seeds[:4]:
        m, calls = _build_recording({**cfg, "seed": s}, monkeypatch)
        assert (p["S"], p["A"], p["L"], p["diameter"]) == (m.S, m.A, m.sequence_length, m.diameter)
        assert p["n_term"] == len(m.terminal_states) // m.diameter
        # the sequence draws: one choice(total, n_sel, replace=False) (with repeats) or one per independent set
        assert calls == [(p["total"], p["n_sel"], False, None)] * (1 if p["repeats"] else p["diameter"])
        assert mdp._floyd(p["total"], p["n_sel"])
        if not p["repeats"]:
            assert int(np.prod(p["radices"])) == p["total"] and len(p["radices"]) == p["L"]
        full = [v for k, v in m.rewardable_sequences.items() if len(k) == m.sequence_length]
        assert len(full) == p["diameter"] * p["n_sel"]
        assert p["unit_rewards"] == all(v == 1.0 for v in full)
        if p["rews"] is None:
            assert all(v == 1.0 for v in full)
        else:
            assert len(p["rews"]) == p["diameter"] ** 2 * p["n_sel"]
            pool = list(p["rews"])
            for v in full:                       # every value is one of the linspace values, each used once
                pool.remove(v)
        assert np.array_equal(p["is_term"], m.is_terminal_table())
        assert np.array_equal(p["init_cdf"], m.init_cdf())
        assert p["image"] == (m.image is not None)


def test_uncovered_goldens_and_why():
    out = {}
    for name in _discrete_cases():
        ok, why = mdp.device_coverage(gu.CASES[name]["config"], gu.CASES[name]["seeds"])
        if not ok:
            out[name] = why
    tail = "the sequence draw takes choice's tail-shuffle branch"
    assert out == {
        "d_custom_noise": "use_custom_mdp", "d_custom_pr": "use_custom_mdp",
        "d_l8_s5": tail, "d_l9_repeats": tail,
        "d_s300_diam50_l2": "S > 255", "d_s300_noise": "S > 255",
        "i_irr": "irrelevant_features", "d_irr_noise": "irrelevant_features",
        "d_irr_notmax": "irrelevant_features", "d_irr_plain": "irrelevant_features",
    }
    assert len(COVERED) >= 100


FLOYD_TOTAL_10000 = dict(BASE, action_space_size=13, sequence_length=4, repeats_in_sequences=True)   # 10^4 numbers


def _at_scratch_cap(extra):
    """A = 200, L = 4 without repeats: a bitset of ceil(total / 64) words plus n_sel picks, n_sel chosen so the scratch
    is DEVICE_SCRATCH_CAP bytes, plus `extra` picks."""
    total = 200 * 199 * 198 * 197
    n_sel = mdp.DEVICE_SCRATCH_CAP // 8 - -(-total // 64) + extra
    return dict(BASE, action_space_size=200, sequence_length=4, terminal_state_density=0,
                reward_density=(n_sel + 0.5) / total)


@pytest.mark.parametrize("cfg, seeds, why", [
    (dict(BASE, action_space_size=8), [0, 2 ** 64 - 1], ""),
    (dict(BASE, action_space_size=8), [0, 2 ** 64], "a seed is not an int in [0, 2^64)"),
    (dict(BASE, action_space_size=8), [0, -1], "a seed is not an int in [0, 2^64)"),
    (dict(BASE, action_space_size=8), [0, True], "a seed is not an int in [0, 2^64)"),
    (dict(BASE, action_space_size=8), [0, np.int64(3)], "a seed is not an int in [0, 2^64)"),
    (dict(BASE, state_space_type="continuous", state_space_dim=2), [0], "not a discrete env"),
    (dict(BASE, action_space_size=[8, 4], irrelevant_features=True), [0], "irrelevant_features"),
    (dict(BASE, action_space_size=128, diameter=2), [0], "S > 255"),
    (dict(BASE, action_space_size=255), [0], ""),
    (dict(BASE, action_space_size=8, sequence_length=3, reward_dist=[0.2, 1.0]), [0], ""),
    (dict(BASE, action_space_size=8, sequence_length=3, reward_dist=[0.2, 1.0], make_denser=True), [0],
     "reward_dist list with make_denser and sequence_length > 1"),
    (dict(BASE, action_space_size=8, reward_dist=[0.2, 1.0], make_denser=True), [0], ""),
    (dict(BASE, action_space_size=8, reward_dist=lambda rng, d: 1.0), [0],
     "reward_dist is neither None nor a 2-element list"),
    (dict(BASE, action_space_size=16, sequence_length=4, repeats_in_sequences=True), [0],
     "the sequence draw takes choice's tail-shuffle branch"),
    (dict(BASE, action_space_size=16, sequence_length=4, repeats_in_sequences=True, reward_density=0.01), [0], ""),
    # the exact edges of Floyd's branch: a population of 10 000, and n_sel == total // 50 above it
    (FLOYD_TOTAL_10000, [0], ""),
    (dict(BASE, action_space_size=14, sequence_length=4, repeats_in_sequences=True, reward_density=0.02), [0], ""),
    (dict(BASE, action_space_size=14, sequence_length=4, repeats_in_sequences=True, reward_density=0.0201), [0],
     "the sequence draw takes choice's tail-shuffle branch"),
    # generator scratch of exactly the cap, and one pick more
    (_at_scratch_cap(0), [0], ""),
    (_at_scratch_cap(1), [0], "generator scratch per env above the cap"),
])
def test_coverage_rule(cfg, seeds, why):
    assert mdp.device_coverage(cfg, seeds) == (why == "", why)


def test_coverage_rule_edges_are_exact():
    p = mdp.device_gen_params(FLOYD_TOTAL_10000)
    assert p["total"] == 10000 and p["n_sel"] > p["total"] // 50
    for rd, n_sel in ((0.02, 292), (0.0201, 294)):
        p = mdp.device_gen_params(dict(BASE, action_space_size=14, sequence_length=4, repeats_in_sequences=True,
                                       reward_density=rd))
        assert (p["total"], p["n_sel"], p["total"] // 50) == (14641, n_sel, 292)
    assert 8 * mdp.device_gen_params(_at_scratch_cap(0))["scratch_words"] == mdp.DEVICE_SCRATCH_CAP
    assert 8 * mdp.device_gen_params(_at_scratch_cap(1))["scratch_words"] == mdp.DEVICE_SCRATCH_CAP + 8


def test_reward_values_and_unit_flag():
    p = mdp.device_gen_params(dict(BASE, action_space_size=8, sequence_length=1, reward_density=1.0,
                                   reward_dist=[0.5, 1.0]))
    assert not p["unit_rewards"] and p["rews"][-1] == 1.0 and len(p["rews"]) == p["n_sel"] == 6
    p = mdp.device_gen_params(dict(BASE, action_space_size=8, sequence_length=1, reward_density=1.0,
                                   reward_dist=[1.0, 1.0]))
    assert p["unit_rewards"] and p["rews"] is not None
    p = mdp.device_gen_params(dict(BASE, action_space_size=4, sequence_length=1, reward_density=0.1,
                                   reward_dist=[0.5, 1.0]))
    assert p["n_sel"] == 1 and p["rews"] is None and p["unit_rewards"]      # a single value: [1.0]
