"""The closed-loop agents' LDS placement (mdpp_discrete_closed.hpp: closed_agent_lds, the one rule of the learner and
evaluation launchers) built for the host through tests/closed_lds_host_shim.hip and called on hand-filled handles (no GPU).

The rule, restated here from its statement.  Candidates: the agent's Q-tables, the envs' MDP slots, the per-level cdfs.
The subsets are tried in the order {Q, slots, cdfs}, {Q, slots}, {Q, cdfs}, {Q}, {slots, cdfs}, {slots}, {cdfs}, {}; a subset
that holds a candidate which does not exist or is not allowed is skipped; {} is taken without asking the device.
  Q      q_lds != 0, q_lds <= 160 KiB, not under NO_LEARN_LDS
  slots  one MDP per env (pm) only: rew_in_lds, 256 lds_noise <= 64 KiB, not under NO_PM_LDS
  cdfs   per-env noise levels, numpy streams and a transition-noise key only: <= 32 KiB, not under NO_NLEV_LDS (shared MDP)
         / NO_PM_NLEV_LDS (pm)
  bytes  the chosen candidates + lds_bytes (shared MDP) / lds_bytes - lds_noise (pm, no levels) / 0 (pm with levels)"""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import pytest

import closed_forms_shape_cases as forms
import closed_loop_shape_cases as shp
import noise_seed_cases as nsc
from mdp_playground_amd import _capi as capi
from mdp_playground_amd import build as hipbuild

SHIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "closed_lds_host_shim.hip")
KIB = 1024
LIMIT = 160 * KIB                    # a workgroup's LDS on gfx950
ORDER = [(1, 1, 1), (1, 1, 0), (1, 0, 1), (1, 0, 0), (0, 1, 1), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
OPT = {k: capi.OPTIONS[k] for k in ("NO_LEARN_LDS", "NO_NLEV_LDS", "NO_PM_LDS", "NO_PM_NLEV_LDS")}
MODES = {"shared": dict(pm=0, nl_on=0), "shared_levels": dict(pm=0, nl_on=1), "pm": dict(pm=1, nl_on=0), "pm_levels": dict(pm=1, nl_on=1)}


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    hipcc = shutil.which(hipbuild._hipcc())
    if hipcc is None:
        pytest.skip("no hipcc: the placement cannot be built for the host")
    so = str(tmp_path_factory.mktemp("closed_lds_host_shim") / "closed_lds_host_shim.so")
    subprocess.run([hipcc] + hipbuild.FLAGS + ["-shared", SHIM, "-o", so], check=True)
    lib = C.CDLL(so)
    i32, u32, u64 = C.c_int, C.c_uint32, C.c_uint64
    lib.closed_lds_host.argtypes = [i32, u64, u32, u32, i32, i32, i32, u32, i32, i32, i32, u64, C.POINTER(u64), C.POINTER(i32)]
    lib.closed_lds_host.restype = i32
    return lib


def handle(pm=0, q_lds=64 * KIB, lds_bytes=720, lds_noise=208, rew_in_lds=1, philox=0, has_p_noise=1, opts=0, nl_on=0, levels=5, S=8):
    """what the rule reads of a handle; the default is 8 x 8 with unit rewards and both noise keys"""
    return dict(pm=pm, q_lds=q_lds, lds_bytes=lds_bytes, lds_noise=lds_noise, rew_in_lds=rew_in_lds, philox=philox,
                has_p_noise=has_p_noise, opts=opts, nl_on=nl_on, levels=levels, S=S)


def call(lib, h, budget):
    """-> (the calls of granted [(q, slots, cdfs, bytes)], the subset chosen (q, slots, cdfs))"""
    asked, n = (C.c_uint64 * 32)(), C.c_int(0)
    got = lib.closed_lds_host(h["pm"], h["q_lds"], h["lds_bytes"], h["lds_noise"], h["rew_in_lds"], h["philox"], h["has_p_noise"],
                              h["opts"], h["nl_on"], h["levels"], h["S"], budget, asked, C.byref(n))
    assert 0 <= n.value <= 7, n.value
    return [tuple(asked[4 * k:4 * k + 4]) for k in range(n.value)], (got >> 2 & 1, got >> 1 & 1, got & 1)


def sizes(h):
    return h["q_lds"], 256 * h["lds_noise"], (h["levels"] * h["S"] * h["S"] * 8 + 15) // 16 * 16


def allowed(h):
    q, slots, cdf = sizes(h)
    return (q != 0 and q <= 160 * KIB and not h["opts"] & OPT["NO_LEARN_LDS"],
            bool(h["pm"]) and bool(h["rew_in_lds"]) and slots <= 64 * KIB and not h["opts"] & OPT["NO_PM_LDS"],
            bool(h["nl_on"]) and not h["philox"] and bool(h["has_p_noise"]) and cdf <= 32 * KIB
            and not h["opts"] & OPT["NO_PM_NLEV_LDS" if h["pm"] else "NO_NLEV_LDS"])


def fixed(h):
    return h["lds_bytes"] if not h["pm"] else 0 if h["nl_on"] else h["lds_bytes"] - h["lds_noise"]


def expected(h, budget):
    ok, size, asked = allowed(h), sizes(h), []
    for sub in ORDER:
        if any(s and not o for s, o in zip(sub, ok)):
            continue
        if sub == (0, 0, 0):
            break
        asked.append(sub + (fixed(h) + sum(b for s, b in zip(sub, size) if s),))
        if asked[-1][3] <= budget:
            return asked, sub
    return asked, (0, 0, 0)


def check(lib, h, budget):
    asked, chosen = call(lib, h, budget)
    assert (asked, chosen) == expected(h, budget), (h, budget)
    assert all(a[:3] != (0, 0, 0) for a in asked), (h, asked)          # the empty set is never asked for
    # the subset chosen is the first in ORDER that is allowed and granted -- and every one before it was asked and refused
    ok = allowed(h)
    before = [s for s in ORDER[:ORDER.index(chosen)] if all(o or not x for x, o in zip(s, ok))]
    assert [a[:3] for a in asked] == before + ([chosen] if chosen != (0, 0, 0) else [])
    assert all(a[3] > budget for a in asked[:len(before)]) and (chosen == (0, 0, 0) or asked[-1][3] <= budget)
    return asked, chosen


# each candidate allowed, switched off by its option, by the other mode's option (which must not count), and at / beyond its bound
Q_WAYS = [dict(), dict(opts=OPT["NO_LEARN_LDS"]), dict(q_lds=0), dict(q_lds=160 * KIB), dict(q_lds=160 * KIB + 1024)]
SLOT_WAYS = [dict(), dict(opts=OPT["NO_PM_LDS"]), dict(rew_in_lds=0), dict(lds_noise=256), dict(lds_noise=272)]
CDF_WAYS = [dict(), dict(opts=OPT["NO_NLEV_LDS"]), dict(opts=OPT["NO_PM_NLEV_LDS"]), dict(philox=1), dict(has_p_noise=0),
            dict(S=32, levels=4), dict(S=29, levels=5)]


@pytest.mark.parametrize("mode", sorted(MODES))
def test_the_grid_of_allowed_candidates_and_budgets(shim, mode):
    assert (4 * 32 * 32 * 8, 5 * 29 * 29 * 8) == (32 * KIB, 33640) and 256 * 256 == 64 * KIB < 256 * 272
    seen, cases = set(), 0
    for qw, sw, cw in itertools.product(Q_WAYS, SLOT_WAYS, CDF_WAYS):
        h = handle(**MODES[mode])
        for w in (qw, sw, cw):
            h.update({k: v for k, v in w.items() if k != "opts"})
            h["opts"] |= w.get("opts", 0)
        h["lds_bytes"] = h["lds_noise"] + (h["S"] * h["S"] * 8 + 15) // 16 * 16        # (the carve: the handle's own cdf behind a lane's slot)
        size, fx = sizes(h), fixed(h)
        sums = sorted({fx + sum(b for s, b in zip(sub, size) if s) for sub in ORDER})
        for budget in sorted({0, 1 << 40} | {s + d for s in sums for d in (-1, 0) if s + d >= 0}):
            _, chosen = check(shim, h, budget)
            seen.add(chosen)
            cases += 1
    exists = (1, MODES[mode]["pm"], MODES[mode]["nl_on"])
    assert seen == {s for s in ORDER if all(e or not x for x, e in zip(s, exists))}, (mode, seen)      # every subset of the mode was reached
    assert cases >= 175 * 4


def test_the_modes_differ_in_the_fixed_bytes_and_the_cdfs_option(shim):
    big = 1 << 40
    assert call(shim, handle(), big) == ([(1, 0, 0, 720 + 64 * KIB)], (1, 0, 0))
    assert call(shim, handle(nl_on=1), big) == ([(1, 0, 1, 720 + 64 * KIB + 2560)], (1, 0, 1))
    assert call(shim, handle(pm=1), big) == ([(1, 1, 0, 512 + 64 * KIB + 256 * 208)], (1, 1, 0))
    assert call(shim, handle(pm=1, nl_on=1), big) == ([(1, 1, 1, 64 * KIB + 256 * 208 + 2560)], (1, 1, 1))
    assert call(shim, handle(nl_on=1, opts=OPT["NO_PM_NLEV_LDS"]), big)[1] == (1, 0, 1)
    assert call(shim, handle(nl_on=1, opts=OPT["NO_NLEV_LDS"]), big)[1] == (1, 0, 0)
    assert call(shim, handle(pm=1, nl_on=1, opts=OPT["NO_NLEV_LDS"]), big)[1] == (1, 1, 1)
    assert call(shim, handle(pm=1, nl_on=1, opts=OPT["NO_PM_NLEV_LDS"]), big)[1] == (1, 1, 0)
    # nothing allowed, or nothing granted: {} without a question, or after every allowed subset was refused
    assert call(shim, handle(pm=1, nl_on=1, opts=sum(OPT.values())), big) == ([], (0, 0, 0))
    asked, chosen = call(shim, handle(pm=1, nl_on=1), 0)
    assert chosen == (0, 0, 0) and [a[:3] for a in asked] == ORDER[:7]


# ---- agreement with the placements the case modules restate, at their own worked examples
def _budget(static, limit=LIMIT):
    """dynamic_lds_ok as a budget: up to 32 KiB of dynamic LDS is never asked about"""
    return max(32 * KIB, limit - static)


def _of_cfg(cfg, double, rng="numpy", options=(), **mode):
    """the handle of a case module's config: the carve of closed_loop_shape_cases.lds_bytes, a lane's slot without the noise cdf"""
    S = shp.shape_of(cfg)[0]
    return handle(q_lds=shp.q_lds(cfg, double), lds_bytes=shp.lds_bytes(cfg), lds_noise=forms.lane_bytes(cfg), philox=int(rng == "philox"),
                  has_p_noise=int("transition_noise" in cfg), opts=sum(OPT[o] for o in options), S=S, **mode)


def test_agrees_with_noise_seed_cases_placement(shim):
    budget = nsc.LDS_BYTES - nsc.ZIG_BYTES
    runs = [(nsc.TABULAR, "q_learning", "numpy", ()), (nsc.TABULAR, "double_q", "numpy", ()), (nsc.S20, "q_learning", "numpy", ()),
            (nsc.S29, "sarsa", "numpy", ()), (nsc.RDIST, "sarsa", "philox", ()), (nsc.CFG2, "q_learning", "numpy", ()),
            (nsc.TABULAR, "q_learning", "numpy", ("NO_NLEV_LDS",))]
    runs += [(nsc.TABULAR, "q_learning", "numpy", tuple(o for o, on in zip(("NO_LEARN_LDS", "NO_PM_LDS", "NO_PM_NLEV_LDS"), bits) if on))
             for bits in itertools.product((0, 1), repeat=3)]
    for cfg, algo, rng, options in runs:
        h = _of_cfg(dict(cfg, **nsc.CREATED), algo == "double_q", rng, options, pm=1, nl_on=1)
        asked, (q, m, c) = check(shim, h, budget)
        assert (q, 2 if m else 1, bool(c), asked[-1][3] if q or m or c else 0) == nsc.placement(cfg, algo, rng, *options), (cfg, algo, rng, options)


def test_agrees_with_closed_forms_shape_cases_at_the_bounds_worked_by_hand(shim):
    s10, s11, s12, d4 = (forms.CASES[c] for c in ("s10", "s11", "s12", "d4_s24_a6"))
    noisy = dict(s10, **forms.CREATED)
    # one MDP per env, no levels: (QLDS, PM)
    for cfg, limit, options in [(s11, LIMIT, ()), (s11, LIMIT, ("NO_LEARN_LDS",)), (s11, LIMIT, ("NO_LEARN_LDS", "NO_PM_LDS")), (s12, LIMIT, ()),
                                (s12, LIMIT, ("NO_LEARN_LDS",)), (s10, LIMIT, ()), (noisy, LIMIT, ()), (noisy, LIMIT + 2848, ()), (noisy, LIMIT + 2847, ()),
                                (dict(s10, reward_noise=0.5), LIMIT, ())] + [(forms.CASES[c], LIMIT, ()) for c in forms.DOUBLE_PM2]:
        for double in (False, True):
            static = forms.ZIG_BYTES if "transition_noise" in cfg or "reward_noise" in cfg else 24
            _, (q, m, c) = check(shim, _of_cfg(cfg, double, options=options, pm=1), _budget(static, limit))
            assert (q, 2 if m else 1) == forms.pm_expected(cfg, double, limit, options) and not c, (cfg, limit, options, double)
    # ... with levels: (QLDS, PM, cdfs staged); a shared MDP with levels: (QLDS, cdfs staged)
    for cfg, rng, options in [(s10, "numpy", ()), (s10, "philox", ()), (s10, "numpy", ("NO_LEARN_LDS",)), (s12, "numpy", ()), (s12, "philox", ("NO_PM_LDS",)),
                              (d4, "numpy", ()), (d4, "numpy", ("NO_LEARN_LDS",)), (d4, "numpy", ("NO_LEARN_LDS", "NO_PM_NLEV_LDS")),
                              (d4, "numpy", ("NO_LEARN_LDS", "NO_NLEV_LDS"))]:
        created = dict(forms._plain(cfg), **forms.CREATED)
        for double in (False, True):
            _, (q, m, c) = check(shim, _of_cfg(created, double, rng, options, pm=1, nl_on=1), _budget(forms.ZIG_BYTES))
            assert (q, 2 if m else 1, bool(c)) == forms.pm_nlev_expected(cfg, double, rng, LIMIT, options), (cfg, rng, options, double)
            _, (q, m, c) = check(shim, _of_cfg(created, double, rng, options, nl_on=1), _budget(forms.ZIG_BYTES))
            assert (q, bool(c)) == forms.nlev_expected(cfg, double, rng, LIMIT, options) and not m, (cfg, rng, options, double)


def test_agrees_with_closed_loop_shape_cases_qlds_edges(shim):
    """a shared MDP without levels: Q in LDS or not"""
    for name, (cfg, double) in list(shp.QLDS_EDGE.items()) + [("cfg2_double", (shp.CFG2, True)), ("s255_a85", (shp.CASES["s255_a85"][0], False))]:
        asked, (q, m, c) = check(shim, _of_cfg(cfg, double), _budget(shp.static_lds(cfg)))
        assert bool(q) == shp.qlds_expected(cfg, double, LIMIT) and not m and not c, name
