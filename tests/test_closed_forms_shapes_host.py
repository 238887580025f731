"""The shape cases of the per-env-MDP, noise-level and schedule forms of the closed-loop kernels on the host (no GPU): every
condition tests/test_gpu_closed_forms_shapes.py asserts about its own coverage (tests/closed_forms_shape_cases.py) is met by the
32-env CPU closed loop -- the oracle env driven by the restatement, on the seeds the cases module names -- and every LDS
placement the GPU file asserts by kernel name is worked out by hand against the cases module's restatement of the rule."""
import numpy as np
import pytest

import closed_forms_shape_cases as cases
import closed_loop_shape_cases as shp
import learner_sweep_ref as ref
import per_env_mdp_cpu as pm

N = 32
KIB = 1024
LIMIT = 160 * KIB                    # a workgroup's LDS on gfx950
# (a scheduled run's kind of schedule goes by its stream too: those are kept apart; the CPU loop's own streams are Philox streams)
HOST_RUNS = sorted({(form, c, a, r if form == "sched" else "philox") for form, runs in cases.RUNS.items() for c, a, r in runs})


def restated_info(form, case, algo, traj, mdps, k):
    """learner_sweep_ref.run fed the CPU loop's own outputs launch by launch, as the GPU file feeds it the device's: the counts
    the GPU file asserts come from it.  Its actions are the loop's."""
    n = traj["obs"].shape[1]
    P = pm.PerEnvP(mdps) if len(mdps) > 1 else np.asarray(mdps[0].P)
    autoreset = cases.KW[case].get("autoreset", ref.SAME_STEP)
    S, A = np.asarray(mdps[0].P).shape
    Q = np.zeros((n, 2, S, A) if algo == "double_q" else (n, S, A), np.float32)
    pending, total, before = np.zeros(n, bool), {}, traj["obs0"]
    for launch in range(cases.LAUNCHES):
        sl = slice(launch * k, (launch + 1) * k)
        w = [ref.tick_words(cases.SEED, cases.OFF, launch * k, k + 1, n, st) for st in (ref.EXPLORE_STREAM, ref.ACTION_STREAM, ref.UPDATE_STREAM)]
        act, Q, pending, info = ref.run(algo, cases.ALPHA, cases.GAMMA, cases.EPS, Q, before, traj["obs"][sl], traj["reward"][sl], traj["terminated"][sl],
                                        traj["truncated"][sl], P, autoreset, *w, pending)
        assert np.array_equal(act, traj["actions"][sl]), (form, case, algo, launch)
        ref.merge_info(total, info)
        before = traj["obs"][sl][-1]
    return total, Q


def check(form, case, algo, rng="philox", n=N):
    """one CPU pass of a (form, case, algorithm) held to every condition the GPU file asserts; returns what it measured"""
    k = cases.K_OF.get((form, case), cases.K)
    Q, traj, extra = cases.cpu_loop(form, case, algo, n, rng=rng)
    mdps = cases.mdps_of(form, case, n)
    autoreset = cases.KW[case].get("autoreset", ref.SAME_STEP)
    P = np.stack([np.asarray(m.P) for m in mdps]) if len(mdps) > 1 else np.asarray(mdps[0].P)
    f = cases.flow(cases.states_of(traj), traj["actions"], traj["obs"], traj["reward"], traj["terminated"], traj["truncated"], autoreset, P)
    assert np.array_equal(f["reset_call"], traj["reset_call"])
    if form == "sched":
        agent = extra
        cases.sched_honest(case, algo, cases.sched_kind(case, algo, rng), agent.info, agent.ep, agent.sched.row)
        info = agent.info
        cases.learner_honest(case, algo, info, agent.Q)
        if case == "trunc_disabled":
            assert f["trunc"].any() and (f["term"] | f["trunc"])[-1].all()
    else:
        same_step_noise = form != "pm" and autoreset == ref.SAME_STEP and cases.KW[case].get("max_episode_steps")
        assert not same_step_noise                           # (the restatement cannot see what learn() saw there)
        info, Qr = restated_info(form, case, algo, traj, mdps, k)
        assert np.array_equal(Qr.view(np.int32), Q.view(np.int32))
        cases.learner_honest(case, algo, info, Q)
        if algo == "sarsa":
            assert info["carried"] > 0, info
    tn, rn = extra if form in ("nlev", "pm_nlev") else (None, None)
    cases.flow_honest(case, form, cases.CASES[case], f, mdps, autoreset, tn, rn)
    nz = pm.nonzero_envs(Q)
    return dict(nonzero=int(nz.sum()), terminated=int(f["term"].any(axis=0).sum()), ep=None if form != "sched" else (int(extra.ep.min()), int(np.median(extra.ep)), int(extra.ep.max())),
                info={k_: v for k_, v in info.items() if not isinstance(v, np.ndarray)})


@pytest.mark.parametrize("form,case,algo,rng", HOST_RUNS)
def test_cpu_closed_loop_meets_the_conditions(form, case, algo, rng):
    print(form, case, algo, rng, check(form, case, algo, rng))


@pytest.mark.parametrize("form,case", sorted(cases.FLOORS))
def test_per_env_floors_are_met_by_the_cpu_loop_of_the_gpu_set_up(form, case):
    """the floors the GPU file re-asserts, on the CPU loop of exactly its set-up (all N envs, Philox streams, q_learning)"""
    Q, traj, _ = cases.cpu_loop(form, case, "q_learning")
    print(form, case, cases.check_floors(case, form, Q, traj["terminated"]))


def test_every_form_x_mechanism_cell_of_the_case_table_has_a_run():
    want = {
        "pm": "d2_s12_a6_L2 d4_s24_a6 custom_5x3 custom_13x12 s4_L4 s2_L7 s4_L7 delay32_affine delay33 a1_s3 s255_a85 s10 s11 s12 trunc_same",
        "pm_nlev": "d2_s12_a6_L2 d4_s24_a6 custom_5x3 custom_13x12 s4_L4 delay32_affine s10 s11 s12 trunc_next",
        "nlev": "d2_s12_a6_L2 d4_s24_a6 custom_13x12_noise s4_L7 delay32_affine a1_s3 s255_a85",
        "sched": "d2_s12_a6_L2 d4_s24_a6 s4_L4 delay33 a1_s3 trunc_disabled",
    }
    for form, names in want.items():
        assert set(names.split()) == set(cases.FORMS[form]), form
        for c, pairs in cases.FORMS[form].items():
            assert {r for _, r in pairs} >= ({"numpy"} if c in ("s10", "s11", "s12") else {"numpy", "philox"}), (form, c)
    for form, cs in cases.CPU_LOOP_SHARED.items():
        assert set(cs) <= set(cases.FORMS[form])


def test_the_carve_numbers_of_the_case_table():
    lane = {c: cases.lane_bytes(cfg) for c, cfg in cases.CASES.items()}
    assert lane["d2_s12_a6_L2"] == 80 + 16 + 96 + 32 == 224          # P 72 -> 80, flags 12 -> 16, cdf 96, 144 reward bits = 18 B -> 32
    assert lane["d4_s24_a6"] == 144 + 32 + 192 + 16 == 384
    assert lane["custom_5x3"] == 16 + 16 + 48 + 128 == 208            # 15 doubles of R(s, a) = 120 B -> 128
    assert lane["custom_13x12"] == 160 + 16 + 112 + 1248 == 1536
    assert lane["s4_L4"] == 16 + 16 + 32 + 32 == 96                   # 256 reward bits = 32 B
    assert lane["s2_L7"] == 16 + 16 + 16 + 16 == 64                   # 128 reward bits = 16 B
    assert lane["s4_L7"] == 16 + 16 + 32 + 2048 == 2112               # 16 384 reward bits = 2 KiB per env
    assert lane["delay33"] == 64 + 16 + 64 + 64 == 208                # delay > 32: 8 doubles instead of 8 bits
    assert lane["delay32_affine"] == 64 + 16 + 64 + 16 == 160
    assert lane["a1_s3"] == 16 + 16 + 32 + 16 == 80
    assert lane["s10"] == 112 + 16 + 80 + 16 == 224 and lane["s11"] == 128 + 16 + 96 + 16 == 256 and lane["s12"] == 144 + 16 + 96 + 16 == 272
    # every per-env case's slot is what mdp.build_mdp's tables take
    for c in cases.FORMS["pm"]:
        m = cases.mdps_of("pm", c, 1)[0]
        unit = shp.shape_of(cases._plain(cases.CASES[c]))[4]
        rew = (len(m.reward_table()) + 7) // 8 if unit else 8 * len(m.reward_table())
        a16 = lambda x: (x + 15) // 16 * 16
        assert lane[c] == a16(m.S * m.A) + a16(m.S) + a16(8 * m.S) + a16(rew), c


def test_the_placements_at_the_bounds_worked_by_hand():
    pm_, nl, sh = cases.pm_expected, cases.pm_nlev_expected, cases.nlev_expected
    s10, s11, s12, d4 = (cases.CASES[c] for c in ("s10", "s11", "s12", "d4_s24_a6"))
    # s11: 256 lanes x 256 B are exactly 64 KiB of slots -- allowed -- and Q is 121 KiB: 185 KiB together, 121 KiB alone
    assert 256 * 256 == 64 * KIB and 256 * 121 * 4 == 121 * KIB and 24 + (64 + 121) * KIB > LIMIT >= 24 + 121 * KIB
    assert pm_(s11, False, LIMIT) == (1, 1)
    assert pm_(s11, False, LIMIT, ("NO_LEARN_LDS",)) == (0, 2)       # the slots alone: at their bound, not over it
    assert pm_(s11, False, LIMIT, ("NO_LEARN_LDS", "NO_PM_LDS")) == (0, 1)
    # s12: 272 B per lane are 68 KiB: never a candidate, whatever the options
    assert 256 * 272 == 68 * KIB > 64 * KIB
    for dbl in (False, True):
        for opts in ((), ("NO_LEARN_LDS",), ("NO_PM_LDS",), ("NO_LEARN_LDS", "NO_PM_LDS")):
            assert pm_(s12, dbl, LIMIT, opts)[1] == 1
            for rng in ("numpy", "philox"):
                assert nl(s12, dbl, rng, LIMIT, opts)[1] == 1
    # s10: slots 56 KiB + Q 100 KiB = 156 KiB fit with the 24 B of a noise-free kernel; a noise kernel's 6 KiB of ziggurat
    # tables and the shared cdf of 800 B tip them over, Q stays alone
    assert 256 * 224 == 56 * KIB and 256 * 100 * 4 == 100 * KIB
    assert pm_(s10, False, LIMIT) == (1, 2)
    noisy = dict(s10, **cases.CREATED)
    assert 6144 + 800 + 156 * KIB == 166688 > LIMIT == 163840 >= 6144 + 800 + 100 * KIB
    assert pm_(noisy, False, LIMIT) == (1, 1)
    assert pm_(noisy, False, LIMIT + 2848) == (1, 2) and pm_(noisy, False, LIMIT + 2847) == (1, 1)     # the sum decides, to the byte
    assert pm_(dict(s10, reward_noise=0.5), False, LIMIT) == (1, 1)      # (no cdf: 6144 + 156 KiB is still 2.1 KiB too much)
    # ... under levels the shared cdf is not staged: Q + slots + ziggurat = 162 KiB, over; Q + the 4000 B of five levels fit
    assert nl(s10, False, "numpy", LIMIT) == (1, 1, True) and nl(s10, False, "philox", LIMIT) == (1, 1, False)
    assert nl(s10, False, "numpy", LIMIT, ("NO_LEARN_LDS",)) == (0, 2, True)
    # d4_s24_a6 under five levels, numpy streams: cdfs 5 x 24 x 24 x 8 = 22.5 KiB, Q 144 KiB: 172.5 KiB with the ziggurat tables
    assert cases.cdf_bytes(d4, 5) == 23040 and cases.cdf_bytes(d4, 7) == 32256 <= 32 * KIB and 256 * 144 * 4 == 144 * KIB
    assert 6144 + 144 * KIB + 23040 > LIMIT >= 6144 + 144 * KIB
    assert nl(d4, False, "numpy", LIMIT) == (1, 1, False)
    assert nl(d4, False, "numpy", LIMIT, ("NO_LEARN_LDS",)) == (0, 1, True)
    assert nl(d4, False, "numpy", LIMIT, ("NO_LEARN_LDS", "NO_PM_NLEV_LDS")) == (0, 1, False)
    assert nl(d4, True, "numpy", LIMIT) == (0, 1, True)              # (two tables: 288 KiB, no candidate)
    # the shared-MDP handle of the same shape: its carve (384 B + its own cdf of 4.5 KiB) beside them
    assert sh(d4, False, "numpy", LIMIT) == (1, False) and sh(d4, False, "numpy", LIMIT, ("NO_LEARN_LDS",)) == (0, True)
    assert sh(d4, False, "numpy", LIMIT, ("NO_LEARN_LDS", "NO_NLEV_LDS")) == (0, False)
    # Q twice beside the slots
    for c in cases.DOUBLE_PM2:
        assert pm_(cases.CASES[c], True, LIMIT) == (1, 2), c
    # the restatement agrees with noise_seed_cases' on the shapes that one covers
    import noise_seed_cases as nsc
    for cfg in (nsc.TABULAR, nsc.CFG2, nsc.S20, nsc.S29):
        for algo in cases.ALGOS:
            for rng in ("numpy", "philox"):
                for opts in ((), ("NO_LEARN_LDS",), ("NO_PM_LDS", "NO_PM_NLEV_LDS")):
                    assert nl(cfg, algo == "double_q", rng, LIMIT, opts) == nsc.placement(cfg, algo, rng, *opts)[:3]


def test_levels_sit_as_the_conditions_ask():
    for n in (cases.N, 257, 65, 63):
        cases.levels_honest(*cases.level_arrays(n))


def test_no_live_state_of_the_truncation_cases_mdps_leads_to_itself():
    """why trunc_next is not held to sarsa's dropped carry (closed_forms_shape_cases.learner_honest)"""
    for m in cases.mdps_of("pm_nlev", "trunc_next", N):
        P = np.asarray(m.P)
        live = np.setdiff1d(np.arange(P.shape[0]), m.terminal_states)      # (a terminal state is never acted from)
        assert (P[live] != live[:, None]).all()


@pytest.mark.parametrize("form,case,double", sorted({(f, c, a == "double_q") for f, c, a, _ in cases.EVAL_RUNS}))
def test_cpu_evaluation_meets_the_evaluation_conditions(form, case, double):
    info, ended, reward, reset_call, rn = cases.cpu_eval_loop(form, case, double, N)
    print(form, case, double, info, ended)
    cases.eval_flow_honest(form, case, info, double, reward, reset_call, rn)
    assert ended > 0
