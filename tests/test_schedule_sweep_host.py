"""Schedules on the noise-level and per-env-MDP learners on the host (no GPU): every condition
tests/test_gpu_schedule_sweep.py asserts about its own coverage (tests/schedule_sweep_cases.py) is met by the 32-env CPU closed
loop -- one oracle env per env, on its own MDP at its own level, driven by the scheduled restatement -- and
tests/learner_schedule_ref.py's run(), fed that loop's outputs launch by launch with P per env as the GPU file feeds it the
device's, reproduces the loop: the restatement alone meets the conditions before any GPU run.  The kernel names the GPU file
expects are worked out for the device's 160 KiB, and the new entry point is checked as far as it runs without a device."""
import ctypes as C

import numpy as np
import pytest

import learner_schedule_ref as sref
import learner_sweep_ref as ref
import schedule_sweep_cases as cases

N = 32
LIMIT = 160 * 1024                  # a workgroup's LDS on gfx950
# (a run's kind of schedule goes by its stream too: both are kept; the CPU loop's own streams are Philox streams)
HOST_RUNS = cases.RUNS


def _restated(form, case, algo, kind, traj, n, k=cases.K):
    """learner_schedule_ref.run fed the CPU loop's own outputs launch by launch: its actions are the loop's, and the agent it
    leaves is what the GPU file compares get_q() and learner_episodes() with"""
    agent = cases.new_agent(form, case, algo, kind, n)
    P = cases.P_of(form, case, n)
    before = traj["obs0"]
    for launch in range(cases.LAUNCHES):
        sl = slice(launch * k, (launch + 1) * k)
        w = [ref.tick_words(cases.SEED, cases.OFF, launch * k, k + 1, n, st) for st in (ref.EXPLORE_STREAM, ref.ACTION_STREAM, ref.UPDATE_STREAM)]
        act = sref.run(agent, before, traj["obs"][sl], traj["reward"][sl], traj["terminated"][sl], traj["truncated"][sl], P, *w)
        assert np.array_equal(act, traj["actions"][sl]), (form, case, algo, launch, np.argwhere(act != traj["actions"][sl])[:5])
        before = traj["obs"][sl][-1]
    return agent


def check(form, case, algo, rng, n=N):
    kind = cases.kind_of(form, case, algo, rng)
    loop, traj = cases.closed_loop(form, case, algo, kind, n)
    agent = _restated(form, case, algo, kind, traj, n)
    assert np.array_equal(agent.Q.view(np.int32), loop.Q.view(np.int32)) and np.array_equal(agent.ep, loop.ep)
    tn, _ = cases.levels_of(form, n)
    P = cases.P_of(form, case, n)
    cases.honest(form, case, algo, kind, agent.info, agent.ep, agent.sched.row, traj["state"], traj["actions"], traj["next_state"],
                 ~traj["reset_call"], tn, P.P if form in cases.PER_ENV_FORMS else P)
    m = cases.sched_m(form, case)
    return dict(kind=kind, M=m, ep=(int(agent.ep.min()), int(np.median(agent.ep)), int(agent.ep.max())), past=int((agent.ep >= m).sum()),
                short=int((agent.ep < m - 1).sum()), E_changes=agent.info["E_changes"], alpha_changes=agent.info["alpha_changes"],
                carried_old_E=agent.info["carried_old_E"], carried_old_E_differs=agent.info["carried_old_E_differs"])


@pytest.mark.parametrize("form,case,algo,rng", HOST_RUNS)
def test_cpu_closed_loop_and_the_restatement_meet_the_conditions(form, case, algo, rng):
    print(form, case, algo, rng, check(form, case, algo, rng))


@pytest.mark.parametrize("form", cases.FORMS)
def test_the_conditions_at_the_gpu_files_320_envs(form):
    """autoreset disabled: EVERY env clamps (a statement about all 320); elsewhere the conditions are existence statements that
    more envs only make easier -- one run per form at the GPU file's size shows the set-up itself (levels, rows, seeds)"""
    case = cases.FORM_CASES[form][-1]
    cases.triples_honest(form, case, cases.N)
    cases.triples_honest(form, case, 223, 97)
    print(form, case, check(form, case, "sarsa", "philox", cases.N))


def test_every_form_and_case_runs_all_three_kinds_and_both_streams():
    for form in cases.FORMS:
        for case in cases.FORM_CASES[form]:
            kinds = {cases.kind_of(form, case, a, r) for a in cases.ALGOS for r in cases.RNGS}
            assert kinds == set(cases.KINDS), (form, case, kinds)
    tn, rn = cases.level_arrays(cases.N)
    row = cases.rows(cases.N)
    assert len({(p, s, r) for p, s, r in zip(tn, rn, row)}) == 28           # every (pair, row) combination
    for lo in range(0, cases.N, 64):
        assert len({(p, s, r) for p, s, r in zip(tn[lo:lo + 64], rn[lo:lo + 64], row[lo:lo + 64])}) == 28


# ---- the kernel names
def test_expected_kernel_names_for_160_kib():
    want = {
        ("nlev", "s8_noise", "q_learning", "numpy"): "k_discrete_learn_rollout<PHILOX=0,NOISE=1,UNIT=1,QLDS=1,PE=1,NLEV=1,SCHED=1>",
        ("nlev", "d4_s24_a6", "double_q", "philox"): "k_discrete_learn_rollout<PHILOX=1,NOISE=1,UNIT=1,QLDS=0,PE=1,DOUBLE=1,NLEV=1,SCHED=1>",
        ("pm", "s8_noise", "sarsa", "numpy"): "k_discrete_learn_rollout<PHILOX=0,NOISE=1,UNIT=1,QLDS=1,PE=1,PM=2,SCHED=1>",
        ("pm", "d2_s12_a6_L2", "q_learning", "philox"): "k_discrete_learn_rollout<PHILOX=1,NOISE=0,UNIT=1,QLDS=1,PE=1,PM=2,SCHED=1>",
        ("pm", "d4_s24_a6", "double_q", "numpy"): "k_discrete_learn_rollout<PHILOX=0,NOISE=0,UNIT=1,QLDS=0,PE=1,DOUBLE=1,PM=1,SCHED=1>",
        ("pm", "custom_5x3", "q_learning", "numpy"): "k_discrete_learn_rollout<PHILOX=0,NOISE=0,UNIT=0,QLDS=1,PE=1,PM=2,SCHED=1>",
        ("pm_nlev", "d2_s12_a6_L2", "sarsa", "numpy"): "k_discrete_learn_rollout<PHILOX=0,NOISE=1,UNIT=1,QLDS=1,PE=1,NLEV=1,PM=2,SCHED=1>",
        ("pm_nlev", "d4_s24_a6", "q_learning", "philox"): "k_discrete_learn_rollout<PHILOX=1,NOISE=1,UNIT=1,QLDS=1,PE=1,NLEV=1,PM=1,SCHED=1>",
    }
    for (form, case, algo, rng), name in want.items():
        qlds, pmv = cases.expected_placement(form, case, algo, rng, LIMIT)
        got = cases.kernel_name(form, cases.handle_cfg(form, case), algo, rng, qlds, pmv)
        assert got == name, (form, case, algo, rng, got)
    # the summary kernel, and the same handle without its schedule
    cfg = cases.handle_cfg("pm_nlev", "d2_s12_a6_L2")
    assert cases.kernel_name("pm_nlev", cfg, "double_q", "numpy", 1, 2, summary=True) == \
        "k_discrete_learn_summary<PHILOX=0,NOISE=1,UNIT=1,QLDS=1,PE=1,DOUBLE=1,NLEV=1,PM=2,SCHED=1>"
    assert cases.kernel_name("pm_nlev", cfg, "double_q", "numpy", 1, 2, sched=False) == \
        "k_discrete_learn_rollout<PHILOX=0,NOISE=1,UNIT=1,QLDS=1,PE=1,DOUBLE=1,NLEV=1,PM=2>"
    # a schedule has no LDS placement: every case is placed as its unscheduled handle is, under every option
    for form, case, algo, rng in cases.RUNS:
        assert cases.expected_placement(form, case, algo, rng, LIMIT) == cases.expected_placement(form, case, algo, rng, LIMIT, ())


# ---- the C ABI as far as it runs without a device
def test_the_entry_point_is_exported_declared_and_refuses_a_null_handle():
    from mdp_playground_amd import _capi
    assert "mdpp_learner_schedule_sweep" in _capi.EXPORTS
    lib = _capi.load()
    assert lib.mdpp_learner_schedule_sweep.argtypes == [C.c_void_p, C.c_int32] or len(lib.mdpp_learner_schedule_sweep.argtypes) == 2
    for on in (0, 1):
        assert lib.mdpp_learner_schedule_sweep(None, on) == -1                  # MDPP_EINVAL: no handle
    assert lib.mdpp_abi_version() == _capi.MDPP_ABI_VERSION                   # (additive: the version stays)


def test_the_python_keyword_defaults_to_off():
    import inspect
    from mdp_playground_amd import RLToyVectorEnv
    sig = inspect.signature(RLToyVectorEnv.set_learner_schedule)
    assert sig.parameters["sweep"].default is False and list(sig.parameters)[1:] == ["epsilon", "alpha", "row", "sweep"]
    assert "sweep=True" in RLToyVectorEnv.set_learner_schedule.__doc__
