"""The per-env-MDP, noise-level and schedule forms of the closed-loop kernels beyond square MDPs (PM=1 / PM=2, NLEV=1, NLEV=1 with
PM, SCHED=1 of k_discrete_learn_rollout / k_discrete_eval_rollout and their summary kernels): S != A, use_custom_mdp reward
matrices, sequence_length 4 and 7, the delay line at 32 and 33, the reward plumbing, A = 1, state byte 0xFE, truncation, and the
LDS placements at their bounds.  The cases, the forms each runs under and what a pass must have exercised are in
tests/closed_forms_shape_cases.py; tests/test_closed_forms_shapes_host.py shows on the CPU that those conditions can be met and
works the placements out by hand.

The yardsticks are those of the files extended, whose helpers this file uses, all bit for bit:
  open-loop twin   a second handle of the same config, seeds and streams fed the returned actions through rollout(): outputs
                   (reward by bits), state record, both streams, tick;
  restatement      tests/learner_sweep_ref.py / tests/learner_schedule_ref.py fed the launch's own outputs: actions, get_q(),
                   learner_episodes(); and the kernel's name with its UNIT / QLDS / DOUBLE / NLEV / PM / SCHED values;
  CPU loop         (Philox streams) the whole launch predicted from the oracle env with no GPU output in the loop;
  uniform twins    (levels) env i of a mixed handle equals env i of a handle created uniformly at its pair of levels.
N = 320, K = 37 (s4_L4 and s4_L7 per env: 74), two launches, env_id_offset = 1000."""
import numpy as np
import pytest
import torch

import closed_forms_shape_cases as cases
import closed_loop_shape_cases as shp
import eval_summary_ref as eref
import graph_replay_util as gr
import learner_schedule_cases as lsc
import learner_schedule_ref as sref
import learner_sweep_ref as ref
import per_env_mdp_cpu as pm
import test_gpu_learn_sweep as shared_mdp
import test_gpu_noise_seeds as levels
from test_gpu_closed_loop_shapes import _lds_limit
from test_gpu_learn_rollout import _mk as _mk_shared
from test_gpu_per_env_mdp import (Restated, _assert_same_handles, _assert_same_outputs, _assert_summary, _bits, _check_launch, _np, _obs_now,
                                  _tick)

pytestmark = pytest.mark.gpu

N, K, OFF, SEED = cases.N, cases.K, cases.OFF, cases.SEED
ALPHA, GAMMA, EPS = cases.ALPHA, cases.GAMMA, cases.EPS
ALL = np.arange(N)
_same_at, _same_handles_at, _run_twin_rule, _close = levels._same_at, levels._same_handles_at, levels._run_twin_rule, levels._close


def _autoreset(case):
    return cases.KW[case].get("autoreset", ref.SAME_STEP)


# ---- handles
def _mk(cfg, rng, seeds, off=OFF, options=(), **kw):
    """a handle with one MDP per env (mdps=[...] where the envs differ by more than the seed)"""
    from mdp_playground_amd import RLToyVectorEnv
    config, more = cases.handle_cfg(cfg, list(seeds))
    extra = dict(rng="philox", philox_seed=cases.PHILOX_SEED) if rng == "philox" else {}
    env = RLToyVectorEnv(seeds=list(seeds), env_id_offset=off, **extra, **more, **kw, **config)
    if options:
        env.set_kernel_options(*options)
    return env


def _learner(env, algo, q=None, per_env=True):
    more = dict(per_env_mdp=True) if per_env else {}
    env.set_learner(algo, alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=SEED, q=None if q is None else torch.as_tensor(q, device=env.device), **more)


def _pm_handle(case, rng, algo, n=None, lo=0, options=(), q=None, learner=True):
    seeds = cases.seeds_of(case, n, lo)
    env = _mk(cases.per_env_cfg(case), rng, seeds, OFF + lo, options, **cases.KW[case])
    if learner:
        _learner(env, algo, q)
    return env


def _mixed(case, rng, algo, per_env, n=None, lo=0, options=(), q=None):
    """a handle of envs lo ... of the seven-pair level cycle with its learner and its levels; per_env: on one MDP per env"""
    n = N if n is None else n
    tn, rn = cases.level_arrays(n, lo)
    if per_env:
        env = _mk(dict(cases.per_env_cfg(case), **cases.CREATED), rng, cases.seeds_of(case, n, lo), OFF + lo, options, **cases.KW[case])
    else:
        env = _mk_shared(dict(cases.shared_cfg(case), **cases.CREATED), rng, n=n, env_id_offset=OFF + lo, **cases.KW[case])
        if options:
            env.set_kernel_options(*options)
    _learner(env, algo, q, per_env)
    env.set_noise_levels(transition_noise=tn, reward_noise=rn, **(dict(per_env_mdp=True) if per_env else {}))
    return env, tn, rn


def _twins(case, rng, algo, per_env, tn, rn, n=None, lo=0, q=None):
    """(p, sigma) -> (the handle created uniformly at that pair with the same seeds and learner, the mixed handle's envs at it)"""
    n = N if n is None else n
    out = {}
    for p, s in cases.pairs_present(tn, rn):
        noise = dict(transition_noise=float(p), reward_noise=float(s))
        if per_env:
            env = _mk(dict(cases.per_env_cfg(case), **noise), rng, cases.seeds_of(case, n, lo), OFF + lo, **cases.KW[case])
        else:
            env = _mk_shared(dict(cases.shared_cfg(case), **noise), rng, n=n, env_id_offset=OFF + lo, **cases.KW[case])
        _learner(env, algo, q, per_env)
        assert "NLEV" not in env.learn_kernel_name(K)
        out[(p, s)] = (env, np.flatnonzero((tn == p) & (rn == s)))
    return out


def _names(env, form, cfg, algo, rng, qlds, pmv=None):
    want = cases.kernel_name("learn", form, cfg, algo, rng, qlds, pmv)
    assert env.learn_kernel_name(K) == want, (env.learn_kernel_name(K), want)
    if form != "sched":                                  # (evaluation ignores a schedule)
        want = cases.kernel_name("eval", form, cfg, algo, rng, qlds, pmv)
        assert env.eval_kernel_name(K) == want, (env.eval_kernel_name(K), want)


def _stack(outs):
    return [np.concatenate([_np(o[j]) for o in outs]) for j in range(5)]


def _flow(case, befores, outs, mdps):
    obs, rew, term, trunc, act = _stack(outs)
    state = np.concatenate([np.concatenate([b[None], _np(o[0])[:-1]]) for b, o in zip(befores, outs)]).astype(np.int64)
    P = np.stack([np.asarray(m.P) for m in mdps]) if len(mdps) > 1 else np.asarray(mdps[0].P)
    return cases.flow(state, act.astype(np.int64), obs.astype(np.int64), rew, term, trunc, _autoreset(case), P)


def _assert_cpu_loop(form, case, algo, env, outs, what):
    """Philox streams: the whole of both launches is what the CPU loop predicts"""
    Q, traj, extra = cases.cpu_loop(form, case, algo, env.num_envs)
    obs, rew, term, trunc, act = _stack(outs)
    for name, g, w in (("actions", act, traj["actions"]), ("obs", obs, traj["obs"]), ("terminated", term.astype(bool), traj["terminated"]),
                       ("truncated", trunc.astype(bool), traj["truncated"]), ("reward", _bits(rew), _bits(traj["reward"]))):
        assert np.array_equal(g, w), (what, "CPU loop", name, np.argwhere(g != w)[:5])
    assert np.array_equal(_bits(_np(env.get_q())), _bits(Q)), (what, "CPU loop", "Q")
    return extra


def _floors(form, case, rng, env, term, what):
    if rng == "philox":                                  # (measured on the Philox streams)
        return cases.check_floors(case, form, _np(env.get_q()), term.astype(bool), what)
    nz = pm.nonzero_envs(_np(env.get_q()))
    assert nz[:256].any() and nz[256:].any(), what
    return int(nz.sum())


# ---- one MDP per env
@pytest.mark.parametrize("case,algo,rng", cases.RUNS["pm"])
def test_per_env_mdp_twin_restatement_and_cpu_loop(case, algo, rng):
    cfg, k = cases.per_env_cfg(case), cases.K_OF.get(("pm", case), K)
    a, b = _pm_handle(case, rng, algo), _pm_handle(case, rng, algo, learner=False)
    double = algo == "double_q"
    qlds, pmv = cases.pm_expected(cfg, double, _lds_limit())
    _names(a, "pm", cfg, algo, rng, qlds, pmv)
    if case in cases.DOUBLE_PM2 and double:
        assert (qlds, pmv) == (1, 2) and ",DOUBLE=1,PM=2>" in a.learn_kernel_name(K)
    seeds = cases.seeds_of(case)
    r = Restated(cfg, algo, seeds=seeds, autoreset=_autoreset(case))
    what = ("pm", case, algo, rng)
    outs, befores = [], []
    for launch in range(cases.LAUNCHES):
        assert _tick(a) == launch * k
        befores.append(_obs_now(a))
        out = _check_launch(a, r, k, what + (launch,))
        _assert_same_outputs(out[:4], b.rollout(out[4]), what + (launch,))
        outs.append(out)
    _assert_same_handles(a, b, rng)
    if rng == "philox":
        _assert_cpu_loop("pm", case, algo, a, outs, what)
    mdps = cases.mdps_of("pm", case)
    f = _flow(case, befores, outs, mdps)
    cases.learner_honest(case, algo, r.info, r.Q)
    if algo == "sarsa":
        assert r.info["carried"] > 0, r.info
    cases.flow_honest(case, "pm", cases.CASES[case], f, mdps, _autoreset(case))
    print(what, a.learn_kernel_name(k), _floors("pm", case, rng, a, f["term"], what), {k_: v for k_, v in r.info.items() if not isinstance(v, np.ndarray)})
    a.close(); b.close()


# ---- per-env noise levels, on one MDP per env and on a shared MDP
def _levels_pass(form, case, algo, rng):
    per_env = form == "pm_nlev"
    cfg = cases.per_env_cfg(case) if per_env else cases.shared_cfg(case)
    a, tn, rn = _mixed(case, rng, algo, per_env)
    double = algo == "double_q"
    if per_env:
        qlds, pmv, _ = cases.pm_nlev_expected(cfg, double, rng, _lds_limit())
    else:
        (qlds, _), pmv = cases.nlev_expected(cfg, double, rng, _lds_limit()), None
    _names(a, form, cfg, algo, rng, qlds, pmv)
    got_tn, got_rn = a.noise_levels()
    assert np.array_equal(got_tn, tn) and np.array_equal(got_rn, rn)
    twins = _twins(case, rng, algo, per_env, tn, rn)
    assert len(twins) == 7
    r = (levels.Restated(cfg, algo, seeds=cases.seeds_of(case), autoreset=_autoreset(case)) if per_env
         else shared_mdp.Restated(a, algo, off=OFF, autoreset=_autoreset(case)))
    what = (form, case, algo, rng)
    from mdp_playground_amd import _capi as capi
    space_before = a.get_rng_streams(capi.STREAM_SPACE).copy() if rng == "numpy" else None
    step = levels._restated_step(a, r, K, what)
    outs = _run_twin_rule(a, twins, rng, what, step=step)
    if rng == "philox" and (per_env or case in cases.CPU_LOOP_SHARED["nlev"]):
        _assert_cpu_loop(form, case, algo, a, outs, what)
    mdps = cases.mdps_of(form, case)
    f = _flow(case, step.before, outs, mdps)
    cases.learner_honest(case, algo, r.info, r.Q)
    cases.flow_honest(case, form, cases.CASES[case], f, mdps, _autoreset(case), tn, rn)
    if rng == "numpy":
        # an env of level 0, whose space stream did not move, beside one whose stream did
        moved = (a.get_rng_streams(capi.STREAM_SPACE) != space_before).reshape(N, -1).any(axis=1)
        assert not moved[tn == 0].any()
        if case != "a1_s3":
            assert ((tn[1:] == 0) & moved[:-1]).any() or ((tn[:-1] == 0) & moved[1:]).any()
    if per_env:
        print(what, a.learn_kernel_name(K), _floors(form, case, rng, a, f["term"], what))
    _close(a, twins)


@pytest.mark.parametrize("case,algo,rng", cases.RUNS["pm_nlev"])
def test_levels_on_one_mdp_per_env_uniform_twins_restatement_and_cpu_loop(case, algo, rng):
    _levels_pass("pm_nlev", case, algo, rng)


@pytest.mark.parametrize("case,algo,rng", cases.RUNS["nlev"])
def test_levels_on_a_shared_mdp_uniform_twins_restatement_and_cpu_loop(case, algo, rng):
    assert shp.learner_refused(dict(cases.shared_cfg(case), **cases.CREATED)) is None
    _levels_pass("nlev", case, algo, rng)


# ---- schedules
def _scheduled(case, rng, algo, kind, options=()):
    e = _mk_shared(cases.shared_cfg(case), rng, n=N, env_id_offset=OFF, **cases.KW[case])
    if options:
        e.set_kernel_options(*options)
    _learner(e, algo, per_env=False)
    eps, al = lsc.tables(kind, cases.sched_m(case, kind))
    e.set_learner_schedule(epsilon=eps, alpha=al, row=lsc.rows(N))
    return e


@pytest.mark.parametrize("case,algo,rng", cases.RUNS["sched"])
def test_scheduled_launch_twin_restatement_and_cpu_loop(case, algo, rng):
    cfg, kw = cases.shared_cfg(case), cases.KW[case]
    kind = cases.sched_kind(case, algo, rng)
    a, b = _scheduled(case, rng, algo, kind), _mk_shared(cfg, rng, n=N, env_id_offset=OFF, **kw)
    double = algo == "double_q"
    qlds = shp.qlds_expected(cfg, double, _lds_limit())
    if case == "d4_s24_a6" and double:
        assert not qlds                                  # the global-form Q of a rectangular table: 288 KiB
    _names(a, "sched", cfg, algo, rng, qlds)
    m = a.mdps[0]
    shape = (N, 2, m.S, m.A) if double else (N, m.S, m.A)
    sched = lsc.schedule(kind, cases.sched_m(case, kind), N)
    agent = sref.Agent(algo, N, ALPHA, GAMMA, EPS, sched, np.zeros(shape, np.float32), _autoreset(case))
    what = ("sched", case, algo, rng, kind)
    outs, befores = [], []
    for launch in range(cases.LAUNCHES):
        before, tick0 = _obs_now(a), _tick(a)
        assert tick0 == launch * K
        out = a.rollout_learn(K)
        w = [ref.tick_words(SEED, OFF, tick0, K + 1, N, st) for st in (ref.EXPLORE_STREAM, ref.ACTION_STREAM, ref.UPDATE_STREAM)]
        want = sref.run(agent, before, *(_np(x) for x in out[:4]), np.asarray(m.P), *w)
        got = _np(out[4])
        assert np.array_equal(got, want), (what, launch, "actions", np.argwhere(got != want)[:5])
        assert np.array_equal(_bits(_np(a.get_q())), _bits(agent.Q)), (what, launch, "Q")
        assert np.array_equal(_np(a.learner_episodes()), agent.ep), (what, launch, "episodes")
        _assert_same_outputs(out[:4], b.rollout(out[4]), what + (launch,))
        outs.append(out); befores.append(before)
    _assert_same_handles(a, b, rng)
    if rng == "philox" and case in cases.CPU_LOOP_SHARED["sched"]:
        cpu_agent = _assert_cpu_loop("sched", case, algo, a, outs, what)        # (rng: philox, the kind of this run)
        assert np.array_equal(cpu_agent.ep, agent.ep)
    cases.sched_honest(case, algo, kind, agent.info, agent.ep, sched.row)
    cases.learner_honest(case, algo, agent.info, agent.Q)
    mdps = cases.mdps_of("sched", case)
    cases.flow_honest(case, "sched", cases.CASES[case], _flow(case, befores, outs, mdps), mdps, _autoreset(case))
    print(what, a.learn_kernel_name(K), "ep", agent.ep.min(), agent.ep.max())
    a.close(); b.close()


# ---- the placements at their bounds: asserted by name from the device's own limit, and every placement forced through the
# options computes what the default placement computes, on every array
def _equal_passes(handles, rng, what, eval_too=True):
    for launch in range(2):
        want = handles[0].rollout_learn(K)
        for j, e in enumerate(handles[1:]):
            _same_at(e.rollout_learn(K), want, ALL, what + (j + 1, launch))
            _same_handles_at(e, handles[0], ALL, rng, what + (j + 1, launch))
    if eval_too:
        want = handles[0].rollout_eval(K)
        for j, e in enumerate(handles[1:]):
            _same_at(e.rollout_eval(K), want, ALL, what + (j + 1, "eval"))
    for e in handles:
        e.close()


PM_OPTIONS = [(), ("NO_PM_LDS",), ("NO_LEARN_LDS",), ("NO_PM_LDS", "NO_LEARN_LDS")]


@pytest.mark.parametrize("case", ["s10", "s11", "s12"])
def test_placement_of_q_and_the_slots_at_the_bounds(case):
    limit, cfg = _lds_limit(), cases.per_env_cfg(case)
    handles = []
    for options in PM_OPTIONS:
        e = _pm_handle(case, "numpy", "q_learning", options=options)
        _names(e, "pm", cfg, "q_learning", "numpy", *cases.pm_expected(cfg, False, limit, options))
        handles.append(e)
    d, no_q = handles[0].learn_kernel_name(K), handles[2].learn_kernel_name(K)
    if limit == 160 * 1024:
        if case == "s10":
            assert "QLDS=1" in d and d.endswith("PM=2>")                 # 56 + 100 KiB fit
        if case == "s11":
            assert "QLDS=1" in d and d.endswith("PM=1>")                 # slots of exactly 64 KiB and Q of 121 KiB do not fit together
            assert "QLDS=0" in no_q and no_q.endswith("PM=2>")           # ... the slots alone do: 64 KiB is within the bound
    if case == "s12":
        assert all(e.learn_kernel_name(K).endswith("PM=1>") and e.eval_kernel_name(K).endswith("PM=1>") for e in handles)    # 68 KiB: never
    _equal_passes(handles, "numpy", ("pm", case))


def test_placement_of_s10_with_both_noise_keys():
    """static LDS + shared cdf + slots + Q against the limit: the 6 KiB of ziggurat tables decide"""
    limit = _lds_limit()
    cfg = dict(cases.per_env_cfg("s10"), **cases.CREATED)
    want = cases.pm_expected(cfg, False, limit)
    assert want == ((1, 2) if 6144 + 800 + 156 * 1024 <= limit else (1, 1))
    handles = []
    for options in PM_OPTIONS:
        e = _mk(cfg, "numpy", cases.seeds_of("s10"), options=options)
        _learner(e, "q_learning")
        _names(e, "pm", cfg, "q_learning", "numpy", *cases.pm_expected(cfg, False, limit, options))
        handles.append(e)
    _equal_passes(handles, "numpy", ("pm", "s10 with noise keys"))


NLEV_OPTIONS = [(), ("NO_PM_NLEV_LDS",), ("NO_PM_LDS",), ("NO_LEARN_LDS",), ("NO_LEARN_LDS", "NO_PM_NLEV_LDS"), ("NO_LEARN_LDS", "NO_PM_LDS", "NO_PM_NLEV_LDS")]


@pytest.mark.parametrize("case", ["d4_s24_a6", "s10", "s11", "s12"])
def test_placement_of_q_the_slots_and_the_level_cdfs_at_the_bounds(case):
    limit, cfg = _lds_limit(), cases.per_env_cfg(case)
    handles, placed = [], []
    for options in NLEV_OPTIONS:
        e, _, _ = _mixed(case, "numpy", "q_learning", True, options=options)
        qlds, pmv, _ = cases.pm_nlev_expected(cfg, False, "numpy", limit, options)
        _names(e, "pm_nlev", cfg, "q_learning", "numpy", qlds, pmv)
        handles.append(e); placed.append((qlds, pmv))      # (whether the cdfs are staged shows in no name: the equal outputs cover it)
    if limit == 160 * 1024:
        if case == "d4_s24_a6":
            assert placed[0] == (1, 1) and placed[3] == (0, 1)                  # Q alone by default (the rule then stages the cdfs without Q)
        if case == "s11":
            assert placed[0] == (1, 1) and placed[3] == (0, 2)
    if case == "s12":
        assert all(p[1] == 1 for p in placed)
    _equal_passes(handles, "numpy", ("pm_nlev", case))


def test_placement_of_the_level_cdfs_against_q_on_a_shared_mdp():
    """d4_s24_a6 under five levels, numpy streams: Q alone by default, the cdfs staged without it"""
    limit, cfg = _lds_limit(), cases.shared_cfg("d4_s24_a6")
    handles, placed = [], []
    for options in [(), ("NO_NLEV_LDS",), ("NO_LEARN_LDS",), ("NO_LEARN_LDS", "NO_NLEV_LDS")]:
        e, _, _ = _mixed("d4_s24_a6", "numpy", "q_learning", False, options=options)
        qlds, _ = cases.nlev_expected(cfg, False, "numpy", limit, options)
        _names(e, "nlev", cfg, "q_learning", "numpy", qlds)
        handles.append(e); placed.append(qlds)             # (whether the cdfs are staged shows in no name: the equal outputs cover it)
    if limit == 160 * 1024:
        assert placed == [1, 1, 0, 0]
    _equal_passes(handles, "numpy", ("nlev", "d4_s24_a6"))


# ---- evaluation and summaries
def _summary_follows(s, summ, full_out, st, pending, autoreset, what):
    rc, pending = eref.reset_calls(_np(full_out[2]).astype(bool), _np(full_out[3]).astype(bool), autoreset, pending)
    st = eref.summary(_np(full_out[1]), _np(full_out[2]).astype(bool), _np(full_out[3]).astype(bool), rc, st)
    _assert_summary(summ, st, what)
    return st, pending


@pytest.mark.parametrize("case,algo,rng", [r[1:] for r in cases.EVAL_RUNS if r[0] == "pm"])
def test_evaluation_and_summaries_on_one_mdp_per_env(case, algo, rng):
    cfg, autoreset, double = cases.per_env_cfg(case), _autoreset(case), algo == "double_q"
    q0 = cases.eval_tables(cfg, N, double)
    a, s, b = _pm_handle(case, rng, algo, q=q0), _pm_handle(case, rng, algo, q=q0), _pm_handle(case, rng, algo, learner=False)
    qlds, pmv = cases.pm_expected(cfg, double, _lds_limit())
    _names(a, "pm", cfg, algo, rng, qlds, pmv)
    what = ("pm", case, algo, rng)
    summ = s.episode_summary()
    st, pending, info, rews, rcs = eref.new_state5(N), None, eref.new_info(), [], []
    for launch in range(cases.LAUNCHES):                 # greedy launches from tie-laden random tables
        before = _obs_now(a)
        out = a.rollout_eval(K)
        want, rc, pend_eval, i = eref.eval_run(q0, before, _np(out[0]), _np(out[2]), _np(out[3]), autoreset, pending)
        eref.merge_info(info, i)
        rews.append(_np(out[1])); rcs.append(rc)
        assert np.array_equal(_np(out[4]), want), (what, launch, "greedy actions", np.argwhere(_np(out[4]) != want)[:5])
        _assert_same_outputs(out[:4], b.rollout(out[4]), what + (launch, "eval"))
        assert np.array_equal(_bits(_np(a.get_q())), _bits(q0))
        assert s.rollout_eval(K, summary=summ) is summ
        st, pending = _summary_follows(s, summ, out, st, pending, autoreset, what + (launch, "eval summary"))
        assert np.array_equal(pending, pend_eval)
    _assert_same_handles(a, b, rng)
    cases.eval_flow_honest("pm", case, info, double, np.concatenate(rews), np.concatenate(rcs))
    r = Restated(cfg, algo, seeds=cases.seeds_of(case), autoreset=autoreset, q0=q0)
    r.pending = pending.copy()
    out = _check_launch(a, r, K, what + ("learn after eval",))     # then a learning launch, and its summary form
    _assert_same_outputs(out[:4], b.rollout(out[4]), what + ("learn after eval",))
    assert s.rollout_learn(K, summary=summ) is summ
    st, pending = _summary_follows(s, summ, out, st, pending, autoreset, what + ("learn summary",))
    assert torch.equal(a.get_q().view(torch.int32), s.get_q().view(torch.int32))
    assert st["episodes"].sum() > 0 or case in cases.NO_TERMINAL
    _assert_same_handles(a, b, rng)
    a.close(); s.close(); b.close()


@pytest.mark.parametrize("form,case,algo,rng", [r for r in cases.EVAL_RUNS if r[0] != "pm"])
def test_evaluation_and_summaries_under_levels(form, case, algo, rng):
    per_env = form == "pm_nlev"
    cfg, autoreset, double = cases.CASES[case], _autoreset(case), algo == "double_q"
    q0 = cases.eval_tables(cfg, N, double)
    a, tn, rn = _mixed(case, rng, algo, per_env, q=q0)
    twins = _twins(case, rng, algo, per_env, tn, rn, q=q0)
    what = (form, case, algo, rng)
    befores = []

    def eval_step(e):
        if e is a:
            befores.append(_obs_now(a))
        return e.rollout_eval(K)
    evs = _run_twin_rule(a, twins, rng, what + ("eval",), step=eval_step)         # two greedy launches from tie-laden random tables
    assert np.array_equal(_bits(_np(a.get_q())), _bits(q0))                     # evaluation writes no table
    info, pending, rcs = eref.new_info(), None, []
    for before, ev in zip(befores, evs):
        want, rc, pending, i = eref.eval_run(q0, before, _np(ev[0]), _np(ev[2]), _np(ev[3]), autoreset, pending)
        assert np.array_equal(_np(ev[4]), want), (what, "greedy actions", np.argwhere(_np(ev[4]) != want)[:5])
        eref.merge_info(info, i)
        rcs.append(rc)
    cases.eval_flow_honest(form, case, info, double, np.concatenate([_np(ev[1]) for ev in evs]), np.concatenate(rcs), rn)
    full, _, _ = _mixed(case, rng, algo, per_env, q=q0)                         # the summary forms against the full-output launches
    for ev in evs:
        _same_at(full.rollout_eval(K), ev, ALL, what + ("second mixed handle",))
    summ, st = a.episode_summary(), eref.new_state5(N)
    for call in ("learn", "eval", "learn"):
        assert getattr(a, "rollout_" + call)(K, summary=summ) is summ
        out = getattr(full, "rollout_" + call)(K)
        _same_handles_at(a, full, ALL, rng, what + (call, "summary against full output"))
        st, pending = _summary_follows(a, summ, out, st, pending, autoreset, what + (call, "summary"))
    assert st["episodes"].sum() > 0
    full.close()
    _close(a, twins)


@pytest.mark.parametrize("case,algo,rng", [("d2_s12_a6_L2", "sarsa", "numpy"), ("s4_L4", "q_learning", "philox"), ("trunc_disabled", "double_q", "numpy")])
def test_scheduled_summary_launch_equals_the_full_output_launch(case, algo, rng):
    full, summ = _scheduled(case, rng, algo, "both"), _scheduled(case, rng, algo, "both")
    want = cases.kernel_name("learn", "sched", cases.shared_cfg(case), algo, rng, 1)
    assert summ.learn_kernel_name(K) == want, (summ.learn_kernel_name(K), want)
    s = summ.episode_summary()
    st, pending = eref.new_state5(N), None
    for launch in range(cases.LAUNCHES):
        ep0, epi0 = _np(summ.learner_episodes()), _np(s.episodes)
        out = full.rollout_learn(K)
        assert summ.rollout_learn(K, summary=s) is s
        st, pending = _summary_follows(summ, s, out, st, pending, _autoreset(case), ("sched", case, algo, rng, launch))
        assert torch.equal(summ.get_q().view(torch.int32), full.get_q().view(torch.int32)), (case, launch)
        assert torch.equal(summ.learner_episodes(), full.learner_episodes()), (case, launch)
        # the counter moves as the summary's episodes do
        assert np.array_equal(_np(summ.learner_episodes()) - ep0, _np(s.episodes) - epi0) and (_np(s.episodes) - epi0).any()
    _assert_same_handles(full, summ, rng)
    full.close(); summ.close()


# ---- sizes and one-step launches
@pytest.mark.parametrize("rng", ["numpy", "philox"])
@pytest.mark.parametrize("n", cases.N_EDGES)
def test_sizes_with_a_launch_of_one_step_on_a_reward_matrix_handle(n, rng):
    """tail lanes stage table set N - 1 of a rew_sa handle"""
    case, cfg = "custom_5x3", cases.per_env_cfg("custom_5x3")
    a, b = _pm_handle(case, rng, "q_learning", n=n), _pm_handle(case, rng, "q_learning", n=n, learner=False)
    assert (",PM=2" in a.learn_kernel_name(1)) == (n > 1) and "UNIT=0" in a.learn_kernel_name(1), a.learn_kernel_name(1)
    r = Restated(cfg, "q_learning", seeds=cases.seeds_of(case, n))
    for k in (1, K):
        out = _check_launch(a, r, k, (n, rng, k))
        _assert_same_outputs(out[:4], b.rollout(out[4]), (n, rng, k))
    _assert_same_handles(a, b, rng)
    a.close(); b.close()


@pytest.mark.parametrize("rng", ["numpy", "philox"])
@pytest.mark.parametrize("n", cases.N_EDGES)
def test_sizes_with_a_launch_of_one_step_under_levels(n, rng):
    case = "d2_s12_a6_L2"
    lo = 3 if n == 1 else 0                              # (one env: the env of levels (0.10, 10))
    a, tn, rn = _mixed(case, rng, "q_learning", True, n=n, lo=lo)
    assert (",NLEV=1,PM=" in a.learn_kernel_name(1)) == (n > 1) and ",NLEV=1" in a.learn_kernel_name(1), a.learn_kernel_name(1)
    twins = _twins(case, rng, "q_learning", True, tn, rn, n=n, lo=lo)
    assert len(twins) == min(n, 7)
    for k in (1, K):
        _run_twin_rule(a, twins, rng, (n, rng, k), launches=1, k=k)
    _close(a, twins)


# ---- pieces
@pytest.mark.parametrize("case,algo,rng", [("s4_L4", "sarsa", "numpy"), ("s4_L4", "q_learning", "philox"), ("custom_5x3", "sarsa", "philox"),
                                           ("custom_5x3", "double_q", "numpy")])
def test_a_call_sent_out_in_pieces_of_5_steps_equals_one_launch(case, algo, rng):
    """the hand-over of history bytes 4 to 7 and the ring (s4_L4), of the key ring's head (custom_5x3)"""
    one, many = _pm_handle(case, rng, algo), _pm_handle(case, rng, algo, options=("LEARN_SHORT_PIECES",))
    b = _pm_handle(case, rng, algo, learner=False)
    assert one.learn_kernel_name(K) == many.learn_kernel_name(K) and one.learn_kernel_name(K).endswith("PM=2>")
    r = Restated(cases.per_env_cfg(case), algo, seeds=cases.seeds_of(case))
    rewards = 0
    for launch in range(cases.LAUNCHES):
        want = one.rollout_learn(K)
        got = _check_launch(many, r, K, (case, algo, rng, launch))
        for g, w in zip(got, want):
            assert torch.equal(g, w), (case, algo, rng, launch)
        _assert_same_outputs(got[:4], b.rollout(got[4]), (case, algo, rng, launch))
        rewards += int((_np(got[1]) != 0).sum())
    assert torch.equal(one.get_q().view(torch.int32), many.get_q().view(torch.int32)) and rewards > 0
    _assert_same_handles(one, many, rng)
    _assert_same_handles(many, b, rng)
    one.close(); many.close(); b.close()


# ---- graph replay (the library's capture mode, by graph_replay_util's pattern)
def _graph_replay(make, rng, what, k=9):
    g, e, gs, es = make(), make(), make(), make()
    out = g.alloc_rollout_learn(k)
    want = e.rollout_learn(k)
    got = g.rollout_learn(k, out=out)                    # the eager launch of the same form before the capture
    assert all(torch.equal(x, y) for x, y in zip(got, want))
    cap = gr.capture(g, lambda: g.rollout_learn(k, out=out), k)
    sg, se = gs.episode_summary(), es.episode_summary()
    gs.rollout_learn(k, summary=sg); es.rollout_learn(k, summary=se)
    cap_s = gr.capture(gs, lambda: gs.rollout_learn(k, summary=sg), k)
    for replay in range(3):
        for h in (g, e, gs, es):                         # eager launches in between: the counter moves by 5
            h.rollout_eval(5)
        cap.replay()
        want = e.rollout_learn(k)
        for name, x, y in zip(("obs", "reward", "terminated", "truncated", "actions"), out, want):
            assert torch.equal(x.view(torch.uint8) if x.dtype == torch.bool else x, y.view(torch.uint8) if y.dtype == torch.bool else y), (what, replay, name)
        assert torch.equal(g.get_q().view(torch.int32), e.get_q().view(torch.int32)), (what, replay)
        cap_s.replay()
        es.rollout_learn(k, summary=se)
        for x, y in zip(sg.tensors(), se.tensors()):
            assert torch.equal(x, y), (what, replay, "summary")
        assert torch.equal(gs.get_q().view(torch.int32), es.get_q().view(torch.int32)), (what, replay, "summary")
    g._obs_src = out[0][k - 1]
    _same_handles_at(g, e, np.arange(g.num_envs), rng, what + ("after the replays",))
    assert gr.tick(gs) == gr.tick(es) and not gs.status().any()
    del cap, cap_s
    for h in (g, e, gs, es):
        h.close()


def test_graph_replay_of_a_reward_matrix_handle_in_the_slots():
    make = lambda: _pm_handle("custom_5x3", "philox", "sarsa")
    h = make()
    assert h.learn_kernel_name(9).endswith("PM=2>") and "UNIT=0" in h.learn_kernel_name(9)     # (the key ring in memory)
    h.close()
    _graph_replay(make, "philox", ("custom_5x3",))


def test_graph_replay_under_levels_on_one_mdp_per_env():
    _graph_replay(lambda: _mixed("d2_s12_a6_L2", "numpy", "double_q", True)[0], "numpy", ("d2_s12_a6_L2 levels",))


# ---- shards
@pytest.mark.parametrize("form,algo,rng", [("pm", "sarsa", "numpy"), ("pm", "double_q", "philox"), ("pm_nlev", "q_learning", "numpy"), ("pm_nlev", "sarsa", "philox")])
def test_two_unequal_shards_equal_the_whole(form, algo, rng):
    """custom_13x12 per env: env_id_offset with the seed, level and matrix halves"""
    case = "custom_13x12"
    make = (lambda n, lo: _pm_handle(case, rng, algo, n=n, lo=lo)) if form == "pm" else (lambda n, lo: _mixed(case, rng, algo, True, n=n, lo=lo)[0])
    whole = make(N, 0)
    outs = [whole.rollout_learn(K) for _ in range(2)]
    q = whole.get_q()
    for lo, n in ((0, 97), (97, N - 97)):
        sh = make(n, lo)
        sl = slice(lo, lo + n)
        for launch in range(2):
            for g, w in zip(sh.rollout_learn(K), outs[launch]):
                assert torch.equal(g, w[:, sl]), (form, algo, rng, lo, launch)
        assert torch.equal(sh.get_q().view(torch.int32), q[sl].view(torch.int32))
        sh.close()
    whole.close()
