"""Per-episode epsilon / alpha schedules on the noise-level and per-env-MDP learners on the GPU
(set_learner_schedule(..., sweep=True); the SCHED forms of k_discrete_learn_rollout / k_discrete_learn_summary with NLEV=1 and / or
PM=1|2; include/mdpp.h "Schedules"): a decay schedule over noise levels x seeds in ONE launch.

Every launch is held, bit for bit, to
  the open-loop twin   an unlearned handle of the same config, seeds and streams fed the returned actions through rollout():
                       outputs, state record, both streams, tick -- on a levelled form one such handle per pair of levels, held
                       to the envs at that pair;
  the restatement      tests/learner_schedule_ref.py fed the launch's own outputs, with P per env where the handle has one
                       MDP per env: actions, get_q() and learner_episodes();
  the uniform twins    (levelled forms) env i equals env i of a handle created uniformly at its pair of levels, with the same
                       rows: on a shared MDP the SCHED kernel that needs no opt-in, on one MDP per env the new path;
  the name             computed from the carve and the device's LDS limit: the unscheduled handle's placement and ",SCHED=1".
N = 320, K = 37, two launches, env_id_offset = 1000.  The cases, the schedules and what a pass must have exercised are in
tests/schedule_sweep_cases.py; tests/test_schedule_sweep_host.py shows on the CPU that the conditions can be met.  There is no
tolerance anywhere.  Without the feature every test fails: sweep= is a TypeError."""
import numpy as np
import pytest
import torch

import closed_forms_shape_cases as cfs
import eval_summary_ref as sumref
import graph_replay_util as gr
import learner_schedule_ref as sref
import learner_sweep_ref as ref
import schedule_sweep_cases as cases
import test_gpu_closed_forms_shapes as shapes
import test_gpu_noise_seeds as levels
from test_gpu_closed_loop_shapes import _lds_limit
from test_gpu_learn_rollout import _mk as _mk_shared
from test_gpu_per_env_mdp import _assert_same_handles, _assert_same_outputs, _bits, _np, _obs_now, _tick

pytestmark = pytest.mark.gpu

N, K, OFF, SEED = cases.N, cases.K, cases.OFF, cases.SEED
ALPHA, GAMMA, EPS = cases.ALPHA, cases.GAMMA, cases.EPS
ALL = np.arange(N)
NOT_BUILT = "an epsilon/alpha schedule with per-env noise levels / one MDP per env: not built"
_same_at, _same_handles_at = levels._same_at, levels._same_handles_at


# ---- handles
def _handle(form, case, rng, algo, n=None, lo=0, options=(), pair=None, learner=True, **over):
    """a handle of the form: its learner and, on a levelled form, its levels by the seven-pair cycle -- or, with pair, the
    uniform handle created at that pair"""
    n = N if n is None else n
    cfg, kw = cases.handle_cfg(form, case, pair), cases.kw_of(case)
    per_env = form in cases.PER_ENV_FORMS
    if per_env:
        env = shapes._mk(cfg, rng, cases.seeds_of(case, n, lo), OFF + lo, options, **kw)
    else:
        env = _mk_shared(cfg, rng, n=n, env_id_offset=OFF + lo, **kw)
        if options:
            env.set_kernel_options(*options)
    if learner:
        env.set_learner(algo, **dict(dict(alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=SEED), **over), **(dict(per_env_mdp=True) if per_env else {}))
        if form in cases.LEVEL_FORMS and pair is None:
            tn, rn = cases.level_arrays(n, lo)
            env.set_noise_levels(transition_noise=tn, reward_noise=rn, **(dict(per_env_mdp=True) if per_env else {}))
    return env


def _schedule(env, form, case, kind, lo=0, sweep=True):
    eps, al = cases.tables(form, case, kind)
    env.set_learner_schedule(epsilon=eps, alpha=al, row=cases.rows(env.num_envs, lo), **(dict(sweep=True) if sweep else {}))
    return env


def _scheduled(form, case, rng, algo, kind, n=None, lo=0, options=(), pair=None, **over):
    """... with its schedule; a uniform twin on a shared MDP takes the SCHED form that needs no opt-in"""
    env = _handle(form, case, rng, algo, n, lo, options, pair, **over)
    return _schedule(env, form, case, kind, lo, sweep=not (pair is not None and form == "nlev"))


def _name(form, case, algo, rng, options=(), summary=False, sched=True):
    qlds, pmv = cases.expected_placement(form, case, algo, rng, _lds_limit(), options)
    return cases.kernel_name(form, cases.handle_cfg(form, case), algo, rng, qlds, pmv, summary, sched)


class Restated:
    """the restatement, carried from launch to launch beside a handle"""

    def __init__(self, form, case, algo, kind, n=None, lo=0, sched="case"):
        n = N if n is None else n
        self.P, self.off = cases.P_of(form, case, n, lo), OFF + lo
        self.agent = cases.new_agent(form, case, algo, kind, n, lo, sched)

    def launch(self, tick0, obs_before, out):
        obs, rew, term, trunc = (_np(x) for x in out[:4])
        k, n = obs.shape
        w = [ref.tick_words(SEED, self.off, tick0, k + 1, n, st) for st in (ref.EXPLORE_STREAM, ref.ACTION_STREAM, ref.UPDATE_STREAM)]
        return sref.run(self.agent, obs_before, obs, rew, term, trunc, self.P, *w)


def _check_launch(a, r, k, what):
    """one learning launch of handle a against the restatement r (actions, tables, counters); returns (outputs, obs before)"""
    before, tick0 = _obs_now(a), _tick(a)
    out = a.rollout_learn(k)
    want = r.launch(tick0, before, out)
    got = _np(out[4])
    assert np.array_equal(got, want), (what, "actions", np.argwhere(got != want)[:5])
    assert np.array_equal(_bits(_np(a.get_q())), _bits(r.agent.Q)), (what, "Q")
    assert np.array_equal(_np(a.learner_episodes()), r.agent.ep), (what, "episodes", np.argwhere(_np(a.learner_episodes()) != r.agent.ep)[:5])
    return out, before


def _equal_launches(a, b, launches, what, k=K, rng=None):
    for launch in range(launches):
        for name, g, w in zip(("obs", "reward", "terminated", "truncated", "actions"), a.rollout_learn(k), b.rollout_learn(k)):
            assert torch.equal(g, w), (what, launch, name)
    assert torch.equal(a.get_q().view(torch.int32), b.get_q().view(torch.int32)), what
    if rng is not None:
        _assert_same_handles(a, b, rng)


def _same_outputs_at(got, want, at, what):
    """(obs, reward, terminated, truncated) of two launches, equal at the envs `at` (reward by bits)"""
    for name, g, w in zip(("obs", "reward", "terminated", "truncated"), got, want):
        g, w = _np(g)[:, at], _np(w)[:, at]
        if name == "reward":
            g, w = _bits(g), _bits(w)
        assert g.shape == w.shape and np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5])


def _close(*handles):
    for e in handles:
        assert not e.status().any()
        e.close()


# ---- twins, restatement, name
@pytest.mark.parametrize("form,case,algo,rng", cases.RUNS)
def test_scheduled_launch_open_loop_twin_restatement_uniform_twins_and_name(form, case, algo, rng):
    from mdp_playground_amd import _capi as capi
    kind = cases.kind_of(form, case, algo, rng)
    what = (form, case, algo, rng, kind)
    a = _scheduled(form, case, rng, algo, kind)
    assert a.learn_kernel_name(K) == _name(form, case, algo, rng), (a.learn_kernel_name(K), _name(form, case, algo, rng))
    assert "SCHED" not in a.eval_kernel_name(K)
    cases.triples_honest(form, case, N)
    tn, rn = cases.levels_of(form, N)
    if form in cases.LEVEL_FORMS:
        pairs = cases.pairs_present(tn, rn)
        assert len(pairs) == 7
        at = {p: np.flatnonzero((tn == p[0]) & (rn == p[1])) for p in pairs}
        open_loop = {p: _handle(form, case, rng, algo, pair=p, learner=False) for p in pairs}
        uniform = {p: _scheduled(form, case, rng, algo, kind, pair=p) for p in pairs}
        for p, u in uniform.items():
            name = u.learn_kernel_name(K)
            assert name.endswith(",SCHED=1>") and "NLEV" not in name and (",PM=" in name) == (form == "pm_nlev"), name
    else:
        at, open_loop, uniform = {None: ALL}, {None: _handle(form, case, rng, algo, learner=False)}, {}
    space_before = a.get_rng_streams(capi.STREAM_SPACE).copy() if rng == "numpy" else None
    r = Restated(form, case, algo, kind)
    outs, befores = [], []
    for launch in range(cases.LAUNCHES):
        assert _tick(a) == launch * K
        out, before = _check_launch(a, r, K, what + (launch,))
        for p, b in open_loop.items():
            _same_outputs_at(out[:4], b.rollout(out[4]), at[p], what + (p, launch, "open loop"))
        for p, u in uniform.items():
            _same_at(out, u.rollout_learn(K), at[p], what + (p, launch, "uniform twin"))
            _same_handles_at(a, u, at[p], rng, what + (p, launch, "uniform twin"))
            assert np.array_equal(_np(a.learner_episodes())[at[p]], _np(u.learner_episodes())[at[p]]), what + (p, launch)
        outs.append(out); befores.append(before)
    # the open-loop twin's state record, streams and tick
    for p, b in open_loop.items():
        sa, sb = a.get_augmented_state(), b.get_augmented_state()
        assert sa.keys() == sb.keys()
        for key in sa:
            assert np.array_equal(sa[key][at[p]], sb[key][at[p]]), what + (p, key)
        if rng == "numpy":
            for st in (capi.STREAM_ENV, capi.STREAM_SPACE):
                assert np.array_equal(a.get_rng_streams(st)[at[p]], b.get_rng_streams(st)[at[p]]), what + (p, "stream", st)
        assert _tick(a) == _tick(b)
    # what the pass must have exercised
    mdps = cases.mdps_of(form, case)
    # (s8_noise is not a case of closed_forms_shape_cases, whose names the helper goes by: it borrows one with its autoreset mode)
    f = shapes._flow(case if case in cfs.CASES else "d2_s12_a6_L2", befores, outs, mdps if form in cases.PER_ENV_FORMS else mdps[:1])
    P = np.stack([np.asarray(m.P) for m in mdps]) if form in cases.PER_ENV_FORMS else np.asarray(mdps[0].P)
    cases.honest(form, case, algo, kind, r.agent.info, r.agent.ep, r.agent.sched.row, f["state"], f["actions"], f["next_state"], f["seen"], tn, P)
    if rng == "numpy" and form in cases.LEVEL_FORMS:
        # an env of level 0, whose space stream did not move, beside one whose stream did
        moved = (a.get_rng_streams(capi.STREAM_SPACE) != space_before).reshape(N, -1).any(axis=1)
        assert not moved[tn == 0].any()
        assert ((tn[1:] == 0) & moved[:-1]).any() or ((tn[:-1] == 0) & moved[1:]).any()
    print(what, a.learn_kernel_name(K), "ep", r.agent.ep.min(), r.agent.ep.max())
    _close(a, *open_loop.values(), *uniform.values())


# ---- equivalences, per form
_EQ = [(form, algo) for form in cases.FORMS for algo in ("sarsa", "double_q")]


@pytest.mark.parametrize("form,algo", [(form, algo) for form in cases.FORMS for algo in cases.ALGOS])
def test_constant_tables_give_the_same_handle_without_a_schedule(form, algo):
    case, rng = "d2_s12_a6_L2", "numpy"
    plain, sc = _handle(form, case, rng, algo), _handle(form, case, rng, algo, alpha=0.7, epsilon=0.9)     # (both overridden by the tables)
    sc.set_learner_schedule(epsilon=np.full(3, EPS), alpha=np.full(3, ALPHA), sweep=True)
    assert plain.learn_kernel_name(K) == _name(form, case, algo, rng, sched=False) and sc.learn_kernel_name(K) == _name(form, case, algo, rng)
    _equal_launches(sc, plain, 2, (form, algo), rng=rng)
    assert _np(sc.learner_episodes()).max() > 3
    _close(plain, sc)


@pytest.mark.parametrize("rng", cases.RNGS)
@pytest.mark.parametrize("form,algo", _EQ)
def test_summary_launch_equals_the_full_output_launch(form, algo, rng):
    case = cases.FORM_CASES[form][-1]                    # the form's truncation case
    full, summ = _scheduled(form, case, rng, algo, "both"), _scheduled(form, case, rng, algo, "both")
    assert summ.learn_kernel_name(K) == _name(form, case, algo, rng)
    s = summ.episode_summary()
    st5, pending = sumref.new_state5(N), None
    for launch in range(cases.LAUNCHES):
        ep0, epi0 = _np(summ.learner_episodes()), _np(s.episodes)
        out = full.rollout_learn(K)
        assert summ.rollout_learn(K, summary=s) is s
        reset_call, pending = sumref.reset_calls(_np(out[2]), _np(out[3]), cases.autoreset_of(case), pending)
        st5 = sumref.summary(_np(out[1]), _np(out[2]), _np(out[3]), reset_call, st5)
        for (name, _), t in zip(sumref.FIELDS, s.tensors()):
            g, w = _np(t), st5[name]
            assert np.array_equal(g.view(np.int64) if g.dtype == np.float64 else g, w.view(np.int64) if w.dtype == np.float64 else w), (form, launch, name)
        assert torch.equal(summ.get_q().view(torch.int32), full.get_q().view(torch.int32)), (form, launch)
        assert torch.equal(summ.learner_episodes(), full.learner_episodes()), (form, launch)
        # the counter moves as the summary's episodes do
        assert np.array_equal(_np(summ.learner_episodes()) - ep0, _np(s.episodes) - epi0) and (_np(s.episodes) - epi0).any()
    _assert_same_handles(full, summ, rng)
    _close(full, summ)


_OPTIONS = {"nlev": ("LEARN_SHORT_PIECES", "NO_LEARN_LDS", "NO_NLEV_LDS"),
            "pm": ("LEARN_SHORT_PIECES", "NO_LEARN_LDS", "NO_PM_LDS"),
            "pm_nlev": ("LEARN_SHORT_PIECES", "NO_LEARN_LDS", "NO_PM_LDS", "NO_PM_NLEV_LDS")}


@pytest.mark.parametrize("form,algo", _EQ)
def test_pieces_and_every_forced_placement_equal_the_default(form, algo):
    case, rng = "d2_s12_a6_L2", "numpy"                  # (numpy streams: the cdfs have an LDS placement to be forced out of)
    one = _scheduled(form, case, rng, algo, "both")
    others = [_scheduled(form, case, rng, algo, "both", options=(o,)) for o in _OPTIONS[form]]
    others.append(_scheduled(form, case, rng, algo, "both", options=tuple(o for o in _OPTIONS[form] if o != "LEARN_SHORT_PIECES")))
    names = {one.learn_kernel_name(K)}
    for o, e in zip(_OPTIONS[form], others):
        placed = () if o == "LEARN_SHORT_PIECES" else (o,)
        assert e.learn_kernel_name(K) == _name(form, case, algo, rng, placed), (o, e.learn_kernel_name(K))
        names.add(e.learn_kernel_name(K))
    assert len(names) >= 2                               # (a forced placement launches another kernel)
    summaries = [e.episode_summary() for e in [one] + others]
    for launch in range(2):
        want = one.rollout_learn(K)
        for j, e in enumerate(others):
            _same_at(e.rollout_learn(K), want, ALL, (form, algo, j, launch))
            _same_handles_at(e, one, ALL, rng, (form, algo, j, launch))
            assert torch.equal(e.learner_episodes(), one.learner_episodes()), (form, algo, j, launch)
    # ... and keeping summaries
    for e, s in zip([one] + others, summaries):
        e.rollout_learn(K, summary=s)
    for j, (e, s) in enumerate(zip(others, summaries[1:])):
        for g, w in zip(s.tensors(), summaries[0].tensors()):
            assert torch.equal(g, w), (form, algo, j)
        assert torch.equal(e.learner_episodes(), one.learner_episodes()) and torch.equal(e.get_q().view(torch.int32), one.get_q().view(torch.int32))
    _close(one, *others)


@pytest.mark.parametrize("form,algo", _EQ)
def test_counters_beyond_the_table_hold_the_last_entries(form, algo):
    case, rng = cases.FORM_CASES[form][-1], "philox"
    m = cases.sched_m(form, case)
    a = _scheduled(form, case, rng, algo, "both")
    a.set_learner_episodes(np.full(N, m + 3))
    assert (_np(a.learner_episodes()) == m + 3).all()
    eps, al = cases.tables(form, case, "both")
    row = cases.rows(N)
    last = _handle(form, case, rng, algo, alpha=al[row, -1], epsilon=eps[row, -1])
    assert "SCHED" not in last.learn_kernel_name(K)
    _equal_launches(a, last, 2, (form, algo, "held at the last entries"), rng=rng)
    assert (_np(a.learner_episodes()) > m + 3).all()
    _close(a, last)


@pytest.mark.parametrize("form,algo", [(form, algo) for form in cases.FORMS for algo in ("q_learning", "double_q")])
def test_evaluation_reads_no_table_and_moves_no_counter(form, algo):
    case, rng = "d2_s12_a6_L2", "numpy"
    a = _scheduled(form, case, rng, algo, "both")
    a.rollout_learn(K)
    # (under levels no handle can be fed a's actions open loop: the scheduled handle c and the unscheduled handle b both
    #  evaluate a's tables from a fresh env state, c with a's counters)
    b, c = _handle(form, case, rng, algo), _scheduled(form, case, rng, algo, "both")
    q = a.get_q()
    c.set_q(q); b.set_q(q)
    c.set_learner_episodes(a.learner_episodes())
    ep, sched = c.learner_episodes(), c.learner_schedule()
    assert _np(ep).any()
    for name, g, w in zip(("obs", "reward", "terminated", "truncated", "actions"), c.rollout_eval(K), b.rollout_eval(K)):
        assert torch.equal(g, w), (form, algo, name)
    sc, sb = c.episode_summary(), b.episode_summary()
    c.rollout_eval(K, summary=sc); b.rollout_eval(K, summary=sb)
    for g, w in zip(sc.tensors(), sb.tensors()):
        assert torch.equal(g, w)
    assert _np(sc.episodes).any()
    assert torch.equal(c.learner_episodes(), ep) and torch.equal(c.get_q().view(torch.int32), q.view(torch.int32))
    now = c.learner_schedule()
    assert all(np.array_equal(now[k], sched[k]) for k in sched)
    assert c.eval_kernel_name(K) == b.eval_kernel_name(K) and "SCHED" not in c.eval_kernel_name(K)
    assert c.learn_kernel_name(K) == _name(form, case, algo, rng)
    _assert_same_handles(c, b, rng)
    _close(a, b, c)


@pytest.mark.parametrize("n", [1, 63, 257])
@pytest.mark.parametrize("form", cases.FORMS)
def test_sizes_with_a_launch_of_one_step(form, n):
    case, algo, rng = "s8_noise", "sarsa", "numpy"
    a = _scheduled(form, case, rng, algo, "both", n=n)
    r = Restated(form, case, algo, "both", n=n)
    for launch in range(3):
        _check_launch(a, r, 1, (form, n, launch))
    _close(a)


@pytest.mark.parametrize("rng", cases.RNGS)
@pytest.mark.parametrize("form,algo", _EQ)
def test_two_unequal_shards_with_their_rows_levels_and_seeds_equal_the_whole(form, algo, rng):
    case = "s8_noise"
    whole = _scheduled(form, case, rng, algo, "both")
    outs = [whole.rollout_learn(K) for _ in range(2)]
    q, ep = whole.get_q(), whole.learner_episodes()
    for lo, n in ((0, 97), (97, 223)):
        sl = slice(lo, lo + n)
        sh = _scheduled(form, case, rng, algo, "both", n=n, lo=lo)
        assert np.array_equal(sh.learner_schedule()["row"], cases.rows(N)[sl])
        for launch in range(2):
            for g, w in zip(sh.rollout_learn(K), outs[launch]):
                assert torch.equal(g, w[:, sl]), (form, algo, rng, lo, launch)
        assert torch.equal(sh.get_q().view(torch.int32), q[sl].view(torch.int32)) and torch.equal(sh.learner_episodes(), ep[sl])
        _close(sh)
    _close(whole)


# ---- graph replay
@pytest.mark.parametrize("summary", [False, True])
@pytest.mark.parametrize("form", cases.FORMS)
def test_captured_launch_continues_the_schedule_at_every_replay(form, summary):
    case, algo, rng = cases.FORM_CASES[form][-1], "sarsa", "philox"
    a, b = _scheduled(form, case, rng, algo, "both"), _scheduled(form, case, rng, algo, "both")
    sa, sb = (a.episode_summary(), b.episode_summary()) if summary else (None, None)
    out_a = None if summary else a._alloc_rollout_closed(K)

    def call(e, s, out=None):
        return e.rollout_learn(K, summary=s) if summary else e.rollout_learn(K, out)

    call(a, sa, out_a); call(b, sb)                         # the eager launch before the capture (fills, LDS attribute)
    g = gr.capture(a, lambda: call(a, sa, out_a), K)
    for replay in range(3):
        ep0 = _np(a.learner_episodes())
        g.replay()
        out_b = call(b, sb)
        if summary:
            for x, y in zip(sa.tensors(), sb.tensors()):
                assert torch.equal(x, y), replay
        else:
            for name, x, y in zip(("obs", "reward", "terminated", "truncated", "actions"), out_a, out_b):
                assert torch.equal(x.view(torch.uint8) if x.dtype == torch.bool else x, y.view(torch.uint8) if y.dtype == torch.bool else y), (replay, name)
        assert torch.equal(a.get_q().view(torch.int32), b.get_q().view(torch.int32)), replay
        assert torch.equal(a.learner_episodes(), b.learner_episodes()), replay
        assert (_np(a.learner_episodes()) > ep0).all(), replay                 # (max_episode_steps = 5: every env ends episodes in 37 steps)
        # the counter moves between the replays too: five eager steps on both handles
        for x, y in zip(a.rollout_learn(5), b.rollout_learn(5)):
            assert torch.equal(x, y), replay
    assert _tick(a) == _tick(b) == 4 * K + 15
    _assert_same_handles(a, b, rng)
    assert (_np(a.learner_episodes()) >= cases.sched_m(form, case)).any()
    _close(a, b)


# ---- the opt-in
@pytest.mark.parametrize("form", cases.FORMS)
def test_without_the_opt_in_the_refusals_stand_and_leave_what_is_in_force(form):
    case, algo, rng = "s8_noise", "q_learning", "numpy"
    per_env = form in cases.PER_ENV_FORMS
    a = _handle(form, case, rng, algo)
    name = a.learn_kernel_name(K)
    assert "SCHED" not in name
    with pytest.raises(NotImplementedError, match=NOT_BUILT):
        a.set_learner_schedule(epsilon=[0.5, 0.1])
    assert a.learner_schedule() is None and a.learn_kernel_name(K) == name
    # the library's own refusal, and what the flag changes
    assert a._lib.mdpp_learner_schedule_sweep(a._h, 0) == 0
    eps = np.array([0.5, 0.1], np.float32)
    from mdp_playground_amd import _capi as capi
    assert a._lib.mdpp_set_learner_schedule(a._h, capi.nptr(eps), None, 1, 2, None, None) == capi.EUNSUPPORTED
    assert NOT_BUILT.encode() in a._lib.mdpp_last_error(a._h)
    a.rollout_learn(5)
    # with it: the schedule on the form's own kernel; a call without it is refused and what is in force stays
    _schedule(a, form, case, "both")
    assert a.learn_kernel_name(K) == _name(form, case, algo, rng)
    with pytest.raises(NotImplementedError, match=NOT_BUILT):
        a.set_learner_schedule(epsilon=[0.5, 0.1])
    assert a.learn_kernel_name(K) == _name(form, case, algo, rng) and a.learner_schedule()["epsilon"].shape == (4, cases.sched_m(form, case))
    a.rollout_learn(5)
    assert _np(a.learner_episodes()).any()
    # clear_learner_schedule: back to the unscheduled name, and the opt-in is gone
    a.clear_learner_schedule()
    assert a.learner_schedule() is None and a.learn_kernel_name(K) == name
    with pytest.raises(NotImplementedError, match=NOT_BUILT):
        a.set_learner_schedule(epsilon=[0.5, 0.1])
    # set_learner drops the schedule and leaves the flag: the library accepts a schedule at once
    _schedule(a, form, case, "eps")
    a.set_learner(algo, alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=SEED, **(dict(per_env_mdp=True) if per_env else {}))
    assert a.learner_schedule() is None and "SCHED" not in a.learn_kernel_name(K)
    assert a._lib.mdpp_set_learner_schedule(a._h, capi.nptr(eps), None, 1, 2, None, None) == 0
    assert a.learn_kernel_name(K).endswith(",SCHED=1>")
    # the flag off drops a schedule that runs with levels or one MDP per env
    assert a._lib.mdpp_learner_schedule_sweep(a._h, 0) == 0
    assert a.learn_kernel_name(K) == name
    a.rollout_learn(5)
    _close(a)


@pytest.mark.parametrize("algo", ["q_learning", "double_q"])
def test_schedule_then_levels_and_levels_then_schedule_launch_the_same(algo):
    form, case, rng = "nlev", "s8_noise", "numpy"
    tn, rn = cases.level_arrays(N)
    first = _scheduled(form, case, rng, algo, "both")                       # levels, then the schedule
    second = _mk_shared(cases.handle_cfg(form, case), rng, n=N, env_id_offset=OFF)
    second.set_learner(algo, alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=SEED)
    _schedule(second, form, case, "both")                                   # sweep=True on a plain handle: today's kernel
    assert second.learn_kernel_name(K).endswith(",PE=1%s,SCHED=1>" % (",DOUBLE=1" if algo == "double_q" else "")) and "NLEV" not in second.learn_kernel_name(K)
    second.set_noise_levels(transition_noise=tn, reward_noise=rn)           # ... then the levels, accepted under the opt-in
    assert second.learn_kernel_name(K) == first.learn_kernel_name(K) == _name(form, case, algo, rng)
    _equal_launches(first, second, 2, (algo, "both orders"), rng=rng)
    assert torch.equal(first.learner_episodes(), second.learner_episodes())
    # a schedule set without the opt-in still refuses levels, and the flag off keeps a schedule that runs alone
    third = _mk_shared(cases.handle_cfg(form, case), rng, n=N, env_id_offset=OFF)
    third.set_learner(algo, alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=SEED)
    _schedule(third, form, case, "both", sweep=False)
    with pytest.raises(NotImplementedError, match=NOT_BUILT):
        third.set_noise_levels(transition_noise=tn, reward_noise=rn)
    _schedule(third, form, case, "both")
    assert third._lib.mdpp_learner_schedule_sweep(third._h, 0) == 0
    assert third.learn_kernel_name(K).endswith(",SCHED=1>")                 # (no levels, a shared MDP: nothing to drop)
    _close(first, second, third)


def test_schedule_then_the_per_env_mdp_learner_is_accepted_by_the_library_under_the_flag():
    from mdp_playground_amd import _capi as capi
    form, case, rng, algo = "pm", "s8_noise", "numpy", "q_learning"
    a = _handle(form, case, rng, algo)
    _schedule(a, form, case, "both")
    assert a._lib.mdpp_learner_per_env_mdp(a._h, 1) == 0                    # on while a sweep schedule is in force: accepted
    assert a.learn_kernel_name(K) == _name(form, case, algo, rng)
    a.rollout_learn(5)
    # a continuous handle: the flag call is accepted and changes nothing
    from test_gpu_learn_rollout import _CONT
    from mdp_playground_amd import RLToyVectorEnv
    c = RLToyVectorEnv(num_envs=64, **_CONT)
    assert c._lib.mdpp_learner_schedule_sweep(c._h, 1) == 0
    with pytest.raises(NotImplementedError, match="discrete"):
        c.set_learner_schedule(epsilon=[0.5, 0.1], sweep=True)
    assert capi.EUNSUPPORTED != 0
    c.close()
    _close(a)
