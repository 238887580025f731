"""Per-env noise levels of grid handles on the GPU (k_grid_learn_nlev_rollout, k_grid_learn_nlev_sched_rollout,
k_grid_learn_nlev_log_rollout; include/mdpp.h "Grid noise levels"): RLToyVectorEnv.set_grid_noise_levels / grid_noise_levels /
clear_grid_noise_levels under rollout_grid_learn / rollout_grid_eval and their summary=, log= and scheduled forms.

Every case of tests/grid_noise_level_cases.py x {numpy, philox} x {q_learning, sarsa} runs at N = 320, K = 37, two launches, and
the mixed handle is held to (a) one uniform handle per pair, created at that pair, on the pair's envs -- outputs, action
vectors, Q as int32 bits, the state record, the stream words (numpy handles: a Philox handle keeps none), status and tick --,
(b) the CPU composition tests/grid_noise_levels_ref.py on Philox streams, (c) the kernel's name with ",NLEV=1" and (d) the
open-loop rule on each uniform twin.  Nothing here has a tolerance: every comparison is bit for bit.
tests/test_grid_noise_levels_host.py shows on the CPU that the cases exercise what a pass claims."""
import ctypes as C

import numpy as np
import pytest
import torch

import episode_log_ref as lref
import eval_summary_ref as eref
import graph_replay_util as gru
import grid_learner_ref as gref
import grid_noise_level_cases as nc
import grid_noise_levels_ref as nref

pytestmark = pytest.mark.gpu

N, K = nc.N, nc.K
SEED = nc.LEARNER_SEED
M_LOG = 3
SENT_RET, SENT_LEN = -7.5, -7
EINVAL, ESTATE = -1, -4       # MDPP_EINVAL, MDPP_ESTATE
ONLY = "grid noise levels: learner and evaluation launches only; clear_grid_noise_levels\\(\\) first"


def _mk(case, rng, n=N, cfg=None, **over):
    from mdp_playground_amd import RLToyVectorEnv
    c = nc.CASES[case]
    extra = dict(rng="philox", philox_seed=nc.PHILOX_SEED) if rng == "philox" else {}
    return RLToyVectorEnv(num_envs=n, env_id_offset=nc.ENV_ID_OFFSET, **extra, **dict(c["kw"], **over), **(c["cfg"] if cfg is None else cfg))


def _learner(env, case, algo):
    al, ga, ep = nc.CASES[case]["rates"]
    env.set_grid_learner(algo, alpha=al, gamma=ga, epsilon=ep, seed=SEED, noop=nc.CASES[case]["noop"])


def _mixed(case, rng, algo, n=N, **over):
    """the case's handle with its learner and its levels"""
    a = _mk(case, rng, n, **over)
    _learner(a, case, algo)
    a.set_grid_noise_levels(**nc.levels(case, n))
    return a


def _uniform(case, pair, rng, algo=None, n=N, **over):
    """a handle created uniformly at `pair` (algo: with the case's learner)"""
    u = _mk(case, rng, n, cfg=nc.uniform_cfg(case, pair), **over)
    if algo is not None:
        _learner(u, case, algo)
    return u


def _np(x):
    return x.cpu().numpy().copy() if torch.is_tensor(x) else np.asarray(x)


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def _assert_same_outputs(got, want, what, mine=None):
    """obs, reward (as bits), terminated, truncated[, actions], on the envs `mine` (all)"""
    for name, g, w in zip(("obs", "reward", "terminated", "truncated", "actions"), got, want):
        g, w = _np(g), _np(w)
        if name == "reward":
            g, w = _bits(g.astype(np.float32)), _bits(w.astype(np.float32))
        assert g.shape == w.shape, (what, name)
        if mine is not None:
            g, w = g[:, mine], w[:, mine]
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5])


def _assert_same_handles(a, b, rng, what, mine=None):
    """the state record, the three stream records (numpy), status and tick"""
    from mdp_playground_amd import _capi as capi
    mine = slice(None) if mine is None else mine
    sa, sb = a.get_augmented_state(), b.get_augmented_state()
    assert sa.keys() == sb.keys()
    for k in sa:
        assert np.array_equal(sa[k][mine], sb[k][mine]), (what, k)
    if rng == "numpy":
        for st in (capi.STREAM_ENV, capi.STREAM_SPACE, capi.STREAM_ACTION):
            assert np.array_equal(a.get_rng_streams(st)[mine], b.get_rng_streams(st)[mine]), (what, st)
    assert not a.status()[mine].any() and not b.status()[mine].any(), what
    assert gru.tick(a) == gru.tick(b), what


def _assert_same_q(a, want, what, mine=None):
    q = _np(a.get_grid_q()) if not isinstance(a, np.ndarray) else a
    w = _np(want.get_grid_q()) if not isinstance(want, np.ndarray) else want
    if mine is not None:
        q, w = q[mine], w[mine]
    assert q.shape == w.shape and np.array_equal(_bits(q), _bits(w)), (what, np.argwhere(_bits(q) != _bits(w))[:5])


def _state5(s):
    return {name: _np(t) for (name, _), t in zip(lref.FIELDS5, s.tensors())}


def _log3(lg):
    return {k: _np(t) for k, t in zip(("count", "ret", "len"), lg.tensors())}


def _new_log(env, m=M_LOG):
    lg = env.episode_log(m)
    lg.ret.fill_(SENT_RET)
    lg.len.fill_(SENT_LEN)
    return lg


def _assert_same5(s, want, what, mine=None):
    got = _state5(s) if not isinstance(s, dict) else s
    mine = slice(None) if mine is None else mine
    for name, _ in lref.FIELDS5:
        g, w = got[name][mine], want[name][mine]
        assert g.dtype == w.dtype and np.array_equal(g.view(np.uint8), w.view(np.uint8)), (what, name)


def _assert_same_log(lg, want, what, mine=None):
    got = _log3(lg) if not isinstance(lg, dict) else lg
    for name in ("count", "ret", "len"):
        g, w = got[name], want[name]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        if mine is not None:
            g, w = g[..., mine], w[..., mine]
        assert np.array_equal(np.ascontiguousarray(g).view(np.uint8), np.ascontiguousarray(w).view(np.uint8)), (what, name)


def _close(*envs):
    for e in envs:
        e.close()


# ---- 1. the cases: uniform twins, restatement, name, open-loop rule
@pytest.mark.parametrize("case", sorted(nc.CASES))
def test_mixed_handle_twins_restatement_name_and_open_loop_rule(case):
    """every case x {numpy, philox} x {q_learning, sarsa} (one test per case: the suite's count of GPU tests stays small)"""
    for rng in ("numpy", "philox"):
        for algo in gref.ALGOS:
            _mixed_handle_twins_restatement_name_and_open_loop_rule(case, rng, algo)


def _mixed_handle_twins_restatement_name_and_open_loop_rule(case, rng, algo):
    c = nc.CASES[case]
    idx = nc.pair_index(case)
    a = _mixed(case, rng, algo)
    # (c) the names
    assert a.grid_learn_kernel_name(K) == nc.expected_name(case, rng), a.grid_learn_kernel_name(K)
    assert a.grid_learn_kernel_name(K, summary=True) == nc.expected_name(case, rng, summary=True)
    assert a.grid_learn_kernel_name(K, eval=True) == nc.expected_name(case, rng, eval=True)
    assert a.grid_learn_kernel_name(K, eval=True, summary=True) == nc.expected_name(case, rng, eval=True, summary=True)
    tn, rn = a.grid_noise_levels()
    lv = nc.levels(case)
    assert np.array_equal(tn, lv["transition_noise"] if lv["transition_noise"] is not None else np.zeros(N))
    assert np.array_equal(rn, lv["reward_noise"] if lv["reward_noise"] is not None else np.zeros(N))
    twins = [(_uniform(case, pair, rng, algo), _uniform(case, pair, rng)) for pair in c["pairs"]]      # (learner twin, open-loop twin)
    for pair, (u, o) in zip(c["pairs"], twins):
        assert u.grid_learn_kernel_name(K) == nc.uniform_name(case, pair, rng), (pair, u.grid_learn_kernel_name(K))
    if rng == "philox":
        infos, Q, traj = nref.cpu_run(case, algo)
        assert np.array_equal(_np(a._obs), traj["obs0"])
    for launch in range(nc.LAUNCHES):
        out = a.rollout_grid_learn(K)
        if rng == "philox":                                         # (b) the CPU composition
            sl = slice(launch * K, (launch + 1) * K)
            _assert_same_outputs(out, (traj["obs"][sl], traj["reward"][sl], traj["terminated"][sl], traj["truncated"][sl], traj["vectors"][sl]),
                                 (case, rng, algo, launch, "composition"))
        for j, (u, o) in enumerate(twins):
            what = (case, rng, algo, launch, c["pairs"][j])
            _assert_same_outputs(out, u.rollout_grid_learn(K), what + ("twin",), idx == j)             # (a)
            _assert_same_outputs(out[:4], o.rollout(out[4]), what + ("open loop",), idx == j)          # (d)
    for j, (u, o) in enumerate(twins):
        what = (case, rng, algo, c["pairs"][j])
        _assert_same_q(a, u, what, idx == j)
        _assert_same_handles(a, u, rng, what + ("twin",), idx == j)
        _assert_same_handles(a, o, rng, what + ("open loop",), idx == j)
    if rng == "philox":
        _assert_same_q(a, gref.as_grid(Q, c["cfg"]["grid_shape"]), (case, rng, algo, "composition"))
    _close(a, *[e for t in twins for e in t])


# ---- 2. boundaries
def test_small_and_ragged_sizes_and_launches_of_one_step():
    case, algo = "g34_both", "sarsa"
    for n in (1, 63, 257):
        idx = nc.pair_index(case, n)
        for rng in ("numpy", "philox"):
            a = _mixed(case, rng, algo, n=n)
            twins = [_uniform(case, pair, rng, algo, n=n) for pair in nc.CASES[case]["pairs"]]
            for k in (1, 7, 1, 7):
                out = a.rollout_grid_learn(k)
                for j, u in enumerate(twins):
                    _assert_same_outputs(out, u.rollout_grid_learn(k), (n, rng, k, j), idx == j)
            for j, u in enumerate(twins):
                _assert_same_q(a, u, (n, rng, j), idx == j)
                _assert_same_handles(a, u, rng, (n, rng, j), idx == j)
            _close(a, *twins)


def test_one_pair_everywhere_equals_the_uniform_handles_existing_kernel():
    case, algo = "g34_both", "sarsa"
    for rng in ("numpy", "philox"):
        for pair in nc.CASES[case]["pairs"]:
            a, u = _mk(case, rng), _uniform(case, pair, rng, algo)
            _learner(a, case, algo)
            a.set_grid_noise_levels(transition_noise=pair[0], reward_noise=np.full(N, pair[1]))        # a scalar is broadcast
            assert "NLEV=1" in a.grid_learn_kernel_name(K) and "NLEV" not in u.grid_learn_kernel_name(K)
            for launch in range(2):
                _assert_same_outputs(a.rollout_grid_learn(K), u.rollout_grid_learn(K), (rng, pair, launch))
            _assert_same_q(a, u, (rng, pair))
            _assert_same_handles(a, u, rng, (rng, pair))
            _close(a, u)


def test_levels_equal_to_the_creation_values_equal_the_handle_before_the_call():
    case, algo = "g34_both", "q_learning"
    cfg = nc.CASES[case]["cfg"]
    for rng in ("numpy", "philox"):
        a, b = _mk(case, rng), _mk(case, rng)
        for env in (a, b):
            _learner(env, case, algo)
        a.set_grid_noise_levels(transition_noise=cfg["transition_noise"], reward_noise=cfg["reward_noise"])
        assert "NLEV=1" in a.grid_learn_kernel_name(K) and b.grid_learn_kernel_name(K) == nc.uniform_name(case, (0.2, 0.25), rng)
        for launch in range(2):
            _assert_same_outputs(a.rollout_grid_learn(K), b.rollout_grid_learn(K), (rng, launch))
        _assert_same_q(a, b, rng)
        _assert_same_handles(a, b, rng, rng)
        _close(a, b)


# ---- 3. forms
def test_evaluation_leaves_q_alone_and_steps_with_the_lanes_own_noise():
    for case, rng in (("g34_both", "numpy"), ("g17_both_i32", "philox"), ("g55_noop_next_ponly", "philox"), ("g88_disabled_ronly", "numpy")):
        algo, c, idx = "q_learning", nc.CASES[case], nc.pair_index(case)
        a = _mixed(case, rng, algo)
        twins = [_uniform(case, pair, rng, algo) for pair in c["pairs"]]
        out = a.rollout_grid_learn(K)                               # (tables worth evaluating)
        for j, u in enumerate(twins):
            _assert_same_outputs(out, u.rollout_grid_learn(K), (case, "learn", j), idx == j)
        q = _np(a.get_grid_q())
        assert q.any()
        assert a.grid_learn_kernel_name(K, eval=True) == nc.expected_name(case, rng, eval=True)
        out = a.rollout_grid_eval(K)
        s = a.episode_summary()
        assert a.rollout_grid_eval(K, summary=s) is s
        _assert_same_q(_np(a.get_grid_q()), q, (case, "evaluation left the tables alone"))
        rew = _np(out[1])
        for j, u in enumerate(twins):
            mine = idx == j
            _assert_same_outputs(out, u.rollout_grid_eval(K), (case, rng, "eval", j), mine)
            su = u.episode_summary()
            u.rollout_grid_eval(K, summary=su)
            _assert_same5(s, _state5(su), (case, rng, "eval summary", j), mine)
            _assert_same_handles(a, u, rng, (case, rng, "eval", j), mine)
            sigma = c["pairs"][j][1]
            if sigma is not None:                                   # the lane's own sigma: noisy rewards iff it is above 0
                assert (~np.isin(rew[:, mine], nref.noiseless_lattice(c["cfg"]))).any() == (sigma > 0), (case, rng, j)
        _close(a, *twins)


@pytest.mark.parametrize("case,rng", [("g34_both", "numpy"), ("g55_noop_next_ponly", "philox"), ("g88_disabled_ronly", "philox"), ("g17_both_i32", "numpy")])
def test_summary_and_log_forms_against_the_full_output_run(case, rng):
    autoreset = nc.CASES[case]["kw"]["autoreset"]
    a, b, f = (_mixed(case, rng, "sarsa") for _ in range(3))        # log form, summary form, full output
    sa, sb, lg = a.episode_summary(), b.episode_summary(), _new_log(a)
    want5, pending = lref.new_state5(N), None
    want_log = lref.new_log(N, M_LOG, SENT_RET, SENT_LEN)
    counters = lref.new_counters()
    for launch in range(3):
        assert a.rollout_grid_learn(K, summary=sa, log=lg) is sa
        b.rollout_grid_learn(K, summary=sb)
        obs, rew, term, trunc, act = f.rollout_grid_learn(K)
        rc, pending = eref.reset_calls(_np(term), _np(trunc), autoreset, pending)
        want_log, want5 = lref.run(_np(rew), _np(term), _np(trunc), rc, want5, want_log, counters)
        _assert_same5(sa, want5, (case, rng, launch, "log form"))             # the five values,
        _assert_same5(sb, want5, (case, rng, launch, "summary form"))
        _assert_same_log(lg, want_log, (case, rng, launch))                   # count, ret and len
        if launch == 0:
            sa.pop(); sb.pop()
            want5 = lref.pop5(want5)
    assert counters["ended_terminated"] + counters["ended_truncated"] > 0 and counters["over_M"] + counters["under_M"] > 0
    assert (want_log["ret"] == SENT_RET).any() == (counters["under_M"] > 0)   # unwritten entries kept the sentinel
    for env in (a, b):
        _assert_same_q(env, f, (case, rng))
        _assert_same_handles(env, f, rng, (case, rng))
    _close(a, b, f)


def test_scheduled_forms_against_the_composed_scheduled_restatement():
    import grid_schedule_ref as gsr
    case, rng = nc.SCHED_CASE, "philox"
    c = nc.CASES[case]
    for algo in gref.ALGOS:
        infos, Q, traj = nref.composed(case, algo, sched=nc.ref_schedule())
        a, b, f = (_mixed(case, rng, algo) for _ in range(3))       # log form, summary form, full output
        for env in (a, b, f):
            env.set_grid_learner_schedule(**nc.schedule())
        assert f.grid_learn_kernel_name(K) == nc.expected_name(case, rng, sched=True), f.grid_learn_kernel_name(K)
        assert a.grid_learn_kernel_name(K, summary=True) == nc.expected_name(case, rng, summary=True, sched=True)
        assert a.grid_learn_kernel_name(K, eval=True) == nc.expected_name(case, rng, eval=True)        # evaluation has no SCHED form
        sa, sb, lg = a.episode_summary(), b.episode_summary(), _new_log(a)
        for launch in range(nc.LAUNCHES):
            sl = slice(launch * K, (launch + 1) * K)
            _assert_same_outputs(f.rollout_grid_learn(K), (traj["obs"][sl], traj["reward"][sl], traj["terminated"][sl], traj["truncated"][sl],
                                                            traj["vectors"][sl]), (algo, launch))
            a.rollout_grid_learn(K, summary=sa, log=lg)
            b.rollout_grid_learn(K, summary=sb)
        want_log, want5, counters = gsr.log_of(traj, K, nc.LAUNCHES, M_LOG, fill_ret=SENT_RET, fill_len=SENT_LEN)
        assert counters["over_M"] > 0
        _assert_same5(sa, want5, (algo, "log form")); _assert_same5(sb, want5, (algo, "summary form"))
        _assert_same_log(lg, want_log, algo)
        for env in (a, b, f):
            _assert_same_q(env, gref.as_grid(Q, c["cfg"]["grid_shape"]), algo)
            got_ep = _np(env.grid_learner_episodes())
            assert got_ep.dtype == np.int32 and np.array_equal(got_ep, traj["ep"]), algo
            assert not env.status().any()
        assert traj["ep"].any()
        _close(a, b, f)
    # ... and on numpy streams, against scheduled uniform twins
    idx = nc.pair_index(case)
    a = _mixed(case, "numpy", "sarsa")
    twins = [_uniform(case, pair, "numpy", "sarsa") for pair in c["pairs"]]
    for env in [a] + twins:
        env.set_grid_learner_schedule(**nc.schedule())
    for launch in range(nc.LAUNCHES):
        out = a.rollout_grid_learn(K)
        for j, u in enumerate(twins):
            _assert_same_outputs(out, u.rollout_grid_learn(K), ("numpy", launch, j), idx == j)
    for j, u in enumerate(twins):
        _assert_same_q(a, u, ("numpy", j), idx == j)
        _assert_same_handles(a, u, "numpy", ("numpy", j), idx == j)
        assert np.array_equal(_np(a.grid_learner_episodes())[idx == j], _np(u.grid_learner_episodes())[idx == j])
    _close(a, *twins)


def test_tables_in_lds_equal_tables_in_global_memory():
    case = "g34_both"
    for rng in ("numpy", "philox"):
        a, b = _mk(case, rng), _mk(case, rng)
        b.set_kernel_options("NO_GRID_QLDS")
        for env in (a, b):
            _learner(env, case, "sarsa")
            env.set_grid_noise_levels(**nc.levels(case))
        assert a.grid_learn_kernel_name(K) == nc.expected_name(case, rng, qlds=1)
        assert b.grid_learn_kernel_name(K) == nc.expected_name(case, rng, qlds=0)
        sa, sb, la, lb = a.episode_summary(), b.episode_summary(), _new_log(a), _new_log(b)
        _assert_same_outputs(a.rollout_grid_learn(K), b.rollout_grid_learn(K), (rng, "full"))
        a.rollout_grid_learn(K, summary=sa); b.rollout_grid_learn(K, summary=sb)
        a.rollout_grid_learn(K, summary=sa, log=la); b.rollout_grid_learn(K, summary=sb, log=lb)
        _assert_same_outputs(a.rollout_grid_eval(K), b.rollout_grid_eval(K), (rng, "eval"))
        _assert_same5(sa, _state5(sb), rng)
        _assert_same_log(la, _log3(lb), rng)
        _assert_same_q(a, b, rng)
        _assert_same_handles(a, b, rng, rng)
        _close(a, b)


# ---- 4. lifecycle
def test_cleared_levels_equal_a_handle_that_never_had_them():
    case, algo = "g34_both", "sarsa"
    cfg = nc.CASES[case]["cfg"]
    for rng in ("numpy", "philox"):
        a, b = _mk(case, rng), _mk(case, rng)
        # the creation values before any set
        tn, rn = a.grid_noise_levels()
        assert tn.dtype == rn.dtype == np.float64 and (tn == cfg["transition_noise"]).all() and (rn == cfg["reward_noise"]).all()
        for env in (a, b):
            _learner(env, case, algo)
        # both start from the same state: the same creation-value launch, then levels on a for one launch of its own ...
        _assert_same_outputs(a.rollout_grid_learn(K), b.rollout_grid_learn(K), (rng, "before"))
        a.set_grid_noise_levels(**nc.levels(case))
        a.clear_grid_noise_levels()
        tn, rn = a.grid_noise_levels()
        assert (tn == cfg["transition_noise"]).all() and (rn == cfg["reward_noise"]).all()
        assert a.grid_learn_kernel_name(K) == b.grid_learn_kernel_name(K) == nc.uniform_name(case, (0.2, 0.25), rng)
        for launch in range(2):
            _assert_same_outputs(a.rollout_grid_learn(K), b.rollout_grid_learn(K), (rng, launch))
        _assert_same_q(a, b, rng)
        _assert_same_handles(a, b, rng, rng)
        _close(a, b)


def test_levels_are_configuration_round_trip_one_key_and_replacement():
    case, algo, rng = "g34_both", "sarsa", "philox"
    lv = nc.levels(case)
    a = _mixed(case, rng, algo)
    tn, rn = a.grid_noise_levels()
    assert np.array_equal(tn, lv["transition_noise"]) and np.array_equal(rn, lv["reward_noise"])
    # levels survive set_grid_learner and set_grid_learner(None), the schedule calls and the state accessors
    a.set_grid_learner(None)
    assert np.array_equal(a.grid_noise_levels()[0], lv["transition_noise"])
    _learner(a, case, algo)
    a.set_grid_learner_schedule(epsilon=[0.5, 0.25])
    a.clear_grid_learner_schedule()
    st = a.get_augmented_state()
    a.set_augmented_state(st)
    tn, rn = a.grid_noise_levels()
    assert np.array_equal(tn, lv["transition_noise"]) and np.array_equal(rn, lv["reward_noise"])
    assert a.grid_learn_kernel_name(K) == nc.expected_name(case, rng)
    b = _mixed(case, rng, algo)                                     # ... and the launch is that of a handle that made none of these calls
    _assert_same_outputs(a.rollout_grid_learn(K), b.rollout_grid_learn(K), "after the calls that leave levels alone")
    # one key given: the other stays (a torch tensor, float32: converted to float64)
    sig2 = torch.linspace(0.0, 4.0, N, dtype=torch.float32)
    for env in (a, b):
        q_before = _np(env.get_grid_q())
        env.set_grid_noise_levels(reward_noise=sig2)
        _assert_same_q(_np(env.get_grid_q()), q_before, "replacing levels does not touch Q")
    tn, rn = a.grid_noise_levels()
    assert np.array_equal(tn, lv["transition_noise"]) and np.array_equal(rn, sig2.numpy().astype(np.float64))
    # levels replaced between two launches: the second launch is that of uniform twins continuing at the new values -- here
    # shown against b, and against the CPU by the off-lattice rewards of the envs whose sigma was 0 and no longer is
    out = a.rollout_grid_learn(K)
    _assert_same_outputs(out, b.rollout_grid_learn(K), "after the replacement")
    was_zero = (lv["reward_noise"] == 0.0) & (sig2.numpy() > 0)
    lattice = nref.noiseless_lattice(nc.CASES[case]["cfg"])
    assert was_zero.any() and (~np.isin(_np(out[1])[:, was_zero], lattice)).any()
    still_zero = sig2.numpy() == 0.0
    assert still_zero.any() and np.isin(_np(out[1])[:, still_zero], lattice).all()
    # many distinct transition levels: no limit
    a.set_grid_noise_levels(transition_noise=np.linspace(0.0, 1.0, N))
    assert len(np.unique(a.grid_noise_levels()[0])) == N
    a.rollout_grid_learn(K)
    assert not a.status().any()
    _close(a, b)


def test_replaced_levels_continue_like_uniform_twins_from_the_same_state():
    """the mixed handle runs one launch at the case's levels, then with the pairs shifted by one; the twin of pair j steps the
    first launch's vectors open-loop, takes the Q of the mixed handle and learns on at its pair"""
    case, algo = "g34_both", "q_learning"
    c = nc.CASES[case]
    m = len(c["pairs"])
    for rng in ("numpy", "philox"):
        a = _mixed(case, rng, algo)
        out = a.rollout_grid_learn(K)
        q = a.get_grid_q()
        idx2 = (nc.pair_index(case) + 1) % m
        p, s = (np.array(x) for x in zip(*c["pairs"]))
        a.set_grid_noise_levels(transition_noise=p[idx2], reward_noise=s[idx2])
        _assert_same_q(_np(a.get_grid_q()), _np(q), "the tables stay")
        out2 = a.rollout_grid_learn(K)
        idx1 = nc.pair_index(case)
        for j2, pair in enumerate(c["pairs"]):
            # an env now at pair j2 was at pair j1 before: its twin is created at j1, steps open-loop, then becomes j2 by levels
            # equal everywhere (the uniform handle's NLEV kernel, shown equal to its existing kernel above)
            mine = idx2 == j2
            for j1 in sorted(set(idx1[mine].tolist())):
                both = mine & (idx1 == j1)
                u = _mk(case, rng)
                _learner(u, case, algo)
                u.set_grid_noise_levels(transition_noise=c["pairs"][j1][0], reward_noise=c["pairs"][j1][1])
                u.rollout_grid_learn(K)                             # (its own learning launch: the same as a's on `both`)
                u.set_grid_q(q)
                u.set_grid_noise_levels(transition_noise=pair[0], reward_noise=pair[1])
                _assert_same_outputs(out2, u.rollout_grid_learn(K), (rng, j1, j2), both)
                _assert_same_q(a, u, (rng, j1, j2), both)
                _assert_same_handles(a, u, rng, (rng, j1, j2), both)
                u.close()
        a.close()


# ---- 5. HIP graphs
def test_levelled_launches_replayed_from_a_hip_graph():
    """a Philox g34_both launch, full output and summary, captured and replayed three times at counter offsets 3, 42 and 81
    (evaluation launches move the counter in between: rollout() is refused while levels are set) against an eager twin; before
    the third replay sigma is replaced in place"""
    case, algo, rng = "g34_both", "sarsa", "philox"
    for form in ("full", "summary"):
        a, b = _mixed(case, rng, algo), _mixed(case, rng, algo)
        sa, sb = a.episode_summary(), b.episode_summary()
        bufs = a.alloc_rollout_grid(K)
        run_a = (lambda: a.rollout_grid_learn(K, out=bufs)) if form == "full" else (lambda: a.rollout_grid_learn(K, summary=sa))
        run_b = (lambda: b.rollout_grid_learn(K)) if form == "full" else (lambda: b.rollout_grid_learn(K, summary=sb))
        run_a(); run_b()                                            # the eager launch of the same form before the capture
        call = gru.capture(a, run_a, K)
        for replay, between in enumerate((3, 2, 2)):
            _assert_same_outputs(a.rollout_grid_eval(between), b.rollout_grid_eval(between), (form, "between", replay))
            if replay == 2:                                         # the buffers are overwritten in place: the replay reads the new values
                sig = np.linspace(0.0, 3.0, N)
                for env in (a, b):
                    env.set_grid_noise_levels(reward_noise=sig)
            assert gru.tick(a) - call.tick0 == (3, 42, 81)[replay]
            call.replay()
            want = run_b()
            torch.cuda.synchronize()
            if form == "full":
                _assert_same_outputs(bufs, want, (form, "replay", replay))
            else:
                _assert_same5(sa, _state5(sb), (form, "replay", replay))
        if form == "full":                                          # the new sigma did reach the replay: envs whose sigma was 0 pay noisy rewards
            was_zero = (nc.levels(case)["reward_noise"] == 0.0) & (sig > 0)
            assert (~np.isin(_np(bufs[1])[:, was_zero], nref.noiseless_lattice(nc.CASES[case]["cfg"]))).any()
        _assert_same_q(a, b, form)
        _assert_same_handles(a, b, rng, form)
        _close(a, b)


# ---- 6. refusals that change nothing
_DISCRETE = dict(state_space_type="discrete", action_space_type="discrete", state_space_size=8, action_space_size=8, delay=0,
                 sequence_length=1, seed=0)
_CONTINUOUS = dict(state_space_type="continuous", state_space_dim=4, target_point=[0, 0, 0, 0], target_radius=0.05, state_space_max=10,
                   action_space_max=1, transition_dynamics_order=1, inertia=1, time_unit=0.1, reward_function="move_to_a_point", seed=0)
_GRID = dict(state_space_type="grid", reward_function="move_to_a_point", grid_shape=(4, 4), make_denser=True, target_point=[2, 2], seed=1,
             transition_noise=0.2, reward_noise=0.25)


def test_refusals_change_nothing():
    from mdp_playground_amd import RLToyVectorEnv, _capi as capi
    case, algo, rng = "g34_both", "q_learning", "philox"
    a, b = _mixed(case, rng, algo), _mixed(case, rng, algo)
    lv = nc.levels(case)
    acts = torch.as_tensor(gref.action_vector(np.random.default_rng(0).integers(0, 4, size=(5, N))), device=a.device)
    # step(), rollout(), step_graph() while levels are set -- and the C calls
    for call in (lambda: a.step(acts[0]), lambda: a.rollout(acts), lambda: a.step_graph(acts)):
        with pytest.raises(capi.MdppError, match=ONLY):
            call()
    out = a.alloc_rollout(5)
    rc = a._lib.mdpp_step_n(a._h, 5, C.c_void_p(acts.data_ptr()), *(C.c_void_p(t.data_ptr()) for t in out), a._stream())
    assert rc == ESTATE and b"grid noise levels: learner and evaluation launches only; clear_grid_noise_levels() first" in a._lib.mdpp_last_error(a._h)
    a.reset(); b.reset()                                            # reset() is unaffected
    # bad values through the binding and through the C call: MDPP_EINVAL, the levels in force unchanged
    for bad in (dict(transition_noise=np.full(N, 1.5)), dict(reward_noise=np.full(N, -1.0)), dict(reward_noise=np.full(N, np.nan)),
                dict(transition_noise=np.zeros(N - 1)), dict(reward_noise=np.zeros((N, 1)))):
        with pytest.raises(ValueError):
            a.set_grid_noise_levels(**bad)
    good = np.full(N, 0.5)
    for tn, rn in ((np.full(N, 1.0 + 2.0 ** -52), None), (np.full(N, -1e-9), good), (good, np.full(N, np.inf)), (None, np.full(N, -0.5)),
                   (np.where(np.arange(N) == N - 1, np.nan, 0.5), None), (good, np.where(np.arange(N) == 7, np.nan, 0.5))):
        assert a._lib.mdpp_set_grid_noise_levels(a._h, capi.nptr(tn), capi.nptr(rn), a._stream()) == EINVAL
        assert b"mdpp_set_grid_noise_levels" in a._lib.mdpp_last_error(a._h)
    assert a._lib.mdpp_set_grid_noise_levels(a._h, None, None, a._stream()) == 0                      # both NULL: MDPP_OK, nothing changes
    tn, rn = a.grid_noise_levels()
    assert np.array_equal(tn, lv["transition_noise"]) and np.array_equal(rn, lv["reward_noise"])
    _assert_same_outputs(a.rollout_grid_learn(K), b.rollout_grid_learn(K), "after the refusals")
    _assert_same_q(a, b, "after the refusals")
    # working again after clear
    a.clear_grid_noise_levels(); b.clear_grid_noise_levels()
    _assert_same_outputs(a.rollout(acts), b.rollout(acts), "rollout after clear")
    a.step(acts[0]); b.step(acts[0])
    g = a.step_graph(acts)
    g.replay()
    torch.cuda.synchronize()
    # set_noise_levels on a grid handle: refused as ever
    with pytest.raises((NotImplementedError, capi.MdppError)):
        a.set_noise_levels(reward_noise=0.5)
    assert a._lib.mdpp_set_noise_levels(a._h, None, capi.nptr(good), a._stream()) != 0
    _close(a, b)
    # a key the handle was not created with: ValueError from the binding, MDPP_ESTATE from the library, nothing applied
    for case2, key in (("g88_disabled_ronly", "transition_noise"), ("g55_noop_next_ponly", "reward_noise")):
        e = _mk(case2, rng)
        with pytest.raises(ValueError, match=key):
            e.set_grid_noise_levels(**{key: np.full(N, 0.5)})
        args = (capi.nptr(good), None) if key == "transition_noise" else (None, capi.nptr(good))
        assert e._lib.mdpp_set_grid_noise_levels(e._h, *args, e._stream()) == ESTATE and key.encode() in e._lib.mdpp_last_error(e._h)
        _learner(e, case2, algo)
        assert "NLEV" not in e.grid_learn_kernel_name(K)
        tn, rn = e.grid_noise_levels()
        assert (tn == nc.CASES[case2]["cfg"].get("transition_noise", 0.0)).all() and (rn == nc.CASES[case2]["cfg"].get("reward_noise", 0.0)).all()
        e.close()
    # handles the grid learner does not serve
    for kw in (_DISCRETE, _CONTINUOUS):
        d = RLToyVectorEnv(num_envs=64, **kw)
        for call in (lambda: d.set_grid_noise_levels(reward_noise=0.5), d.grid_noise_levels, d.clear_grid_noise_levels):
            with pytest.raises(NotImplementedError, match="serve grid envs only"):
                call()
        assert d._lib.mdpp_set_grid_noise_levels(d._h, None, capi.nptr(np.full(64, 0.5)), d._stream()) == capi.EUNSUPPORTED
        assert b"grid learners serve grid envs only" in d._lib.mdpp_last_error(d._h)
        d.close()
    # ... G = 4, image observations, episode_stats (created with both keys: the library's refusal is what answers)
    for cfg, kw, why in ((dict(_GRID, irrelevant_features=True), {}, "grid_dims == 2"),
                         (dict(_GRID, image_representations=True, image_width=32, image_height=32), {}, "image observations"),
                         (dict(_GRID), dict(episode_stats=True), "episode_stats")):
        e = RLToyVectorEnv(num_envs=64, **kw, **cfg)
        for lv in (dict(reward_noise=0.5), dict(transition_noise=np.full(64, 0.1))):
            with pytest.raises(NotImplementedError, match=why):
                e.set_grid_noise_levels(**lv)
        e.close()
