"""In-kernel learners and evaluation with ONE MDP PER ENV (RLToyVectorEnv(seeds=[...]).set_learner(..., per_env_mdp=True); the
PM forms of k_discrete_learn_rollout / k_discrete_eval_rollout and their summary kernels).

Every launch is held to three yardsticks:
  twin         an identical seeds= handle fed the returned actions through rollout(): outputs (reward by bits), state record,
               env and space streams, status and step counter all equal;
  restatement  tests/learner_sweep_ref.py fed the launch's own outputs with P[i] per env: actions and get_q() bit for bit;
  CPU loop     (Philox streams) tests/per_env_mdp_cpu.py: one oracle env per seed driven by the restatement -- actions, outputs
               and Q bit for bit, and the floors of per_env_mdp_cpu.FLOORS re-asserted on the device's result.
The set-up (per_env_mdp_cpu): N = 320 envs -- one full workgroup and 64 lanes of a second -- on seeds 100 ... 419, whose 320
P tables are pairwise different (tests/test_per_env_mdp_host.py), env_id_offset 1000, K = 37, two launches in a row."""
import ctypes as C

import numpy as np
import pytest
import torch

import eval_summary_ref as eref
import graph_replay_util as gr
import learner_sweep_ref as ref
import per_env_mdp_cpu as pm

pytestmark = pytest.mark.gpu

N, K, OFF, SEED = pm.N, pm.K, pm.OFF, pm.SEED
ALPHA, GAMMA, EPS = pm.ALPHA, pm.GAMMA, pm.EPS
# shapes beyond the five cases: no size a multiple of 4 (P, the terminal flags and the reward bits are bytes packed into dwords
# of the LDS slots), with unit and with valued rewards (a reward is two dwords there)
ODD = {
    "odd_unit": dict(pm._D, state_space_size=5, action_space_size=5, delay=1, sequence_length=2),             # P 25 B, 25 reward bits
    "odd_rdist": dict(pm._D, state_space_size=7, action_space_size=7, delay=2, sequence_length=1, reward_dist=[0.5, 1.0], reward_density=0.5),   # P 49 B, 7 rewards (3 paid)
}


def _mk(cfg, rng, seeds=pm.SEEDS, **kw):
    from mdp_playground_amd import RLToyVectorEnv
    extra = dict(rng="philox", philox_seed=pm.PHILOX_SEED) if rng == "philox" else {}
    return RLToyVectorEnv(seeds=list(seeds), env_id_offset=OFF, **extra, **kw, **cfg)


def _learner(env, algo, **kw):
    env.set_learner(algo, **dict(dict(alpha=ALPHA, gamma=GAMMA, epsilon=EPS, seed=SEED, per_env_mdp=True), **kw))


def _tick(env):
    t = C.c_uint64()
    assert env._lib.mdpp_tick(env._h, 0, C.byref(t)) == 0
    return int(t.value)


def _np(x):
    return x.cpu().numpy().copy()


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def _obs_now(env):
    return _np(env._obs) if env._obs_src is None else _np(env._obs_src)


def _assert_same_outputs(got, want, what):
    for name, g, w in zip(("obs", "reward", "terminated", "truncated"), got, want):
        g, w = _np(g), _np(w)
        if name == "reward":
            g, w = _bits(g), _bits(w)
        assert g.shape == w.shape and np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5])


def _assert_same_handles(a, b, rng):
    from mdp_playground_amd import _capi as capi
    sa, sb = a.get_augmented_state(), b.get_augmented_state()
    assert sa.keys() == sb.keys()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    if rng == "numpy":
        for st in (capi.STREAM_ENV, capi.STREAM_SPACE):
            assert np.array_equal(a.get_rng_streams(st), b.get_rng_streams(st)), st
    assert not a.status().any() and not b.status().any()
    assert _tick(a) == _tick(b)


class Restated:
    """the restatement on one MDP per env, carried from launch to launch beside a handle"""

    def __init__(self, cfg, algo, seeds=pm.SEEDS, alpha=ALPHA, gamma=GAMMA, eps=EPS, autoreset=ref.SAME_STEP, q0=None):
        mdps = pm.build_mdps(cfg, seeds)
        m, n = mdps[0], len(mdps)
        self.algo, self.alpha, self.gamma, self.eps, self.autoreset = algo, alpha, gamma, eps, autoreset
        self.P = pm.PerEnvP(mdps)
        self.Q = np.zeros((n, 2, m.S, m.A) if algo == "double_q" else (n, m.S, m.A), np.float32) if q0 is None else q0.copy()
        self.pending = np.zeros(n, bool)
        self.info = {}

    def launch(self, tick0, obs_before, out):
        obs, rew, term, trunc = (_np(x) for x in out[:4])
        k, n = obs.shape
        w_e, w_a, w_u = (ref.tick_words(SEED, OFF, tick0, k + 1, n, st) for st in (ref.EXPLORE_STREAM, ref.ACTION_STREAM, ref.UPDATE_STREAM))
        act, self.Q, self.pending, info = ref.run(self.algo, self.alpha, self.gamma, self.eps, self.Q, obs_before, obs, rew, term, trunc,
                                                  self.P, self.autoreset, w_e, w_a, w_u, self.pending)
        ref.merge_info(self.info, info)
        return act


def _check_launch(a, r, k, what):
    """one learning launch of handle a against the restatement r; returns its outputs"""
    before, tick0 = _obs_now(a), _tick(a)
    out = a.rollout_learn(k)
    assert out[4].dtype == torch.int32 and tuple(out[4].shape) == (k, a.num_envs)
    want = r.launch(tick0, before, out)
    got = _np(out[4])
    assert np.array_equal(got, want), (what, "actions", np.argwhere(got != want)[:5])
    q = _np(a.get_q())
    assert q.dtype == np.float32 and np.array_equal(_bits(q), _bits(r.Q)), (what, "Q", np.argwhere(_bits(q) != _bits(r.Q))[:5])
    return out


def _align16(x):
    return (x + 15) & ~15


def _placement(case_or_cfg, algo, *options):
    """(QLDS, PM) by the rule of include/mdpp.h: Q and the MDPs in LDS, Q alone, the MDPs alone, neither -- as far as they fit
    into the 160 KiB of a workgroup beside the shared noise cdf and (with a noise key) the 6 KiB of ziggurat tables; the MDPs
    are candidates up to 64 KiB, the Q-tables up to 160 KiB.  A lane's MDP is its carve: P, terminal flags, start cdf, reward
    bits or rewards, each rounded up to 16 bytes"""
    cfg = pm.CASES[case_or_cfg][0] if isinstance(case_or_cfg, str) else case_or_cfg
    S, A, L = cfg["state_space_size"], cfg["action_space_size"], cfg["sequence_length"]
    rew = 8 * S ** L if "reward_dist" in cfg else (S ** L + 7) // 8
    slots = 256 * (_align16(S * A) + _align16(S) + _align16(8 * S) + _align16(rew))
    q = 256 * S * A * 4 * (2 if algo == "double_q" else 1)
    noise = "transition_noise" in cfg
    fixed = (_align16(8 * S * S) + 6144) if noise else 0
    lds = 160 * 1024
    m_ok = slots <= 64 * 1024 and "NO_PM_LDS" not in options
    q_ok = q <= lds and "NO_LEARN_LDS" not in options
    if q_ok and m_ok and fixed + slots + q <= lds:
        return 1, 2
    if q_ok and fixed + q <= lds:
        return 1, 1
    if m_ok and fixed + slots <= lds:
        return 0, 2
    return 0, 1


def _assert_name(name, kernel, rng, cfg, algo, placement, learn=True):
    qlds, pmv = placement
    noise = "transition_noise" in cfg
    head = "%s<PHILOX=%d,NOISE=%d,UNIT=%d,QLDS=%d," % (kernel, rng == "philox", noise, "reward_dist" not in cfg, qlds)
    assert name.startswith(head) and name.endswith(",PM=%d>" % pmv), (name, head, pmv)
    if learn:
        assert ",PE=1" in name and (",DOUBLE=1" in name) == (algo == "double_q"), name
    else:
        assert ",DOUBLE=%d," % (algo == "double_q") in name, name


def _learn_twice(a, b, r, rng, what):
    """two launches in a row against twin and restatement; returns the outputs of both, stacked"""
    outs = []
    for launch in range(pm.LAUNCHES):
        assert _tick(a) == launch * K
        out = _check_launch(a, r, K, what + (launch,))
        _assert_same_outputs(out[:4], b.rollout(out[4]), what + (launch,))
        outs.append([_np(x) for x in out])
    _assert_same_handles(a, b, rng)
    return [np.concatenate([o[j] for o in outs]) for j in range(5)]


def _assert_cpu_loop(cfg, kw, algo, a, stacked, what, **learner):
    """Philox streams: the whole of both launches is what the CPU loop predicts"""
    _, Q, traj = pm.closed_loop(cfg, kw, algo, learner.get("alpha", ALPHA), learner.get("gamma", GAMMA), learner.get("epsilon", EPS))
    obs, rew, term, trunc, act = stacked
    for name, g, w in (("actions", act, traj["actions"]), ("obs", obs, traj["obs"]), ("terminated", term.astype(bool), traj["terminated"]),
                       ("truncated", trunc.astype(bool), traj["truncated"]), ("reward", _bits(rew), _bits(traj["reward"]))):
        assert np.array_equal(g, w), (what, "CPU loop", name, np.argwhere(g != w)[:5])
    q = _np(a.get_q())
    assert np.array_equal(_bits(q), _bits(Q)), (what, "CPU loop", "Q")


@pytest.mark.parametrize("rng", ["numpy", "philox"])
@pytest.mark.parametrize("algo", pm.ALGOS)
@pytest.mark.parametrize("case", list(pm.CASES))
def test_twin_restatement_and_cpu_loop(case, algo, rng):
    cfg, kw = pm.CASES[case]
    a, b = _mk(cfg, rng, **kw), _mk(cfg, rng, **kw)
    assert a.learn_kernel_name(4) == ""                  # (without the opt-in: refused, as tests/test_gpu_learn_rollout.py pins)
    _learner(a, algo)
    _assert_name(a.learn_kernel_name(K), "k_discrete_learn_rollout", rng, cfg, algo, _placement(case, algo))
    r = Restated(cfg, algo)
    assert np.array_equal(_obs_now(a), _obs_now(b))
    what = (case, algo, rng)
    stacked = _learn_twice(a, b, r, rng, what)
    if rng == "philox":
        _assert_cpu_loop(cfg, kw, algo, a, stacked, what)
    # what keeps the pass honest: the floors of the host test (measured on the Philox streams of seed 77), on the device's result
    if rng == "philox":
        counts = pm.check_floors(case, _np(a.get_q()), stacked[2].astype(bool), what)
    else:
        nz = pm.nonzero_envs(_np(a.get_q()))
        counts = (int(nz.sum()), int(nz[:256].sum()), int(nz[256:].sum()), int(stacked[2].astype(bool).any(axis=0).sum()))
        assert nz[:256].any() and nz[256:].any() and stacked[2].any(), counts
    info = r.info
    print(case, algo, rng, "non-zero Q: all, lanes 0-255, lanes 256-319; envs that terminated:", counts,
          {k: v for k, v in info.items() if not isinstance(v, np.ndarray)})
    assert info["explored"] > 0 and info["greedy_ties"] > 0 and info["greedy_strict"] > 0, info
    if algo == "sarsa":
        assert info["carried"] > 0 and info["carried_differs"] > 0, info
    if algo == "double_q":
        assert info["updates_a"] > 0 and info["updates_b"] > 0 and info["cross_differs"] > 0, info
    a.close(); b.close()


PLACEMENTS = [(), ("NO_PM_LDS",), ("NO_LEARN_LDS",), ("NO_PM_LDS", "NO_LEARN_LDS")]


@pytest.mark.parametrize("rng", ["numpy", "philox"])
@pytest.mark.parametrize("options", PLACEMENTS, ids=lambda o: "+".join(o) or "default")
@pytest.mark.parametrize("algo", pm.ALGOS)
@pytest.mark.parametrize("case", ["s8", "s8_noise"])
def test_every_placement_computes_the_same_and_the_name_says_which(case, algo, options, rng):
    cfg, kw = pm.CASES[case]
    a, b = _mk(cfg, rng, **kw), _mk(cfg, rng, **kw)
    a.set_kernel_options(*options)
    _learner(a, algo)
    placement = _placement(case, algo, *options)
    _assert_name(a.learn_kernel_name(K), "k_discrete_learn_rollout", rng, cfg, algo, placement)
    stacked = _learn_twice(a, b, Restated(cfg, algo), rng, (case, algo, options, rng))
    if rng == "philox":
        _assert_cpu_loop(cfg, kw, algo, a, stacked, (case, algo, options))
    # evaluation takes the same placement
    _assert_name(a.eval_kernel_name(K), "k_discrete_eval_rollout", rng, cfg, algo, placement, learn=False)
    a.close(); b.close()


def test_the_worked_placements_by_name():
    """S = A = 8, L = 3, unit rewards (cfg2): Q and the MDPs in LDS; double_q: Q alone; S = A = 20: neither"""
    for case, algo, want in (("cfg2", "q_learning", "QLDS=1,PE=1,PM=2>"), ("s8", "double_q", "QLDS=1,PE=1,DOUBLE=1,PM=1>"),
                             ("s20", "q_learning", "QLDS=0,PE=1,PM=1>"), ("s20", "double_q", "QLDS=0,PE=1,DOUBLE=1,PM=1>")):
        a = _mk(pm.CASES[case][0], "numpy", seeds=pm.SEEDS[:4])
        _learner(a, algo)
        for name in (a.learn_kernel_name(K), a.eval_kernel_name(K)):
            assert "QLDS=%s" % want[5] in name and name.endswith(want[want.index(",PM="):]), (case, algo, name)
        assert a.learn_kernel_name(K).endswith(want), (case, algo, a.learn_kernel_name(K))
        a.close()


@pytest.mark.parametrize("rng", ["numpy", "philox"])
@pytest.mark.parametrize("algo", pm.ALGOS)
@pytest.mark.parametrize("kw", [dict(autoreset="next_step"), dict(autoreset="disabled", max_episode_steps=5)], ids=["next_step", "disabled_max5"])
def test_autoreset_modes_on_cfg2(kw, algo, rng):
    cfg = pm.CASES["cfg2"][0]
    a, b = _mk(cfg, rng, **kw), _mk(cfg, rng, **kw)
    _learner(a, algo)
    r = Restated(cfg, algo, autoreset=kw["autoreset"])
    stacked = _learn_twice(a, b, r, rng, ("cfg2", kw["autoreset"], algo, rng))
    if rng == "philox":
        _assert_cpu_loop(cfg, kw, algo, a, stacked, ("cfg2", kw["autoreset"], algo))
    term, trunc = stacked[2].astype(bool), stacked[3].astype(bool)
    if kw["autoreset"] == "next_step":
        assert term.any() and r.info["updates"] < 2 * K * N          # (reset calls happened: nothing learnt there)
    else:
        assert trunc.any() and (term | trunc)[-1].all()              # (nothing resets: every env is past its fifth step)
    a.close(); b.close()


@pytest.mark.parametrize("rng", ["numpy", "philox"])
@pytest.mark.parametrize("algo", ["q_learning", "double_q"])
@pytest.mark.parametrize("shape", list(ODD))
def test_sizes_that_are_no_multiple_of_4_bytes(shape, algo, rng):
    cfg = ODD[shape]
    a, b = _mk(cfg, rng), _mk(cfg, rng)
    _learner(a, algo)
    assert _placement(cfg, algo) == (1, 2)               # (small enough for the Q-tables and the slots, double_q included)
    _assert_name(a.learn_kernel_name(K), "k_discrete_learn_rollout", rng, cfg, algo, (1, 2))
    stacked = _learn_twice(a, b, Restated(cfg, algo), rng, (shape, algo, rng))
    if rng == "philox":
        _assert_cpu_loop(cfg, {}, algo, a, stacked, (shape, algo))
    assert stacked[2].any() and (stacked[1] != 0).any()
    a.set_kernel_options("NO_PM_LDS")                    # ... and the same handle goes on in global memory
    assert a.learn_kernel_name(K).endswith(",PM=1>")
    a.close(); b.close()


def test_int32_observations():
    cfg = dict(pm.CASES["s8"][0], dtype_o=np.int32)
    a, b = _mk(cfg, "numpy"), _mk(cfg, "numpy")
    assert a._obs.dtype == torch.int32
    _learner(a, "sarsa")
    out = _learn_twice(a, b, Restated(cfg, "sarsa"), "numpy", ("s8 int32",))
    assert out[0].dtype == np.int32
    a.close(); b.close()


@pytest.mark.parametrize("rng", ["numpy", "philox"])
@pytest.mark.parametrize("n", [1, 63, 257])
def test_sizes_with_a_launch_of_one_step(n, rng):
    cfg, seeds = pm.CASES["s8"][0], pm.SEEDS[:n]
    a, b = _mk(cfg, rng, seeds=seeds), _mk(cfg, rng, seeds=seeds)
    _learner(a, "q_learning")
    # (one env: its one MDP is a shared MDP, the flag changes nothing)
    assert (",PM=" in a.learn_kernel_name(1)) == (n > 1), a.learn_kernel_name(1)
    r = Restated(cfg, "q_learning", seeds=seeds)
    for k in (1, K):
        out = _check_launch(a, r, k, (n, rng, k))
        _assert_same_outputs(out[:4], b.rollout(out[4]), (n, rng, k))
    _assert_same_handles(a, b, rng)
    a.close(); b.close()


@pytest.mark.parametrize("rng", ["numpy", "philox"])
def test_a_sarsa_call_sent_out_in_pieces_equals_one_launch(rng):
    cfg = pm.CASES["s8"][0]
    one, many, b = _mk(cfg, rng), _mk(cfg, rng), _mk(cfg, rng)
    many.set_kernel_options("LEARN_SHORT_PIECES")
    for e in (one, many):
        _learner(e, "sarsa")
    r = Restated(cfg, "sarsa")
    for launch in range(pm.LAUNCHES):
        want = one.rollout_learn(K)
        got = _check_launch(many, r, K, (rng, launch))
        for g, w in zip(got, want):
            assert torch.equal(g, w), (rng, launch)
        _assert_same_outputs(got[:4], b.rollout(got[4]), (rng, launch))
    assert torch.equal(one.get_q().view(torch.int32), many.get_q().view(torch.int32))
    assert r.info["carried_differs"] > 0
    _assert_same_handles(one, many, rng)
    _assert_same_handles(many, b, rng)
    one.close(); many.close(); b.close()


@pytest.mark.parametrize("path", ["device", "mdps"])
def test_device_built_and_host_built_tables_both_go_through_the_kernel(path):
    cfg = pm.CASES["cfg2"][0]
    kw = dict(mdps=pm.build_mdps(cfg)) if path == "mdps" else {}
    a, b = _mk(cfg, "philox", **kw), _mk(cfg, "philox", **kw)
    assert a.tables_built_on == b.tables_built_on == ("device" if path == "device" else "host")
    _learner(a, "q_learning")
    stacked = _learn_twice(a, b, Restated(cfg, "q_learning"), "philox", (path,))
    _assert_cpu_loop(cfg, {}, "q_learning", a, stacked, (path,))
    a.close(); b.close()


@pytest.mark.parametrize("algo", pm.ALGOS)
def test_per_env_hyper_parameters(algo):
    cfg = pm.CASES["s8"][0]
    rs = np.random.default_rng(12)
    alpha = rs.uniform(0.05, 1.0, N).astype(np.float32)
    eps = rs.uniform(0.0, 1.0, N).astype(np.float32)
    eps[:4] = (0.0, 1.0, 0.0, 1.0)
    a, b = _mk(cfg, "philox"), _mk(cfg, "philox")
    _learner(a, algo, alpha=alpha, epsilon=eps)
    r = Restated(cfg, algo, alpha=alpha, eps=eps)
    stacked = _learn_twice(a, b, r, "philox", ("per-env parameters", algo))
    _assert_cpu_loop(cfg, {}, algo, a, stacked, ("per-env parameters", algo), alpha=alpha, epsilon=eps)
    assert r.info["explored_env"][0] == 0 and r.info["explored_env"][1] == r.info["selections_env"][1] > 0
    # a uniform rate again, then a per-env gamma: the arrays are refilled on the next launch
    a.set_learner_rates(alpha=0.5, epsilon=0.1)
    r.alpha, r.eps = 0.5, 0.1
    out = _check_launch(a, r, 9, ("uniform again", algo))
    _assert_same_outputs(out[:4], b.rollout(out[4]), ("uniform again", algo))
    gamma = rs.uniform(0.0, 1.0, N).astype(np.float32)
    a.set_learner_rates(gamma=gamma)
    r.gamma = gamma
    out = _check_launch(a, r, 9, ("per-env gamma", algo))
    _assert_same_outputs(out[:4], b.rollout(out[4]), ("per-env gamma", algo))
    a.close(); b.close()


def _assert_summary(summ, st, what):
    for (name, dt), t in zip(eref.FIELDS, summ.tensors()):
        g, w = _np(t), st[name]
        assert g.dtype == dt and g.shape == w.shape, (what, name)
        if dt == np.float64:
            g, w = g.view(np.int64), w.view(np.int64)
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5])


@pytest.mark.parametrize("rng", ["numpy", "philox"])
@pytest.mark.parametrize("algo", pm.ALGOS)
@pytest.mark.parametrize("case,kw", [("s8_noise", {}), ("cfg2", dict(autoreset="next_step")), ("s20", {})], ids=["s8_noise", "cfg2_next_step", "s20"])
def test_evaluation_and_summaries(case, kw, algo, rng):
    """rollout_eval after learning against the greedy restatement, tables and learner untouched; then the summary forms of
    both launches against the five numbers computed from a full-output twin's launch"""
    cfg = pm.CASES[case][0]
    autoreset = kw.get("autoreset", eref.SAME_STEP)
    a, b, s = _mk(cfg, rng, **kw), _mk(cfg, rng, **kw), _mk(cfg, rng, **kw)
    for e in (a, s):
        _learner(e, algo)
    r = Restated(cfg, algo, autoreset=autoreset)
    out = _check_launch(a, r, K, (case, algo, rng, "learn"))
    b.rollout(out[4])
    s.rollout_learn(K)
    # --- evaluation
    _assert_name(a.eval_kernel_name(K), "k_discrete_eval_rollout", rng, cfg, algo, _placement(case, algo), learn=False)
    q_before, before, tick0 = _np(a.get_q()), _obs_now(a), _tick(a)
    out = a.rollout_eval(K)
    want, reset_call, pending, info = eref.eval_run(q_before, before, _np(out[0]), _np(out[2]), _np(out[3]), autoreset, r.pending)
    assert np.array_equal(_np(out[4]), want), (case, algo, rng, "greedy actions", np.argwhere(_np(out[4]) != want)[:5])
    _assert_same_outputs(out[:4], b.rollout(out[4]), (case, algo, rng, "eval"))
    _assert_same_handles(a, b, rng)
    assert np.array_equal(_bits(_np(a.get_q())), _bits(q_before)) and _tick(a) == tick0 + K
    print(case, algo, rng, "evaluation", info)
    assert info["greedy_strict"] + info["greedy_ties"] == K * N - info["reset_calls"], info
    if case != "cfg2":                                   # (cfg2's delayed reward: 37 steps leave most tables at zero)
        assert info["greedy_strict"] > 0, info
    # (the learner's words and hyper-parameters are untouched: the next learning launch is the restatement's)
    r.pending = pending
    out = _check_launch(a, r, K, (case, algo, rng, "learn after eval"))
    _assert_same_outputs(out[:4], b.rollout(out[4]), (case, algo, rng, "learn after eval"))
    # --- summaries: s makes the launches a made with summary=, the five numbers from a's outputs
    summ = s.episode_summary()
    st = eref.new_state5(N)
    e_out = a.rollout_eval(K)                            # (a: eval at tick 3 K, s: the same with summary=)
    # s is one eval and one learn launch behind a: bring it there with the same calls
    s.rollout_eval(K)
    assert s.rollout_learn(K, summary=summ) is summ
    rc, pend_s = eref.reset_calls(_np(out[2]), _np(out[3]), autoreset, pending)
    st = eref.summary(_np(out[1]), _np(out[2]), _np(out[3]), rc, st)
    _assert_summary(summ, st, (case, algo, rng, "learn summary"))
    assert s.rollout_eval(K, summary=summ) is summ
    rc, _ = eref.reset_calls(_np(e_out[2]), _np(e_out[3]), autoreset, pend_s)
    st = eref.summary(_np(e_out[1]), _np(e_out[2]), _np(e_out[3]), rc, st)
    _assert_summary(summ, st, (case, algo, rng, "eval summary"))
    assert st["episodes"].sum() > 0
    b.rollout(e_out[4])
    assert torch.equal(a.get_q().view(torch.int32), s.get_q().view(torch.int32))
    _assert_same_handles(a, b, rng)
    none = torch.zeros(N, dtype=torch.bool, device=s.device)
    assert torch.equal(s.reset(mask=none)[0], e_out[0][K - 1])
    _assert_same_handles(s, b, rng)
    a.close(); b.close(); s.close()


@pytest.mark.parametrize("algo", ["sarsa", "double_q"])
def test_graph_replay(algo):
    """rollout_learn captured in the library's capture mode, replayed three times with the step counter moved by 5 in between,
    against an eager handle"""
    cfg, k = pm.CASES["s8"][0], 9
    g, e = _mk(cfg, "philox"), _mk(cfg, "philox")
    for h in (g, e):
        _learner(h, algo)
    out = g.alloc_rollout_learn(k)
    xs = torch.as_tensor(np.random.default_rng(3).integers(0, 8, (5, N)).astype(np.int32), device=g.device)
    want = e.rollout_learn(k)
    got = g.rollout_learn(k, out=out)                    # the eager launch of the same form before the capture
    assert all(torch.equal(x, y) for x, y in zip(got, want))
    cap = gr.capture(g, lambda: g.rollout_learn(k, out=out), k)
    for replay in range(3):
        g.rollout(xs); e.rollout(xs)                     # the counter moves by 5
        cap.replay()
        want = e.rollout_learn(k)
        for name, x, y in zip(("obs", "reward", "terminated", "truncated", "actions"), out, want):
            assert torch.equal(x.view(torch.uint8) if x.dtype == torch.bool else x, y.view(torch.uint8) if y.dtype == torch.bool else y), (algo, replay, name)
        assert torch.equal(g.get_q().view(torch.int32), e.get_q().view(torch.int32)), (algo, replay)
    g._obs_src = out[0][k - 1]
    _assert_same_handles(g, e, "philox")
    del cap
    g.close(); e.close()


def test_refusals_with_the_flag_on():
    from mdp_playground_amd import RLToyVectorEnv
    a = _mk(pm.CASES["s8"][0], "numpy", seeds=pm.SEEDS[:64])
    _learner(a, "q_learning")
    assert a.learn_kernel_name(4) != ""
    with pytest.raises(NotImplementedError, match="one shared MDP"):
        a.set_policy(np.zeros(8, np.int64), seed=3)
    assert a.policy_kernel_name(4) == ""
    with pytest.raises(NotImplementedError, match="one shared MDP"):
        a.rollout_policy(4)
    a.close()
    a = _mk(dict(pm.CASES["s8"][0], reward_noise=0.5), "numpy", seeds=pm.SEEDS[:64])
    _learner(a, "q_learning")
    with pytest.raises(NotImplementedError, match="per-env noise levels on one MDP per env: not built"):
        a.set_noise_levels(reward_noise=np.full(64, 0.25))
    a.rollout_learn(4)                                   # (the refusals left the learner as it was)
    a.close()
    irr = dict(pm._D, state_space_size=[8, 5], action_space_size=[8, 5], irrelevant_features=True, delay=0, sequence_length=1)
    for c, kw, reason in ((irr, {}, "irrelevant"), (pm.CASES["s8"][0], dict(episode_stats=True), "episode_stats")):
        env = RLToyVectorEnv(seeds=pm.SEEDS[:64], **kw, **c)
        with pytest.raises(NotImplementedError, match=reason):
            _learner(env, "q_learning")
        assert env.learn_kernel_name(4) == ""
        # (the refused call left no opt-in behind: the plain call meets the rule it met before, which comes ahead of episode_stats)
        with pytest.raises(NotImplementedError, match="irrelevant" if reason == "irrelevant" else "one shared MDP"):
            env.set_learner("q_learning", alpha=ALPHA, gamma=GAMMA, epsilon=EPS)
        env.close()


def test_the_opt_in_is_per_handle_and_set_learner_none_clears_it():
    from mdp_playground_amd import RLToyVectorEnv
    cfg = pm.CASES["s8"][0]
    a = _mk(cfg, "numpy", seeds=pm.SEEDS[:64])
    assert a.learn_kernel_name(4) == ""
    with pytest.raises(NotImplementedError, match="one shared MDP"):
        a.set_learner("q_learning", alpha=ALPHA, gamma=GAMMA, epsilon=EPS)
    _learner(a, "q_learning")
    assert a.learn_kernel_name(4) != "" and a.eval_kernel_name(4) != ""
    a.rollout_learn(4)
    a.set_learner(None)                                  # clears the learner and the flag
    assert a.learn_kernel_name(4) == ""
    with pytest.raises(NotImplementedError, match="one shared MDP"):
        a.rollout_learn(4)
    _learner(a, "sarsa")
    a.rollout_learn(4)
    q, name = a.get_q().clone(), a.learn_kernel_name(4)
    with pytest.raises(NotImplementedError, match="one shared MDP"):     # (a plain set_learner is the call without the opt-in ...)
        a.set_learner("q_learning", alpha=ALPHA, gamma=GAMMA, epsilon=EPS)
    assert a.learn_kernel_name(4) == name and torch.equal(a.get_q(), q)   # (... refused without touching the learner in force)
    a.rollout_learn(4)
    a.close()
    shared = RLToyVectorEnv(num_envs=64, seed=0, **cfg)
    with pytest.raises(ValueError, match="per_env_mdp"):
        shared.set_learner("q_learning", alpha=ALPHA, gamma=GAMMA, epsilon=EPS, per_env_mdp=True)
    # the C call on a shared-MDP handle: accepted, nothing changes
    assert shared._lib.mdpp_learner_per_env_mdp(shared._h, 1) == 0
    shared.set_learner("q_learning", alpha=ALPHA, gamma=GAMMA, epsilon=EPS)
    assert shared.learn_kernel_name(4).endswith("QLDS=1>")
    shared.close()
