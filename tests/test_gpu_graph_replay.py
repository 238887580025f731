"""Fused (mdpp_step_n, K > 1) and closed-loop launches replayed from HIP graphs (include/mdpp.h, the graph section).

A launch takes the handle's step counter by value; in capture mode it adds a device word written before every replay.  The
kernels derive from the counter the Philox keys, their alignment inside a four-tick Philox block, the blocks a launch spans
and the head of a delay line kept in memory -- so a replayed graph is exact only if every one of them reads the counter
through that word.  The twin rule: handle ``a`` replays a graph of one call, handle ``b`` -- same config, seed and
env_id_offset -- makes the same call eagerly; after each of five replays every output array is equal bit for bit, then both
take a few eager steps (the offsets 0, K + 1, 2 K + 3, 3 K + 6, 4 K + 11 visit every residue mod 4 and move the ring head:
tests/test_graph_replay_host.py), and at the end the state records, every RNG stream, the counters, the Q-tables and the
episode summaries are equal and no status bit is set.  No tolerance anywhere.

Every capture follows one eager launch of the same call on the same handle (tests/graph_replay_util.py)."""
import warnings

import numpy as np
import pytest
import torch

import graph_replay_cases as cases
import graph_replay_util as gr

pytestmark = pytest.mark.gpu


def _mk(case):
    from mdp_playground_amd import RLToyVectorEnv
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = RLToyVectorEnv(num_envs=case["N"], env_id_offset=cases.OFF, **case["kw"], **case["config"])
    if case["opts"]:
        env.set_kernel_options(*case["opts"])
    return env


def _policy(seed, S, A):
    """a stochastic policy with some exactly-zero entries"""
    r = np.random.default_rng(seed)
    p = r.random((S, A))
    p[r.random((S, A)) < 0.3] = 0.0
    p[np.arange(S), r.integers(0, A, S)] += 0.25
    return p / p.sum(axis=1, keepdims=True)


def _thresholds(env, seed):
    from mdp_playground_amd.policy import policy_thresholds
    S, A = env.mdps[0].S, env.mdps[0].A
    return torch.from_numpy(policy_thresholds(_policy(seed, S, A), S, A).view(np.int32)).to(env.device).view(torch.uint32)


def _prepare(env, case):
    """the agent of a closed-loop case, and the per-env noise levels"""
    if case["call"] == "policy":
        env.set_policy(thresholds=_thresholds(env, 1), seed=cases.POLICY_SEED)
    lr = case["learner"]
    if lr is not None:
        alpha, eps = (cases.pe_arrays(env.num_envs, 1) if lr.get("per_env") else (lr["alpha"], lr["epsilon"]))
        q = None
        if lr.get("random_q"):       # (evaluation: tables whose greedy action differs from state to state and env to env)
            g = torch.Generator(device=env.device)
            g.manual_seed(11)
            q = torch.rand(env._learn_q_shape(lr["algo"]), generator=g, device=env.device, dtype=torch.float32)
        env.set_learner(lr["algo"], alpha=alpha, gamma=lr["gamma"], epsilon=eps, seed=lr["seed"], q=q)
    if case["levels"]:
        env.set_noise_levels(*cases.level_arrays(env.num_envs))


def _mutate(env, case, round_):
    """replace what a captured launch reads from the handle's buffers at replay"""
    what = case["mutate"]
    if what == "policy":
        env.set_policy(thresholds=_thresholds(env, 2 + round_), seed=cases.POLICY_SEED)
    elif what == "rates":
        alpha, eps = cases.pe_arrays(env.num_envs, 2 + round_)
        env.set_learner_rates(alpha=alpha, epsilon=eps)
    elif what == "levels":
        tn, rn = cases.level_arrays(env.num_envs, cases.NLEV_TN2, cases.NLEV_RN2)
        env.set_noise_levels(np.roll(tn, 5 * round_), np.roll(rn, round_))      # (rolled by whole cycles: the same five levels)


def _kernel_name(env, case):
    K = case["K"]
    return {"rollout": env.rollout_kernel_name, "policy": env.policy_kernel_name, "learn": env.learn_kernel_name,
            "eval": env.eval_kernel_name, "learn_summary": env.learn_kernel_name, "eval_summary": env.eval_kernel_name}[case["call"]](K)


def _rand_actions(env, T, rng):
    N = env.num_envs
    if env.kind == "discrete" and env._irr:
        m = env.mdps[0]
        return np.stack([rng.integers(0, m.A, size=(T, N)), rng.integers(0, m.A_irr, size=(T, N))], axis=2).astype(np.int32)
    if env.kind == "discrete":
        return rng.integers(0, env.mdps[0].A, size=(T, N)).astype(np.int32)
    if env.kind == "grid":
        G = len(env.mdps[0].grid_shape)
        ac = np.zeros((T, N, G), np.int32)
        np.put_along_axis(ac, rng.integers(0, G, size=(T, N, 1)), rng.integers(-1, 2, size=(T, N, 1)).astype(np.int32), axis=2)
        return ac
    return rng.uniform(-1, 1, size=(T, N, env.mdps[0].D)).astype(np.float32)


class _Side:
    """one handle of a case with the buffers of its call: everything call() touches exists before a capture"""

    def __init__(self, env, case):
        self.env, self.case, self.K = env, case, case["K"]
        c = case["call"]
        self.summary = env.episode_summary() if c.endswith("_summary") else None
        self.acts = None
        if c == "rollout":
            self.out = env.alloc_rollout(self.K)
            self.acts = torch.as_tensor(_rand_actions(env, self.K, np.random.default_rng(0)), device=env.device)
        elif self.summary is None:
            self.out = env._alloc_rollout_closed(self.K)
        else:
            self.out = ()

    def run(self, K=None, out=None):
        """the case's call: K steps into the side's own buffers (the captured call), or an eager one of another length"""
        env, c = self.env, self.case["call"]
        K, out = (self.K, self.out) if K is None else (K, out)
        if c == "rollout":
            return env.rollout(self.acts, out)
        if c == "policy":
            return env.rollout_policy(K, out)
        if c == "learn":
            return env.rollout_learn(K, out)
        if c == "eval":
            return env.rollout_eval(K, out)
        if c == "learn_summary":
            return env.rollout_learn(K, summary=self.summary)
        return env.rollout_eval(K, summary=self.summary)

    def call(self):
        self.run()

    def arrays(self):
        """every array the call writes"""
        return tuple(self.out) + (self.summary.tensors() if self.summary is not None else ())


def _bits(t):
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    if t.dtype == torch.float64:
        return t.view(torch.int64)
    return t.view(torch.uint8) if t.dtype == torch.bool else t


def _assert_equal_arrays(xs, ys, what):
    assert len(xs) == len(ys) and len(xs) > 0, what
    for j, (x, y) in enumerate(zip(xs, ys)):
        x, y = _bits(x), _bits(y)
        assert x.shape == y.shape and x.dtype == y.dtype, (what, j)
        if not torch.equal(x, y):
            bad = (x != y).nonzero()[:5].tolist()
            raise AssertionError((what, "array %d differs" % j, bad))


def _streams_of(env):
    from mdp_playground_amd import _capi as capi
    if env.rng != "numpy":
        return ()
    s = [capi.STREAM_ENV, capi.STREAM_SPACE]
    if env.kind == "grid":
        s.append(capi.STREAM_ACTION)
    if env.kind == "discrete" and env._irr:
        s.append(capi.STREAM_SPACE_IRR)
    if env.kind == "discrete" and getattr(env, "_image", None) is not None:
        s.append(capi.STREAM_IMAGE)
    return tuple(s)


def _assert_same_handles(a, b, case, sa, sb, what):
    st_a, st_b = a.get_augmented_state(), b.get_augmented_state()
    assert st_a.keys() == st_b.keys()
    for k in st_a:
        if isinstance(st_a[k], np.ndarray):
            assert np.array_equal(st_a[k], st_b[k], equal_nan=st_a[k].dtype.kind == "f"), (what, k)
        else:
            assert st_a[k] == st_b[k], (what, k)
    for s in _streams_of(a):
        assert np.array_equal(a.get_rng_streams(s), b.get_rng_streams(s)), (what, "stream", s)
    assert gr.tick(a) == gr.tick(b), what
    if case["learner"] is not None:
        _assert_equal_arrays((a.get_q(),), (b.get_q(),), (what, "Q"))
    if sa.summary is not None:
        _assert_equal_arrays(sa.summary.tensors(), sb.summary.tensors(), (what, "summary"))
    assert not a.status().any() and not b.status().any(), what


def _between(sa, sb, n, rng, what):
    """n eager steps on both handles, compared: step() with random actions (open-loop), the case's own call (closed-loop)"""
    a, b = sa.env, sb.env
    if sa.case["call"] == "rollout":
        acts = torch.as_tensor(_rand_actions(a, n, rng), device=a.device)
        for j in range(n):
            ra, rb = a.step(acts[j]), b.step(acts[j])
            _assert_equal_arrays(ra[:4], rb[:4], (what, "step", j))
    elif sa.summary is not None:
        sa.run(n)
        sb.run(n)
        _assert_equal_arrays(sa.summary.tensors(), sb.summary.tensors(), (what, "eager summary"))
    else:
        _assert_equal_arrays(sa.run(n), sb.run(n), (what, "eager call"))


def _setup(case):
    a, b = _mk(case), _mk(case)
    try:
        for e in (a, b):
            _prepare(e, case)
        for e in (a, b):            # before the capture, so a case cannot drift onto another kernel
            name = _kernel_name(e, case)
            assert name.startswith(case["prefix"]) and all(s in name for s in case["has"]), (name, case["prefix"], case["has"])
        return _Side(a, case), _Side(b, case)
    except BaseException:
        a.close(); b.close()
        raise


def _warm_up_and_capture(sa, sb, what):
    """one eager launch of the call on both handles, then the capture on ``a``"""
    sa.call()
    sb.call()
    torch.cuda.synchronize()
    _assert_equal_arrays(sa.arrays(), sb.arrays(), (what, "warm-up"))
    return gr.capture(sa.env, sa.call, sa.K)


def _run_case(name, case):
    sa, sb = _setup(case)
    try:
        _replays(name, case, sa, sb)
    finally:                    # (also after a failure: a handle must not wait for the garbage collector, graph_replay_util.capture)
        sa.env.close(); sb.env.close()


def _replays(name, case, sa, sb):
    a, b = sa.env, sb.env
    rng = np.random.default_rng(sum(name.encode()))
    graph = _warm_up_and_capture(sa, sb, name)
    offsets = cases.offsets(case)
    ended = 0
    for r in range(cases.REPLAYS):
        assert gr.tick(a) - graph.tick0 == offsets[r] and gr.tick(b) == gr.tick(a), (name, r)
        if sa.acts is not None:      # (the captured launch reads the tensor at replay: new actions every time)
            new = torch.as_tensor(_rand_actions(a, sa.K, rng), device=a.device)
            sa.acts.copy_(new)
            sb.acts.copy_(new)
        graph.replay()
        sb.call()
        torch.cuda.synchronize()
        _assert_equal_arrays(sa.arrays(), sb.arrays(), (name, "replay", r, "offset", offsets[r]))
        if sa.summary is None:
            ended += int(sb.out[2].sum()) + int(sb.out[3].sum())
        if r < len(case["between"]):
            if case["mutate"] and r in (0, 2):
                _mutate(a, case, r)
                _mutate(b, case, r)
            _between(sa, sb, case["between"][r], rng, (name, "after replay", r))
    torch.cuda.synchronize()
    _assert_same_handles(a, b, case, sa, sb, name)
    if sa.summary is not None:
        ended = int(sb.summary.episodes.sum())
    # the in-launch resets (start states keyed by the counter) were exercised -- wherever random actions, a sampled policy or
    # an exploring learner drive a discrete or grid env, and wherever a step limit ends episodes
    if (a.kind != "continuous" and case["call"] not in ("eval", "eval_summary")) or case["kw"].get("max_episode_steps"):
        assert ended > 0, (name, "no episode ended")


@pytest.mark.parametrize("name", sorted(n for n, c in cases.CASES.items() if c["call"] == "rollout"))
def test_fused_rollout_replayed_from_a_graph_equals_the_eager_twin(name):
    _run_case(name, cases.CASES[name])


@pytest.mark.parametrize("name", sorted(n for n, c in cases.CASES.items() if c["call"] in cases.CLOSED_CALLS))
def test_closed_loop_launch_replayed_from_a_graph_equals_the_eager_twin(name):
    _run_case(name, cases.CASES[name])


def test_uniform_learner_rates_travel_by_value_in_a_captured_launch():
    """Uniform alpha, gamma and epsilon (like the seeds, the algorithm and the number of noise levels) are arguments of the
    launch: set_learner_rates(alpha=0.5, epsilon=0.5) on the graph's handle after the capture does not reach the replays,
    which equal a twin that kept the captured rates (include/mdpp.h: per-env arrays are how rates change under a graph).
    An eager launch of the handle does use the new rates."""
    case = cases.BY_VALUE_CASE
    sa, sb = _setup(case)
    try:
        _by_value(case, sa, sb)
    finally:
        sa.env.close(); sb.env.close()


def _by_value(case, sa, sb):
    a, b = sa.env, sb.env
    graph = _warm_up_and_capture(sa, sb, "by_value")
    a.set_learner_rates(alpha=0.5, epsilon=0.5)
    rng = np.random.default_rng(1)
    for r in range(cases.REPLAYS):
        graph.replay()
        sb.call()
        torch.cuda.synchronize()
        _assert_equal_arrays(sa.arrays(), sb.arrays(), ("by_value", "replay", r))
        if r < len(case["between"]):                    # (open-loop steps: no launch that would read a's new rates)
            acts = torch.as_tensor(_rand_actions(a, case["between"][r], rng), device=a.device)
            for j in range(acts.shape[0]):
                _assert_equal_arrays(a.step(acts[j])[:4], b.step(acts[j])[:4], ("by_value", "step", r, j))
    _assert_same_handles(a, b, case, sa, sb, "by_value")
    # the new rates are in force for an eager launch: it departs from the twin's (epsilon 0.5 against 0.25)
    ea, eb = sa.run(case["K"], a._alloc_rollout_closed(case["K"])), sb.run(case["K"], b._alloc_rollout_closed(case["K"]))
    torch.cuda.synchronize()
    assert not torch.equal(ea[4], eb[4])
