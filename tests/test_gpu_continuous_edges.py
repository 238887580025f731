"""Continuous kernels at the edges of float32 (tests/continuous_edge_cases.py: walls, the radius, cube faces, -0.0, subnormal,
NaN and inf actions, unbounded boxes): every case under the default dispatch -- k_continuous_rollout_fast in its forms,
k_continuous_step1, k_continuous_line_rollout -- and on the general kernel (NO_CFAST), EVERY env against an oracle instance of
its own, after each of three launches (64 fused steps, one step(), 31 fused steps).

Asserted after every launch: observations bit-equal; rewards equal to float32(oracle reward); terminated / truncated; the
terminal observations of the single step; the BAD_ACTION status bit; the state derivatives; on numpy streams the end states of
both generators.  A NaN is matched as a NaN: the sign and payload of a NaN that arithmetic produces (inf - inf, 0 * inf) are not
IEEE's to define and differ between the host (x86: the negative "indefinite") and gfx950 (positive).  The line reward is held
to the upstream tolerance (LINE_ATOL of tests/test_gpu_parity.py, times reward_scale) against the oracle and to 1e-6 between
the two kernels; its states and flags are bit-equal like all others.
"""
import functools

import numpy as np
import pytest
import torch

import continuous_edge_cases as cec
from test_continuous_edges_host import oracle_trajectories, shared_mdp_streams

pytestmark = pytest.mark.gpu

LINE_ATOL = 1e-5          # tests/test_gpu_parity.py: the reference's own tolerance for its SVD-based reward
PHILOX_SEED = 23
RUNS = [(name,) + v for name in cec.CASES for v in cec.variants(name)]


def _venv(**kw):
    from mdp_playground_amd import RLToyVectorEnv
    return RLToyVectorEnv(**kw)


@functools.lru_cache(maxsize=4)
def _expected(name, autoreset, rng, N):
    """The oracle's trajectories of all N envs, stacked time-major (shared by the dispatches; read-only)."""
    acts, trajs = oracle_trajectories(name, autoreset, rng, N, PHILOX_SEED)
    e = {k: np.stack([tr[k] for tr in trajs], axis=1) for k in ("obs", "final", "reward", "term", "trunc", "reset_call", "bad")}
    e["init"] = np.stack([tr["init"] for tr in trajs])
    e["derivs"] = [np.stack([tr["derivs"][k] for tr in trajs]) for k in range(len(cec.LAUNCHES))]
    e["streams"] = [[np.stack([tr["streams"][k][s] for tr in trajs]) for s in (0, 1)] for k in range(len(cec.LAUNCHES))]
    return acts, e


def _same_floats(got, exp):
    """Bit-equal, a NaN matching any NaN."""
    got, exp = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(exp, np.float32)
    return (got.view(np.uint32) == exp.view(np.uint32)) | (np.isnan(got) & np.isnan(exp))


def _first_bad(ok):
    return tuple(int(x) for x in np.argwhere(~ok)[0]) if not ok.all() else None


def _run(env, acts, autoreset):
    """The three launches; per launch obs, reward, terminated, truncated, final_obs (the single step), status, derivatives, streams."""
    out, t0 = [], 0
    numpy_streams = env.rng == "numpy"
    for K in cec.LAUNCHES:
        a = torch.as_tensor(acts[t0:t0 + K], device=env.device)
        fin = None
        if K == 1:
            o, r, te, tr, info = env.step(a[0])
            o, r, te, tr = (x.cpu().numpy()[None].copy() for x in (o, r, te, tr))
            if autoreset == "same_step":
                fin = info["final_obs"].cpu().numpy().copy()
        else:
            o, r, te, tr = (x.cpu().numpy() for x in env.rollout(a))
        out.append(dict(obs=o, reward=r, term=te.astype(bool), trunc=tr.astype(bool), final=fin, status=env.status(),
                        derivs=env.get_augmented_state()["state_derivatives"],
                        streams=[env.get_rng_streams(s) for s in (0, 1)] if numpy_streams else None))
        t0 += K
    return out


@pytest.mark.parametrize("dispatch", ["default", "general"])
@pytest.mark.parametrize("name,autoreset,rng,N", RUNS)
def test_continuous_kernels_at_the_edges_vs_oracle_every_env(name, autoreset, rng, N, dispatch):
    from mdp_playground_amd import _capi as capi
    c = cec.CASES[name]
    cfg = c["config"]
    kw = dict(rng="philox", philox_seed=PHILOX_SEED) if rng == "philox" else {}
    env = _venv(num_envs=N, autoreset=autoreset, max_episode_steps=c["max_episode_steps"], **kw, **cfg)
    twin = None
    try:
        # ---- the kernels this run is about
        if dispatch == "general":
            env.set_kernel_options("NO_CFAST")
            want_roll = want_step = ("k_continuous_step<",)
        else:
            want_roll, want_step = cec.expected_names(name, rng, N)
        for K in (64, 31, 1):
            got_name = env.rollout_kernel_name(K)
            for piece in (want_step if K == 1 else want_roll):
                assert got_name.startswith(piece) if piece.startswith("k_") else piece in got_name, (name, K, got_name, piece)
        acts, exp = _expected(name, autoreset, rng, N)
        if rng == "numpy":
            ew, sw = shared_mdp_streams(name, N)
            assert np.array_equal(env.seeded_streams[0], ew) and np.array_equal(env.seeded_streams[1], sw)
        assert _same_floats(env._obs.cpu().numpy(), exp["init"]).all()
        got = _run(env, acts, autoreset)
        scale = float(cfg.get("reward_scale", 1.0))
        t0 = 0
        for k, K in enumerate(cec.LAUNCHES):
            g, sl = got[k], slice(t0, t0 + K)
            where = (name, autoreset, rng, N, dispatch, "launch", k)
            ok = _same_floats(g["obs"], exp["obs"][sl])
            assert ok.all(), where + ("obs [t, env, d]", _first_bad(ok))
            if c["line"]:
                diff = np.abs(g["reward"].astype(np.float64) - exp["reward"][sl].astype(np.float64))
                print(name, dispatch, "launch", k, "line reward: max |kernel - oracle| =", float(diff.max()), "of", LINE_ATOL * scale)
                ok = diff <= LINE_ATOL * scale
            else:
                ok = _same_floats(g["reward"], exp["reward"][sl])
            assert ok.all(), where + ("reward [t, env]", _first_bad(ok))
            assert np.array_equal(g["term"], exp["term"][sl]) and np.array_equal(g["trunc"], exp["trunc"][sl]), where
            if g["final"] is not None:
                ended = exp["term"][t0] | exp["trunc"][t0]
                assert _same_floats(g["final"][ended], exp["final"][t0][ended]).all(), where + ("final_obs",)
            bad = (exp["bad"][sl] & ~exp["reset_call"][sl]).any(axis=0)
            assert np.array_equal((g["status"] & capi.STATUS_BAD_ACTION) != 0, bad), where + ("BAD_ACTION",)
            assert not (g["status"] & ~np.uint32(capi.STATUS_BAD_ACTION)).any(), where + ("status", g["status"].max())
            ok = _same_floats(g["derivs"], exp["derivs"][k])
            assert ok.all(), where + ("state_derivatives [env, order, d]", _first_bad(ok))
            if g["streams"] is not None:
                for s in (0, 1):
                    assert np.array_equal(g["streams"][s][:, :4], exp["streams"][k][s][:, :4]), where + ("stream", s)
            t0 += K
        if c["line"] and dispatch == "default":
            # the line kernel against the general kernel on the same script: states and flags bit-equal, rewards within 1e-6
            twin = _venv(num_envs=N, autoreset=autoreset, max_episode_steps=c["max_episode_steps"], **kw, **cfg)
            twin.set_kernel_options("NO_CFAST")
            other = _run(twin, acts, autoreset)
            for k in range(len(cec.LAUNCHES)):
                assert _same_floats(got[k]["obs"], other[k]["obs"]).all() and np.array_equal(got[k]["trunc"], other[k]["trunc"])
                d = float(np.abs(got[k]["reward"].astype(np.float64) - other[k]["reward"].astype(np.float64)).max())
                print(name, "launch", k, "line reward: max |line kernel - general kernel| =", d, "of 1e-6")
                assert d <= 1e-6, (name, k, d)
    finally:
        env.close()
        if twin is not None:
            twin.close()
