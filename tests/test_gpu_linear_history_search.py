"""The two in-kernel searches on a linear policy WITH MEMORY (set_linear_policy(theta, history=2), then rollout_linear(K, search=)
or rollout_linear(K, es=); include/mdpp.h "Linear policies with memory").

linear_search and linear_es on the D = 3 order-2 case (E = 21, PLDS = 1) and linear_es on the D = 12 order-2 case (E = 300,
PLDS = 0), N = 320, two launches, held after EVERY launch, bit for bit, to:
  the twin         rollout(actions) on an identically built handle gives the same outputs and leaves the same handle;
  the restatement  every action, the search's / the ES's arrays, get_linear_policy() (the candidates) and get_linear_memory()
                   equal tests/linear_history_search_ref.py -- the trial end and the generation end over E entries, the act
                   and the memory rule of tests/linear_history_ref.py -- run on the launch's own outputs;
  the form         the kernel's name, HIST=2 and its PLDS value;
and state_dict() -> load_state_dict() on a second handle, with the memory carried over by get_linear_memory(), goes on as the
first does.  No tolerance anywhere."""
import numpy as np
import pytest

import linear_es_ref as ler
import linear_history_cases as hc
import linear_history_ref as href
import linear_history_search_ref as hsr
import linear_search_ref as lsr
from test_gpu_linear_history import _name_ok, _start
from test_gpu_linear_rollout import _mk, _same, _same_handles

pytestmark = pytest.mark.gpu
F32 = np.float32
SEED = 4321


def _pair(name, rng, k=2):
    c = hc.CASES[name]
    return tuple(_mk(c["config"], c["kw"], rng, opts=c["opts"]) for _ in range(k))


def _outputs(a, b, K, what, **agent):
    obs, rew, term, trunc, act = a.rollout_linear(K, **agent)
    tw = b.rollout(act)
    for j, (x, y) in enumerate(zip((obs, rew, term, trunc), tw)):
        _same(x, y, (what, "twin output", j))
    return act, obs.cpu().numpy(), tw[1].cpu().numpy(), tw[2].cpu().numpy(), tw[3].cpu().numpy()


def _same_agent(env, agent, arrays, want, carry, what):
    for k in arrays:
        _same(getattr(agent, k), want[k], (what, k))
    _same(env.get_linear_policy(), want["cand"], (what, "candidates"))
    _same(env.get_linear_memory(), carry["mem"], (what, "memory"))


@pytest.mark.parametrize("rng", hc.RNGS)
def test_search_on_d3_order2_against_twin_and_restatement(rng):
    name = "d3_order2_rel20_box"
    a, b, c = _pair(name, rng, 3)
    try:
        theta = hc.theta_of(name)
        sigma = np.where(np.arange(hc.N) % 3 == 0, 0.0, 0.15).astype(F32)
        rule = dict(seed=SEED, env0=hc.OFF, T=1, up=1.5, down=0.75, sigma_max=0.6, amax=a.mdps[0].action_space_max)
        obs0 = _start(a, b, name)
        c.reset()
        a.set_linear_policy(theta, history=2)
        kname = _name_ok(a, hc.K, 1, kernel="k_continuous_search_rollout", search=True)
        assert kname.split("<")[1] == a.linear_kernel_name(hc.K).split("<")[1]
        search = a.linear_search(sigma, seed=SEED, episodes_per_trial=1, sigma_up=1.5, sigma_down=0.75, sigma_max=0.6)
        assert search.cols == 7 and tuple(search.best.shape) == (21, hc.N)
        state, carry = hsr.search_new_state(theta, sigma), href.new_carry(obs0)
        _same_agent(a, search, lsr.ARRAYS, state, carry, (rng, "start"))
        ended = []
        for launch in range(hc.LAUNCHES):
            act, o, rew, te, tr = _outputs(a, b, hc.K, (rng, launch), search=search)
            want, state, carry, e = hsr.search_launch(state, carry, obs0, o, rew, te, tr, **rule)
            _same(act, want, (rng, launch, "actions against the restatement"))
            _same_agent(a, search, lsr.ARRAYS, state, carry, (rng, launch))
            _same_handles(a, b, (rng, launch))
            ended.append(e)
            obs0 = o[-1]
            if launch == 0:
                # the search goes on elsewhere: c took the same steps; it gets the candidates, the memory and the state_dict
                c.rollout(act)
                c.set_linear_policy(a.get_linear_policy(), history=2)
                mem = a.get_linear_memory()
                differs = (c.get_linear_memory() != mem).any(dim=1)
                assert differs.float().mean() > 0.5            # (a policy just set remembers the state: the memory must be carried)
                c.set_linear_memory(mem)
                search2 = c.linear_search(0.5, seed=0)
                search2.load_state_dict(search.state_dict())
            else:
                out2 = c.rollout_linear(hc.K, search=search2)
                _same(out2[4], act, (rng, "resumed: actions"))
                _same(out2[0], o, (rng, "resumed: observations"))
                for k, x, y in zip(lsr.ARRAYS, search.tensors(), search2.tensors()):
                    _same(x, y, (rng, "resumed", k))
                assert (search2.seed, search2.sigma_up, search2.sigma_down, search2.sigma_max) == (SEED, 1.5, 0.75, float(F32(0.6)))
                _same(c.get_linear_policy(), a.get_linear_policy(), (rng, "resumed: candidates"))
                _same(c.get_linear_memory(), a.get_linear_memory(), (rng, "resumed: memory"))
                _same_handles(a, c, (rng, "resumed"))
        ended = np.concatenate(ended)
        print(rng, kname, "trials ended", int(ended.sum()), "accepted", int(state["accepted"].sum()))
        assert ended.sum() > hc.N and (state["accepted"] > 1).any() and (ended.sum(axis=0) == 0).sum() < hc.N // 4
        assert not np.array_equal(state["cand"][:, :, 3:6], theta[:, :, 3:6])                 # V is searched too
        assert np.array_equal(state["cand"][::3], theta[::3])                                # sigma 0: the start policy stays
        _same(search.best_theta(), np.ascontiguousarray(state["best"].T).reshape(theta.shape), "best_theta")
    finally:
        for e in (a, b, c):
            e.close()


def _es_case(name, rng, plds, E):
    c = hc.CASES[name]
    a, b = _pair(name, rng)
    try:
        D = c["D"]
        G = hc.N // 64
        theta = hc.theta_of(name)
        mean = np.ascontiguousarray(theta[::64][:G])
        sg, lr, T = F32(0.1), F32(0.5), 1
        rule = dict(seed=SEED, env0=hc.OFF, T=T, amax=a.mdps[0].action_space_max, mode=hc.mode_of(name))
        obs0 = _start(a, b, name)
        a.set_linear_policy(theta, history=2)
        kname = _name_ok(a, hc.K, plds, kernel="k_continuous_es_rollout", es=True)
        assert kname.split("<")[1] == a.linear_kernel_name(hc.K).split("<")[1]
        es = a.linear_es(mean, float(sg), float(lr), seed=SEED, episodes_per_member=T, log_generations=4)
        assert es.cols == 2 * D + 1 and tuple(es.mean.shape) == (E, G)
        state = hsr.es_init(hsr.es_new_state(mean, sg, lr, 4), seed=SEED, env0=hc.OFF)
        carry = href.new_carry(obs0)
        _same_agent(a, es, ler.ARRAYS, state, carry, (name, rng, "start"))
        ended = []
        for launch in range(hc.LAUNCHES):
            act, o, rew, te, tr = _outputs(a, b, hc.K, (name, rng, launch), es=es)
            want, state, carry, e = hsr.es_launch(state, carry, obs0, o, rew, te, tr, **rule)
            _same(act, want, (name, rng, launch, "actions against the restatement"))
            _same_agent(a, es, ler.ARRAYS, state, carry, (name, rng, launch))
            _same_handles(a, b, (name, rng, launch))
            ended.append(e)
            obs0 = o[-1]
        ended = np.concatenate(ended)
        print(name, rng, kname, "generations", state["gen"].tolist())
        assert (state["gen"] >= 1).all() and ended[:hc.K].any() and ended[hc.K:].any(), state["gen"]      # generation ends in both launches
        assert not np.array_equal(state["mean"], np.ascontiguousarray(mean.reshape(G, -1).T))
        moved = state["mean"].reshape(D, 2 * D + 1, G)[:, D:2 * D] != mean.transpose(1, 2, 0)[:, D:2 * D]
        assert moved.any(), "the means of V moved"
        _same(es.mean_theta(), np.ascontiguousarray(state["mean"].T).reshape(mean.shape), "mean_theta")
        # state_dict -> load_state_dict -> linear_es_init: the candidates of the generation it was in, over E entries
        es2 = a.linear_es(mean, 0.3, 0.1, seed=1, log_generations=4)
        es2.load_state_dict(es.state_dict())
        a.linear_es_init(es2)
        again = hsr.es_init({k: v.copy() for k, v in state.items()}, seed=SEED, env0=hc.OFF)
        _same(a.get_linear_policy(), again["cand"], (name, rng, "candidates after load_state_dict and init"))
        _same(es2.mean, state["mean"], (name, rng, "mean after load_state_dict"))
        _same(a.get_linear_memory(), carry["mem"], (name, rng, "init leaves the memory alone"))
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("rng", hc.RNGS)
def test_es_on_d3_order2_against_twin_and_restatement(rng):
    _es_case("d3_order2_rel20_box", rng, 1, 21)


@pytest.mark.parametrize("rng", hc.RNGS)
def test_es_on_d12_order2_against_twin_and_restatement(rng):
    _es_case("d12_order2_noise", rng, 0, 300)
