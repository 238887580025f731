"""The summary form of rollout_linear: rollout_linear(K, summary=) on one handle against the full-output launch on a twin.
The five tensors equal the restated rule (tests/linear_policy_ref.py: float64, from the twin's own outputs) bit for bit, the
state record, streams and step counter equal the twin's, two launches accumulate, pop() and clear() work, and reset(mask=)
after a summary launch shows the twin's last observation for the envs it leaves alone (the continuous mdpp_current_obs)."""
import numpy as np
import pytest
import torch

import linear_policy_cases as lc
import linear_policy_ref as ref
from test_gpu_linear_rollout import _mk, _name_ok, _same, _same_handles, _start

pytestmark = pytest.mark.gpu

SUMMARY_CASES = ("c_d2_n0", "c_d2_n0_no_lds", "d3_order2_rel20_box", "d4_delay3_every2_alw", "cfg3", "cfg5", "d2_default_target_f64",
                 "autoreset_same_step", "autoreset_next_step", "max5_autoreset_disabled")


def _same_summary(summary, want, what):
    for t, k in zip(summary.tensors(), ("ret", "len", "episodes", "return_sum", "length_sum")):
        _same(t, want[k], (what, k))


@pytest.mark.parametrize("rng", lc.RNGS)
@pytest.mark.parametrize("name", SUMMARY_CASES)
def test_summary_against_full_output_twin_and_restated_rule(name, rng):
    c = lc.CASES[name]
    a, b = _mk(c["config"], c["kw"], rng, opts=c["opts"]), _mk(c["config"], c["kw"], rng, opts=c["opts"])
    try:
        theta = lc.theta_of(name)
        _start(a, b, name)
        a.set_linear_policy(theta)
        b.set_linear_policy(theta)
        kname = _name_ok(a, lc.K, c["plds"], summary=True)
        assert kname.split("<")[1] == _name_ok(b, lc.K, c["plds"]).split("<")[1]        # the same form as the full-output kernel
        s = a.episode_summary()
        want, pend = ref.new_summary(lc.N), None
        next_step = c["kw"].get("autoreset") == "next_step"
        ended = 0
        for launch in range(lc.LAUNCHES):
            assert a.rollout_linear(lc.K, summary=s) is s
            _, rew, term, trunc, _ = b.rollout_linear(lc.K)
            r, te, tr = rew.cpu().numpy(), term.cpu().numpy(), trunc.cpu().numpy()
            want, pend = ref.summarise(want, r, te, tr, next_step=next_step, pending=pend)
            _same_summary(s, want, (name, rng, launch))
            _same_handles(a, b, (name, rng, launch))
            ended += int((te | tr).sum())
        assert int(want["episodes"].sum()) == ended > 0                    # episodes ended, and the second launch added to the first
        if name != "max5_autoreset_disabled":                              # (there every step from the fifth on ends an "episode")
            assert (want["len"] > 0).any()                                 # ... and some are running
        # pop(): the finished episodes' three, zeroed; the running episode carries on
        ep, rs, ls = s.pop()
        _same(ep, want["episodes"], "pop episodes"); _same(rs, want["return_sum"], "pop return_sum"); _same(ls, want["length_sum"], "pop length_sum")
        assert not s.episodes.any() and not s.return_sum.any() and not s.length_sum.any()
        _same(s.ret, want["ret"], "ret after pop"); _same(s.len, want["len"], "len after pop")
        s.clear()
        assert all(not t.any() for t in s.tensors())
    finally:
        a.close(); b.close()


def test_wrong_summary_is_a_value_error():
    c = lc.CASES["c_d2_n0"]
    a, other = _mk(c["config"], c["kw"], n=64), _mk(c["config"], c["kw"], n=32)
    try:
        a.reset()
        a.set_linear_policy(lc.theta_of("c_d2_n0")[:64])
        with pytest.raises(ValueError):
            a.rollout_linear(3, summary=other.episode_summary())           # [32] tensors on a handle of 64 envs
        with pytest.raises(ValueError):
            a.rollout_linear(3, summary=torch.zeros(64))
        with pytest.raises(ValueError):
            a.rollout_linear(3, out=a.alloc_rollout_linear(3), summary=a.episode_summary())
        s = a.episode_summary()
        s.len = s.len.to(torch.int64)
        with pytest.raises(ValueError):
            a.rollout_linear(3, summary=s)
    finally:
        a.close(); other.close()


@pytest.mark.parametrize("name", ("c_d2_n0", "cfg3"))
def test_masked_reset_after_a_summary_launch_shows_the_current_observation(name):
    c = lc.CASES[name]
    a, b = _mk(c["config"], c["kw"]), _mk(c["config"], c["kw"])
    try:
        theta = lc.theta_of(name)
        _start(a, b, name)
        a.set_linear_policy(theta)
        b.set_linear_policy(theta)
        a.rollout_linear(lc.K, summary=a.episode_summary())
        last = b.rollout_linear(lc.K)[0][lc.K - 1].clone()
        mask = torch.zeros(lc.N, dtype=torch.bool)
        mask[::3] = True
        oa, _ = a.reset(mask=mask)
        ob, _ = b.reset(mask=mask)
        _same(oa, ob, "masked reset")
        keep = ~mask.numpy()
        _same(oa.cpu().numpy()[keep], last.cpu().numpy()[keep], "the envs left alone show the twin's obs[K - 1]")
        assert not np.array_equal(oa.cpu().numpy()[~keep], last.cpu().numpy()[~keep])
        _same_handles(a, b, "masked reset")
    finally:
        a.close(); b.close()
