"""step_graph() captures in thread-local mode: in torch's default global mode a HIP call from any other thread of the
process (a process group's watchdog querying its events, RCCL's threads) invalidates the capture."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_step_graph_captures_thread_local_and_replays(monkeypatch):
    from mdp_playground_amd import RLToyVectorEnv
    modes = []
    orig = torch.cuda.graph

    class Recording(orig):
        def __init__(self, *a, capture_error_mode="global", **kw):
            modes.append(capture_error_mode)
            super().__init__(*a, capture_error_mode=capture_error_mode, **kw)

    monkeypatch.setattr(torch.cuda, "graph", Recording)
    cfg = dict(state_space_type="discrete", action_space_type="discrete", state_space_size=8, action_space_size=8,
               delay=4, sequence_length=3, seed=0)
    N, K = 256, 16
    a = RLToyVectorEnv(num_envs=N, autoreset="same_step", **cfg)
    b = RLToyVectorEnv(num_envs=N, autoreset="same_step", **cfg)
    acts = torch.as_tensor(np.random.default_rng(1).integers(0, 8, size=(K, N)).astype(np.int32), device=a.device)
    g = a.step_graph(acts)
    assert modes == ["thread_local"]
    for _ in range(2):
        g.replay()
        obs, rew, term, trunc = b.rollout(acts)
        torch.cuda.synchronize()
        assert torch.equal(g.obs, obs) and torch.equal(g.reward, rew)
        assert torch.equal(g.terminated, term) and torch.equal(g.truncated, trunc)
    a.close()
    b.close()
