"""Per-env episode summaries kept by the closed-loop launches (RLToyVectorEnv.rollout_learn / rollout_eval with summary=).

An EpisodeSummary owns five tensors of [N], all zero at creation:

    ret         float64  the running episode's return
    len         int32    the running episode's length
    episodes    int32    the count of finished episodes
    return_sum  float64  the sum of finished episodes' returns
    length_sum  int32    the sum of finished episodes' lengths

The kernel applies, per env and in step order, for every step that is not the reset call of a next-step-autoreset env:
ret += (double)reward; len += 1; terminated or truncated: episodes += 1, return_sum += ret, length_sum += len, ret = len = 0.
Nothing of it lives in the env handle: after an env.reset() call clear().
"""
import torch

__all__ = ["EpisodeSummary"]

_FIELDS = (("ret", torch.float64), ("len", torch.int32), ("episodes", torch.int32), ("return_sum", torch.float64),
           ("length_sum", torch.int32))


class EpisodeSummary:
    def __init__(self, num_envs, device):
        self.num_envs = int(num_envs)
        self.device = torch.device(device)
        for name, dtype in _FIELDS:
            setattr(self, name, torch.zeros(self.num_envs, dtype=dtype, device=self.device))

    def tensors(self):
        """(ret, len, episodes, return_sum, length_sum), the order of the C ABI."""
        return tuple(getattr(self, name) for name, _ in _FIELDS)

    def check(self, num_envs, device, what):
        """ValueError unless the five tensors are what a launch on (num_envs, device) can keep."""
        for name, dtype in _FIELDS:
            t = getattr(self, name)
            if not (torch.is_tensor(t) and t.dtype == dtype and t.device == device and tuple(t.shape) == (num_envs,)
                    and t.is_contiguous()):
                raise ValueError(f"{what}: summary.{name} must be a contiguous {dtype} tensor of shape ({num_envs},) on {device}")

    def pop(self):
        """(episodes, return_sum, length_sum) as clones; those three are zeroed, the running episode carries on."""
        out = (self.episodes.clone(), self.return_sum.clone(), self.length_sum.clone())
        self.episodes.zero_()
        self.return_sum.zero_()
        self.length_sum.zero_()
        return out

    def clear(self):
        """Zero all five: the running episode too (after an env.reset())."""
        for t in self.tensors():
            t.zero_()
