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

An EpisodeLog (rollout_learn with summary= and log=) owns three more, all zero at creation, M = max_episodes:

    count       int32    [N]     the episodes this log has seen finish for env i; it goes on counting past M
    ret         float64  [M, N]  entry [m, i]: the return of the m-th episode of env i that finished under this log
    len         int32    [M, N]  ... and its length

Where the rule above finds terminated or truncated, before ret and len are zeroed, the kernel writes row count[i] of env i's
column -- the two values just added to return_sum / length_sum -- while count[i] < M, then count[i] += 1.  The log never reads
``episodes``: EpisodeSummary.pop() does not disturb it, and after an env.reset() its finished episodes stay valid.
"""
import torch

__all__ = ["EpisodeSummary", "EpisodeLog"]

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


class EpisodeLog:
    def __init__(self, num_envs, max_episodes, device):
        self.num_envs = int(num_envs)
        self.max_episodes = int(max_episodes)
        self.device = torch.device(device)
        if self.max_episodes < 1:
            raise ValueError("EpisodeLog: max_episodes must be at least 1")
        if self.max_episodes * self.num_envs > 2 ** 31 - 1:
            raise ValueError("EpisodeLog: max_episodes * num_envs must be at most 2**31 - 1")
        self.count = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
        self.ret = torch.zeros((self.max_episodes, self.num_envs), dtype=torch.float64, device=self.device)
        self.len = torch.zeros((self.max_episodes, self.num_envs), dtype=torch.int32, device=self.device)

    def _fields(self):
        M, N = self.max_episodes, self.num_envs
        return (("count", torch.int32, (N,)), ("ret", torch.float64, (M, N)), ("len", torch.int32, (M, N)))

    def tensors(self):
        """(count, ret, len), the order of the C ABI."""
        return self.count, self.ret, self.len

    def check(self, num_envs, device, what):
        """ValueError unless the three tensors are what a launch on (num_envs, device) can keep."""
        M = self.max_episodes
        if self.num_envs != num_envs or M < 1 or M * num_envs > 2 ** 31 - 1:
            raise ValueError(f"{what}: log must be an EpisodeLog of {num_envs} envs with 1 <= max_episodes * num_envs <= 2**31 - 1")
        for name, dtype, shape in self._fields():
            t = getattr(self, name)
            if not (torch.is_tensor(t) and t.dtype == dtype and t.device == device and tuple(t.shape) == shape
                    and t.is_contiguous()):
                raise ValueError(f"{what}: log.{name} must be a contiguous {dtype} tensor of shape {shape} on {device}")

    def clear(self):
        """Zero all three."""
        for t in self.tensors():
            t.zero_()

    def filled(self):
        """[N]: how many rows of each env's column hold an episode, count.clamp(max=M)."""
        return self.count.clamp(max=self.max_episodes)

    def episodes_of(self, i):
        """(ret, len) of env i's logged episodes in the order they finished, as host numpy arrays (float64, int32)."""
        n = int(self.filled()[i])
        return self.ret[:n, i].cpu().numpy(), self.len[:n, i].cpu().numpy()

    def curve(self, groups=None, num_groups=None):
        """The learning curve by episode index: (n, mean_return, mean_length), each [M] -- row m over the envs with
        count > m --, or [M, G] with ``groups``, an int [N] group id per env (G = num_groups, default max id + 1).  n is
        int64, the means float64 and NaN where n == 0."""
        M = self.max_episodes
        mask = torch.arange(M, device=self.device)[:, None] < self.count[None, :].to(torch.int64)       # [M, N]
        ret = torch.where(mask, self.ret, torch.zeros((), dtype=torch.float64, device=self.device))
        ln = torch.where(mask, self.len.to(torch.float64), torch.zeros((), dtype=torch.float64, device=self.device))
        if groups is None:
            n, rs, ls = mask.sum(1), ret.sum(1), ln.sum(1)
        else:
            g = torch.as_tensor(groups, device=self.device).to(torch.int64)
            if tuple(g.shape) != (self.num_envs,):
                raise ValueError(f"EpisodeLog.curve: groups must have shape ({self.num_envs},)")
            G = int(num_groups) if num_groups is not None else (int(g.max()) + 1 if g.numel() else 0)
            if g.numel() and (int(g.min()) < 0 or int(g.max()) >= G):
                raise ValueError(f"EpisodeLog.curve: group ids must lie in [0, {G})")
            idx = g[None, :].expand(M, -1)
            n = torch.zeros((M, G), dtype=torch.int64, device=self.device).scatter_add_(1, idx, mask.to(torch.int64))
            rs = torch.zeros((M, G), dtype=torch.float64, device=self.device).scatter_add_(1, idx, ret)
            ls = torch.zeros((M, G), dtype=torch.float64, device=self.device).scatter_add_(1, idx, ln)
        nf = n.to(torch.float64)
        return n, rs / nf, ls / nf
