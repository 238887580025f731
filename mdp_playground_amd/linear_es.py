"""One antithetic evolution strategy per 64 linear policies, kept inside the closed-loop launch (RLToyVectorEnv.rollout_linear
with es=; include/mdpp.h "Linear policy ES").

The 64 envs of group g -- local envs 64g .. 64g+63, one wave of the kernel -- are one population: 32 antithetic pairs
mean +- sigma z around the group's mean.  The candidate of env i is the env handle's own parameter buffer
(env.get_linear_policy()).  A LinearES owns everything else, device tensors that the kernel reads and writes, E = D (D + 1),
G = N / 64 -- under a policy with memory (set_linear_policy(theta, history=2)) every D + 1 below is 2 D + 1, the policy's own
column count:

    mean      float32  [E, G]  the population means, entry-major: entry e = r (D + 1) + c of group g at [e, g]
    sigma     float32  [G]     perturbation scale per group
    gain      float32  [G]     lr / (sigma * 4032) in float32: the step per unit of rank-weighted sum
    gen       int32    [G]     generation index
    acc       float64  [N]     summed return of the candidate's counted episodes
    ret       float64  [N]     running return of the current counted episode
    fitness   float64  [N]     each member's acc at the last generation end
    eps       int32    [N]     -1: waiting for an episode boundary; 0 .. T-1: counting; T: done
    log_mean  float64  [M, G]  mean member score of generation j in row j (M = log_generations)

A member counts T = episodes_per_member whole episodes of its env; when all 64 are done the generation ends for the whole
group at once: members are ranked (average ranks for ties, NaN lowest; r in [-63, 63]), the mean moves by
gain * sum_m r_m s_m z_pair(m) -- with gain = lr / (sigma 4032) that is lr / (64 sigma) times the sum of the ranks scaled to
[-1, 1] --, and the next candidates are drawn around it with the normals of Philox stream (seed, the pair's even env id,
gen + 1, 19).  Nothing of it lives in the env handle: env.reset() does not touch it.
"""
import numpy as np
import torch

from . import _capi as capi

__all__ = ["LinearES"]

GROUP = 64
_RANK_NORM = np.float32(4032)         # 64 * 63: 64 members, ranks scaled by 1 / 63
_FIELDS = (("mean", torch.float32), ("sigma", torch.float32), ("gain", torch.float32), ("gen", torch.int32),
           ("acc", torch.float64), ("ret", torch.float64), ("fitness", torch.float64), ("eps", torch.int32),
           ("log_mean", torch.float64))


def _per_group(value, G, name, positive):
    if np.isscalar(value):
        v = np.full(G, value, np.float32)
    else:
        v = value.detach().cpu().numpy() if torch.is_tensor(value) else np.asarray(value)
        if v.dtype != np.float32 or v.shape != (G,):
            raise ValueError(f"LinearES: {name} must be a scalar or a float32 array of shape ({G},)")
    if not np.isfinite(v).all() or (positive and not (v > 0).all()) or (not positive and not (v >= 0).all()):
        raise ValueError(f"LinearES: {name} must be finite and {'> 0' if positive else '>= 0'}")
    return np.ascontiguousarray(v)


class LinearES:
    def __init__(self, mean_theta, sigma, lr, *, seed, episodes_per_member=1, log_generations=0):
        """mean_theta: the start means, a float32 tensor [G, D, D + 1] -- [G, D, 2 D + 1] for policies with memory -- (its device is the ES's); sigma, lr: scalars or float32
        arrays [G], sigma finite and > 0, lr finite and >= 0."""
        if not (torch.is_tensor(mean_theta) and mean_theta.dtype == torch.float32 and mean_theta.dim() == 3
                and mean_theta.shape[0] >= 1 and mean_theta.shape[2] in (mean_theta.shape[1] + 1, 2 * mean_theta.shape[1] + 1)):
            raise ValueError("LinearES: mean_theta must be a float32 tensor of shape (G, D, D + 1) or (G, D, 2 D + 1)")
        G, D = int(mean_theta.shape[0]), int(mean_theta.shape[1])
        self.groups, self.num_envs, self.D, self.device = G, GROUP * G, D, mean_theta.device
        self.cols = int(mean_theta.shape[2])     # D + 1, or 2 D + 1 for a policy with memory
        for name, v, low in (("episodes_per_member", episodes_per_member, 1), ("log_generations", log_generations, 0)):
            if isinstance(v, bool) or int(v) != v or int(v) < low:
                raise ValueError(f"LinearES: {name} must be an integer >= {low}")
        self.episodes_per_member, self.log_generations = int(episodes_per_member), int(log_generations)
        self.seed = int(seed)
        if not 0 <= self.seed < 2 ** 64:
            raise ValueError("LinearES: seed must be in [0, 2**64)")
        sg = _per_group(sigma, G, "sigma", True)
        rate = _per_group(lr, G, "lr", False)
        with np.errstate(over="ignore"):
            gain = (rate / (sg * _RANK_NORM).astype(np.float32)).astype(np.float32)
        E, N, dev = D * self.cols, self.num_envs, self.device
        self.mean = mean_theta.reshape(G, E).t().contiguous()
        self.sigma = torch.from_numpy(sg).to(dev)
        self.gain = torch.from_numpy(gain).to(dev)
        self.gen = torch.zeros(G, dtype=torch.int32, device=dev)
        self.acc = torch.zeros(N, dtype=torch.float64, device=dev)
        self.ret = torch.zeros(N, dtype=torch.float64, device=dev)
        self.fitness = torch.zeros(N, dtype=torch.float64, device=dev)
        self.eps = torch.zeros(N, dtype=torch.int32, device=dev)
        self.log_mean = torch.zeros((self.log_generations, G), dtype=torch.float64, device=dev)

    def _shape(self, name):
        if name == "mean":
            return (self.D * self.cols, self.groups)
        if name == "log_mean":
            return (self.log_generations, self.groups)
        return (self.groups,) if name in ("sigma", "gain", "gen") else (self.num_envs,)

    def tensors(self):
        """(mean, sigma, gain, gen, acc, ret, fitness, eps, log_mean), the order of struct mdpp_linear_es."""
        return tuple(getattr(self, name) for name, _ in _FIELDS)

    def check(self, num_envs, D, device, what, cols=None):
        """ValueError unless the nine tensors are what a launch on (num_envs, D, device) can keep (cols: the column count of the
        handle's policy, D + 1 by default)."""
        if (self.num_envs, self.D, self.cols) != (num_envs, D, D + 1 if cols is None else cols):
            raise ValueError(f"{what}: es must be a LinearES of {num_envs} envs with D = {D}")
        for name, dtype in _FIELDS:
            t = getattr(self, name)
            if not (torch.is_tensor(t) and t.dtype == dtype and t.device == device and tuple(t.shape) == self._shape(name)
                    and t.is_contiguous()):
                raise ValueError(f"{what}: es.{name} must be a contiguous {dtype} tensor of shape {self._shape(name)} on {device}")

    def c_struct(self):
        """struct mdpp_linear_es over the nine tensors (it holds their addresses: keep this object alive)."""
        s = capi.MdppLinearEs()
        for name, _ in _FIELDS:
            setattr(s, name, getattr(self, name).data_ptr() if getattr(self, name).numel() else None)
        s.seed, s.episodes_per_member, s.log_rows = self.seed, self.episodes_per_member, self.log_generations
        return s

    def mean_theta(self):
        """The means in the layout of one policy per group: float32 [G, D, D + 1]."""
        return self.mean.t().reshape(self.groups, self.D, self.cols).contiguous()

    def curve(self):
        """(log_mean[:rows], valid): the rows any group has written, rows = min(max gen, M), and per group the number of them
        that are its own, int64 [G] = min(gen, M)."""
        valid = torch.clamp(self.gen.to(torch.int64), max=self.log_generations)
        rows = int(valid.max()) if self.groups else 0
        return self.log_mean[:rows], valid

    def state_dict(self):
        """Host copies of the nine arrays and the constants.  load_state_dict() on another LinearES and
        env.linear_es_init(es) continue the search from the START of the generation it was in (the candidates are redrawn
        from mean, sigma and gen; a generation's finished episodes are not carried)."""
        d = {name: getattr(self, name).cpu().numpy().copy() for name, _ in _FIELDS}
        d.update(seed=self.seed, episodes_per_member=self.episodes_per_member)
        return d

    def load_state_dict(self, d):
        for name, dtype in _FIELDS:
            v = np.asarray(d[name])
            t = getattr(self, name)
            if v.shape != tuple(t.shape) or torch.from_numpy(v[:0].copy()).dtype != dtype:
                raise ValueError(f"LinearES.load_state_dict: {name} must be {dtype} of shape {tuple(t.shape)}")
            t.copy_(torch.from_numpy(np.ascontiguousarray(v)))
        self.seed, self.episodes_per_member = int(d["seed"]), int(d["episodes_per_member"])
