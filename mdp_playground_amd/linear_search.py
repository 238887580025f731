"""One (1+1)-ES per env on the linear policy, kept inside the closed-loop launch (RLToyVectorEnv.rollout_linear with search=;
include/mdpp.h "Linear policy search").

The candidate of env i -- the policy it acts with -- is the env handle's own parameter buffer (env.get_linear_policy()).  A
LinearSearch owns everything else, device tensors that the kernel reads and writes, E = D (D + 1) -- under a policy with memory
(set_linear_policy(theta, history=2)) every D + 1 below is 2 D + 1, the policy's own column count:

    best      float32  [E, N]  the incumbent, entry-major: entry e = r (D + 1) + c of env i at [e, i]
    sigma     float32  [N]     step size per env
    score     float64  [N]     the incumbent's score, -inf at the start
    acc       float64  [N]     sum of the returns of the candidate's finished episodes in this trial
    ret       float64  [N]     running return of the candidate's current episode
    eps       int32    [N]     episodes finished in this trial
    trial     int32    [N]     index of the current trial, 0 at the start
    accepted  int32    [N]     accepted trials

Per env, at every step that is not a reset call: ret += (double)reward; at an episode's end acc += ret, ret = 0, eps += 1; at
eps == episodes_per_trial the trial ends: improved = acc >= score (false for NaN); after trial 0 sigma becomes
min(sigma * sigma_up, sigma_max) or sigma * sigma_down; an improved candidate becomes the incumbent; then trial += 1 and the
next candidate is best + sigma * z, z the first E normals of Philox stream (seed, env id, trial, 18).  Trial 0 evaluates the
start policy unperturbed.  Nothing of it lives in the env handle: env.reset() does not touch it (abandon_episode() drops the
running episode's return).
"""
import math

import numpy as np
import torch

from . import _capi as capi

__all__ = ["LinearSearch"]

_FIELDS = (("best", torch.float32), ("sigma", torch.float32), ("score", torch.float64), ("acc", torch.float64),
           ("ret", torch.float64), ("eps", torch.int32), ("trial", torch.int32), ("accepted", torch.int32))


class LinearSearch:
    def __init__(self, theta, sigma, *, seed, episodes_per_trial=1, sigma_up=1.0, sigma_down=1.0, sigma_max=math.inf):
        """theta: the start policies, a float32 tensor [N, D, D + 1] -- [N, D, 2 D + 1] for policies with memory -- (its device is the search's); sigma: a scalar or a float32
        array [N], >= 0 and finite."""
        if not (torch.is_tensor(theta) and theta.dtype == torch.float32 and theta.dim() == 3
                and theta.shape[2] in (theta.shape[1] + 1, 2 * theta.shape[1] + 1)):
            raise ValueError("LinearSearch: theta must be a float32 tensor of shape (N, D, D + 1) or (N, D, 2 D + 1)")
        N, D = int(theta.shape[0]), int(theta.shape[1])
        self.num_envs, self.D, self.device = N, D, theta.device
        self.cols = int(theta.shape[2])          # D + 1, or 2 D + 1 for a policy with memory
        if isinstance(episodes_per_trial, bool) or int(episodes_per_trial) != episodes_per_trial or int(episodes_per_trial) < 1:
            raise ValueError("LinearSearch: episodes_per_trial must be an integer >= 1")
        self.episodes_per_trial = int(episodes_per_trial)
        for name, v, inf_ok in (("sigma_up", sigma_up, False), ("sigma_down", sigma_down, False), ("sigma_max", sigma_max, True)):
            v = float(v)
            if math.isnan(v) or v < 0 or (math.isinf(v) and not inf_ok):
                raise ValueError(f"LinearSearch: {name} must be {'>= 0' if inf_ok else 'finite and >= 0'}")
            setattr(self, name, float(np.float32(v)))
        self.seed = int(seed)
        if not 0 <= self.seed < 2 ** 64:
            raise ValueError("LinearSearch: seed must be in [0, 2**64)")
        if np.isscalar(sigma):
            sg = np.full(N, sigma, np.float32)
        else:
            sg = sigma.detach().cpu().numpy() if torch.is_tensor(sigma) else np.asarray(sigma)
            if sg.dtype != np.float32 or sg.shape != (N,):
                raise ValueError(f"LinearSearch: sigma must be a scalar or a float32 array of shape ({N},)")
        if not (np.isfinite(sg).all() and (sg >= 0).all()):
            raise ValueError("LinearSearch: sigma must be finite and >= 0")
        E = D * self.cols
        dev = self.device
        self.best = theta.reshape(N, E).t().contiguous()
        self.sigma = torch.from_numpy(np.ascontiguousarray(sg)).to(dev)
        self.score = torch.full((N,), -math.inf, dtype=torch.float64, device=dev)
        self.acc = torch.zeros(N, dtype=torch.float64, device=dev)
        self.ret = torch.zeros(N, dtype=torch.float64, device=dev)
        self.eps = torch.zeros(N, dtype=torch.int32, device=dev)
        self.trial = torch.zeros(N, dtype=torch.int32, device=dev)
        self.accepted = torch.zeros(N, dtype=torch.int32, device=dev)

    def _shape(self, name):
        return (self.D * self.cols, self.num_envs) if name == "best" else (self.num_envs,)

    def tensors(self):
        """(best, sigma, score, acc, ret, eps, trial, accepted), the order of struct mdpp_linear_search."""
        return tuple(getattr(self, name) for name, _ in _FIELDS)

    def check(self, num_envs, D, device, what, cols=None):
        """ValueError unless the eight tensors are what a launch on (num_envs, D, device) can keep (cols: the column count of
        the handle's policy, D + 1 by default)."""
        if (self.num_envs, self.D, self.cols) != (num_envs, D, D + 1 if cols is None else cols):
            raise ValueError(f"{what}: search must be a LinearSearch of {num_envs} envs with D = {D}")
        for name, dtype in _FIELDS:
            t = getattr(self, name)
            if not (torch.is_tensor(t) and t.dtype == dtype and t.device == device and tuple(t.shape) == self._shape(name)
                    and t.is_contiguous()):
                raise ValueError(f"{what}: search.{name} must be a contiguous {dtype} tensor of shape {self._shape(name)} on {device}")

    def c_struct(self):
        """struct mdpp_linear_search over the eight tensors (it holds their addresses: keep this object alive)."""
        s = capi.MdppLinearSearch()
        for name, _ in _FIELDS:
            setattr(s, name, getattr(self, name).data_ptr())
        s.seed, s.episodes_per_trial = self.seed, self.episodes_per_trial
        s.sigma_up, s.sigma_down, s.sigma_max = self.sigma_up, self.sigma_down, self.sigma_max
        return s

    def best_theta(self):
        """The incumbents in the layout of set_linear_policy: float32 [N, D, D + 1]."""
        return self.best.t().reshape(self.num_envs, self.D, self.cols).contiguous()

    def abandon_episode(self, mask=None):
        """Drop the running episode's return (after an env.reset() that cut it short): ret = 0 for every env, or where ``mask``
        (bool [N]) is set.  The trial's finished episodes stay."""
        if mask is None:
            self.ret.zero_()
            return
        m = torch.as_tensor(mask, device=self.device)
        if m.dtype != torch.bool or tuple(m.shape) != (self.num_envs,):
            raise ValueError(f"LinearSearch.abandon_episode: mask must be bool of shape ({self.num_envs},)")
        self.ret.masked_fill_(m, 0.0)

    def state_dict(self):
        """Host copies of the eight arrays and the constants; with env.get_linear_policy() (the candidate) and the env's own
        state a search can go on elsewhere, mid-trial too."""
        d = {name: getattr(self, name).cpu().numpy().copy() for name, _ in _FIELDS}
        d.update(seed=self.seed, episodes_per_trial=self.episodes_per_trial, sigma_up=self.sigma_up, sigma_down=self.sigma_down,
                 sigma_max=self.sigma_max)
        return d

    def load_state_dict(self, d):
        for name, dtype in _FIELDS:
            v = np.asarray(d[name])
            t = getattr(self, name)
            if v.shape != tuple(t.shape) or torch.from_numpy(v[:0].copy()).dtype != dtype:
                raise ValueError(f"LinearSearch.load_state_dict: {name} must be {dtype} of shape {tuple(t.shape)}")
            t.copy_(torch.from_numpy(np.ascontiguousarray(v)))
        self.seed, self.episodes_per_trial = int(d["seed"]), int(d["episodes_per_trial"])
        self.sigma_up, self.sigma_down, self.sigma_max = float(d["sigma_up"]), float(d["sigma_down"]), float(d["sigma_max"])
