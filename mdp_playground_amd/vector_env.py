"""RLToyVectorEnv — the reference's RLToyEnv (mdp_playground/envs/rl_toy_env.py:26) batched on
one MI355X: same config dict, Gym-style reset/step, torch tensors in and out.

Each env instance i of the batch behaves exactly like one reference object:

* ``RLToyVectorEnv(num_envs=N, **config)`` — one MDP (tables generated on the host from
  ``config["seed"]`` exactly as ``RLToyEnv.__init__`` does) shared by N instances.  Instance i is
  the reference env built from ``config`` and then ``reset(seed=seed_dict["env"] + i)`` (what a
  gymnasium SyncVectorEnv does); its space generator (discrete P-noise, continuous reset
  sampling) is the reference's own for i = 0 and ``Space.seed(space_seed + i)`` for i > 0.
* ``RLToyVectorEnv(seeds=[s0, s1, ...], **config)`` — N *different* MDPs: instance i is the
  reference ``RLToyEnv(**{**config, "seed": seeds[i]})`` verbatim (tables per env in HBM).  Discrete
  configs that ``mdp.device_coverage`` accepts are generated on the device in one launch
  (mdpp_generate.hip, bit-identical to the host builder); ``tables_built_on`` says which path ran.

``rng="numpy"`` (default) keeps numpy ``Generator(PCG64)`` streams per env on the device, so
noise and resets are bit-identical to the reference under identical seeds; ``rng="philox"`` is a
stateless counter-based alternative (no RNG state in HBM, own stream, same distributions).
"""
from __future__ import annotations

import copy
import ctypes as C
from collections.abc import Sequence

import numpy as np
import torch

from . import _capi as capi
from . import mdp as mdp_mod
from . import policy as policy_mod
from .linear_es import LinearES
from .linear_search import LinearSearch
from .summary import EpisodeLog, EpisodeSummary
from .spaces import BatchedSpace, BoxSpace, DiscreteSpace, ImageSpace, TupleSpace

_OBS_FROM_STATE = object()    # _obs_src after a launch that wrote no observations: take them from the state record

_AUTORESET = {"disabled": capi.AUTORESET_DISABLED, "same_step": capi.AUTORESET_SAME_STEP,
              "next_step": capi.AUTORESET_NEXT_STEP}


def _stack(arrs, dtype):
    return np.ascontiguousarray(np.stack([np.asarray(a) for a in arrs]), dtype=dtype)


class _LazyMDPs(Sequence):
    """env.mdps of a handle whose tables were generated on the device: MDP i is built on the host (mdp.build_mdp) the
    first time it is read, and kept."""

    def __init__(self, config, seeds, first):
        self._config, self._seeds = config, list(seeds)
        self._built = {0: first}

    def __len__(self):
        return len(self._seeds)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[k] for k in range(*i.indices(len(self)))]
        n = len(self._seeds)
        i = int(i)
        if i < 0:
            i += n
        if not 0 <= i < n:
            raise IndexError("mdps index out of range")
        m = self._built.get(i)
        if m is None:
            m = self._built[i] = mdp_mod.build_mdp({**self._config, "seed": self._seeds[i]})
        return m


class RLToyVectorEnv:
    metadata = {"render_modes": []}

    def __init__(self, num_envs=None, device=None, *, seeds=None, rng="numpy",
                 autoreset="same_step", max_episode_steps=None, env_id_offset=0,
                 philox_seed=None, episode_stats=False, mdps=None, **config):
        self._lib = capi.load()
        self._h = None
        if not torch.cuda.is_available():
            raise capi.MdppError("RLToyVectorEnv needs a ROCm GPU (torch.cuda.is_available() is False); "
                                 "there is no CPU fallback")
        if autoreset not in _AUTORESET:
            raise ValueError("autoreset must be 'same_step', 'next_step' or 'disabled'")
        if rng not in ("numpy", "philox"):
            raise ValueError("rng must be 'numpy' or 'philox'")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise capi.MdppError("device must be a cuda (ROCm) device")
        if self.device.index is None:          # 'cuda' -> 'cuda:<current>': step() compares tensors' devices with it
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.config = copy.deepcopy(config)   # the reference mutates its config (:339,...); we do not
        self._gen = None                      # mdp.device_gen_params when the per-env tables are generated on the device
        self._learn_rates = None              # [alpha, epsilon] of the learner (set_learner); None: no learner
        self._noise_levels_set = False        # set_noise_levels is in force
        self._learn_q_init = None             # the tensor last handed to set_learner / set_q, kept until its copy has been made
        self._learn_z_init = None             # ... to set_traces
        self._learn_algo = None               # the learner's algorithm ("double_q": two tables per env)
        self._grid_learn_A = None             # the grid learner's number of actions (set_grid_learner); None: never set
        self._grid_q_init = None              # the tensor last handed to set_grid_learner / set_grid_q, kept until its copy has been made
        self._grid_sched = None               # set_grid_learner_schedule's validated arrays while a schedule is in force
        self._grid_ep_init = None             # the tensor last handed to set_grid_learner_episodes, kept until its copy has been made
        self._grid_noise_levels_set = False   # set_grid_noise_levels is in force
        self._learn_pe = {"alpha": None, "gamma": None, "epsilon": None}
        self._learn_pm = False                # set_learner(per_env_mdp=True) is in force (the handle's flag is on)
        self._learn_sched = None              # set_learner_schedule's validated arrays while a schedule is in force
        self._nl_pm = False                   # set_noise_levels(per_env_mdp=True) is in force (the handle's second flag is on)
        self._sched_sweep = False             # set_learner_schedule(sweep=True) has turned the handle's mdpp_learner_schedule_sweep flag on
        self._trace_pm = False                # set_learner_traces(per_env_mdp=True) is in force (the handle's mdpp_learner_traces_per_env_mdp flag is on)
        if seeds is not None:
            if num_envs is not None and num_envs != len(seeds):
                raise ValueError("num_envs != len(seeds)")
            num_envs = len(seeds)
            if mdps is not None:          # prebuilt (mdp.build_many, before the GPU was touched): one per seed, in order
                if len(mdps) != len(seeds):
                    raise ValueError("len(mdps) != len(seeds)")
                self.mdps = list(mdps)
            else:
                # env 0 on the host always: shapes, flags, spaces and the reference's config errors come from it
                first = mdp_mod.build_mdp({**config, "seed": seeds[0]})
                if mdp_mod.device_coverage(self.config, seeds)[0]:
                    self._gen = mdp_mod.device_gen_params(self.config)
                    self._seeds = list(seeds)
                    self.mdps = _LazyMDPs(self.config, seeds, first)
                else:
                    self.mdps = [first] + [mdp_mod.build_mdp({**config, "seed": s}) for s in seeds[1:]]
        else:
            if num_envs is None:
                num_envs = 1
            self.mdps = [mdp_mod.build_mdp(config)]
        self.num_envs = int(num_envs)
        self.env_id_offset = int(env_id_offset)
        self.autoreset = autoreset
        self.rng = rng
        m = self.mdps[0]
        self.kind = m.kind
        self.seed_dict = m.seed_dict
        self._per_env = seeds is not None
        self.seeded_streams = {}

        cfg = capi.MdppConfig()
        cfg.abi_version = capi.MDPP_ABI_VERSION
        cfg.kind = {"discrete": capi.KIND_DISCRETE, "continuous": capi.KIND_CONTINUOUS,
                    "grid": capi.KIND_GRID}[m.kind]
        cfg.num_envs = self.num_envs
        cfg.env_id_offset = self.env_id_offset
        cfg.rng_mode = capi.RNG_NUMPY_PCG64 if rng == "numpy" else capi.RNG_PHILOX
        cfg.autoreset = _AUTORESET[autoreset]
        cfg.max_episode_steps = int(max_episode_steps or 0)
        if philox_seed is None:
            e = m.seed_dict.get("env")
            philox_seed = 0x9E3779B97F4A7C15 if e is None else int(e)
        cfg.philox_seed = int(philox_seed) & (2 ** 64 - 1)
        cfg.delay = int(m.delay)
        cfg.every_n = int(m.reward_every_n_steps)
        cfg.has_reward_noise = int(m.reward_noise is not None)
        cfg.reward_noise = float(m.reward_noise or 0.0)
        cfg.reward_scale = float(m.reward_scale)
        cfg.reward_shift = float(m.reward_shift)
        cfg.term_state_reward = float(m.term_state_reward)
        # the reference's per-episode noise statistics (logged at every reset(), rl_toy_env.py:2231-2247), per env;
        # such handles run on the general kernels
        self.episode_stats = bool(episode_stats)
        cfg.episode_stats = int(self.episode_stats)
        self._irr = False
        if m.kind == "discrete":
            self._init_discrete(cfg)
        elif m.kind == "grid":
            self._init_grid(cfg)
        else:
            self._init_continuous(cfg)
        h = C.c_void_p()
        rc = self._lib.mdpp_create(C.byref(cfg), self.device.index, C.byref(h))
        capi.check(self._lib, None, rc, "mdpp_create")
        self._h = h
        self._cfg = cfg
        if m.kind == "discrete":
            self._upload_discrete()
        elif self._image is not None:
            disc = np.ascontiguousarray(self._image["disc"], dtype=np.uint8)
            rc = self._lib.mdpp_upload_image_disc(self._h, capi.nptr(disc))
            capi.check(self._lib, self._h, rc, "mdpp_upload_image_disc")
            if m.kind == "grid":
                lines = np.ascontiguousarray(self._image["lines"], dtype=np.uint8)
                rc = self._lib.mdpp_upload_image_lines(self._h, capi.nptr(lines))
                capi.check(self._lib, self._h, rc, "mdpp_upload_image_lines")
        self._alloc_buffers()
        if rng == "numpy":
            self._seed_streams(self.seed_dict.get("env"), initial=True)
        # the reference constructor ends with reset(seed=seed_dict["env"]) (:831-833)
        self._reset_all()

    @property
    def tables_built_on(self):
        """"device" when the per-env discrete tables were generated on the GPU (mdpp_generate_discrete), else "host"."""
        return "host" if self._gen is None else "device"

    # ------------------------------------------------------------------ construction helpers
    def _init_discrete(self, cfg):
        m = self.mdps[0]
        for o in ([] if self._gen is not None else self.mdps[1:]):
            if (o.S, o.A, o.sequence_length, o.delay, o.S_irr, o.A_irr) != \
                    (m.S, m.A, m.sequence_length, m.delay, m.S_irr, m.A_irr):
                raise ValueError("per-env MDPs must share S, A, sequence_length and delay")
        cfg.S, cfg.A, cfg.L = m.S, m.A, m.sequence_length
        cfg.num_tables = self.num_envs if self._per_env else 1
        if self._gen is not None:
            unit = self._gen["unit_rewards"]
            custom_r = [False]
        else:
            unit = all(v == 1.0 for mm in self.mdps for k, v in mm.rewardable_sequences.items()
                       if len(k) == mm.sequence_length)
            custom_r = [mm.reward_matrix is not None for mm in self.mdps]
        if any(custom_r) and not all(custom_r):
            raise ValueError("per-env MDPs must all use a reward matrix or all use rewardable sequences")
        cfg.reward_kind = capi.REWARD_STATE_ACTION if custom_r[0] else capi.REWARD_SEQUENCES
        cfg.unit_rewards = int(unit and m.delay <= 32 and not custom_r[0])
        cfg.has_transition_noise = int(bool(m.transition_noise))
        cfg.transition_noise = float(m.transition_noise or 0.0)
        dtype_o = self.config.get("dtype_o", self.config.get("dtype_s", np.int64))
        self._obs_torch_dtype = torch.int32 if np.dtype(dtype_o) == np.int32 else torch.int64
        cfg.obs_dtype = capi.OBS_I32 if self._obs_torch_dtype == torch.int32 else capi.OBS_I64
        self.single_observation_space = DiscreteSpace(m.S, seed=m.seed_dict.get("relevant_state_space"))
        self.single_action_space = DiscreteSpace(m.A, seed=m.seed_dict.get("relevant_action_space"))
        self._irr = bool(m.irrelevant)
        if self._irr:
            # Tuple spaces (:718-733): (relevant, irrelevant) pairs
            cfg.irrelevant, cfg.S_irr, cfg.A_irr = 1, m.S_irr, m.A_irr
            self.single_observation_space = TupleSpace(
                [self.single_observation_space,
                 DiscreteSpace(m.S_irr, seed=m.seed_dict.get("irrelevant_state_space"))],
                seed=m.seed_dict.get("state_space"))
            self.single_action_space = TupleSpace(
                [self.single_action_space,
                 DiscreteSpace(m.A_irr, seed=m.seed_dict.get("irrelevant_action_space"))],
                seed=m.seed_dict.get("action_space"))
        self._image = None
        if m.image is not None:
            from . import image_obs
            im = m.image
            # (with an irrelevant sub-space the observation is one image per sub-space, side by side
            # along x; state s is an (s + 3)-gon in either, so the templates cover the larger one)
            self._image = image_obs.build_templates(max(m.S, m.S_irr) if self._irr else m.S, im)
            cfg.image, cfg.img_w, cfg.img_h = 1, im["width"], im["height"]
            tr = im["transforms"]
            cfg.img_has_scale, cfg.img_has_shift = int("scale" in tr), int("shift" in tr)
            cfg.img_has_rotate, cfg.img_has_flip = int("rotate" in tr), int("flip" in tr)
            cfg.img_sh_quant = int(im["sh_quant"] or 1)
            cfg.img_ro_quant = int(im["ro_quant"] or 1)
            cfg.img_r0 = im["circle_radius"]
            cfg.img_r_min, cfg.img_r_max = self._image["r_min"], self._image["r_max"]
            cfg.img_log_min_r, cfg.img_log_max_r = self._image["log_min_r"], self._image["log_max_r"]
            cfg.img_tpl_size = self._image["tpl_size"]
            cfg.obs_dtype = capi.OBS_IMAGE_U8
            self._obs_torch_dtype = torch.uint8
            self.single_observation_space = ImageSpace((2 if self._irr else 1) * im["width"], im["height"])
        self.transition_matrix = m.P
        self.rewardable_sequences = m.rewardable_sequences
        self.reward_matrix = m.reward_matrix               # use_custom_mdp with matrices (:1259-1267)

    def _upload_discrete(self):
        if self._gen is not None:
            self._generate_discrete()
        else:
            self._upload_discrete_host()
        if self._image is not None:
            t = self._image
            tpl = np.ascontiguousarray(t["tpl"], dtype=np.uint8)
            cx = np.ascontiguousarray(t["cls_x"], dtype=np.int16)
            cy = np.ascontiguousarray(t["cls_y"], dtype=np.int16)
            rc = self._lib.mdpp_upload_image_templates(self._h, capi.nptr(tpl), tpl.shape[1],
                                                       t["n_cls_x"], t["n_cls_y"], capi.nptr(cx),
                                                       capi.nptr(cy))
            capi.check(self._lib, self._h, rc, "mdpp_upload_image_templates")

    def _generate_discrete(self):
        """Every env's tables and streams in one launch (mdpp_generate_discrete); the seed dicts come back to the host."""
        g = self._gen
        p = capi.MdppGenParams()
        p.diameter, p.n_term = g["diameter"], g["n_term"]
        p.maximally_connected, p.repeats = int(g["maximally_connected"]), int(g["repeats"])
        p.total, p.n_sel, p.n_radices = g["total"], g["n_sel"], len(g["radices"])
        for j, r in enumerate(g["radices"]):
            p.radices[j] = r
        rews = g["rews"]
        p.rews, p.n_rews = (None, 0) if rews is None else (rews.ctypes.data, len(rews))
        p.image = int(g["image"])
        sd = np.zeros((self.num_envs, 8), np.uint64)
        p.seed_dicts = sd.ctypes.data
        seeds = np.array(self._seeds, dtype=np.uint64)
        noise = self.mdps[0].noise_cdf()
        noise = None if noise is None else np.ascontiguousarray(noise, dtype=np.float64)
        rc = self._lib.mdpp_generate_discrete(self._h, capi.nptr(seeds), C.byref(p), capi.nptr(g["is_term"]),
                                              capi.nptr(g["init_cdf"]), capi.nptr(noise))
        capi.check(self._lib, self._h, rc, "mdpp_generate_discrete")
        self._seed_dicts = sd

    def _upload_discrete_host(self):
        ms = self.mdps
        unit = bool(self._cfg.unit_rewards)
        P = _stack([m.P for m in ms], np.uint8 if ms[0].S <= 255 else np.uint16)      # (S > 255: 16-bit entries, mdpp_discrete_wide.hip)
        is_term = _stack([m.is_terminal_table() for m in ms], np.uint8)
        init_cdf = _stack([m.init_cdf() for m in ms], np.float64)
        rtable = rbits = None
        if unit:
            rbits = _stack([np.packbits((m.reward_table() != 0).astype(np.uint8), bitorder="little")
                            for m in ms], np.uint8)
        else:
            rtable = _stack([m.reward_table() for m in ms], np.float64)
        noise = ms[0].noise_cdf()
        noise = None if noise is None else np.ascontiguousarray(noise, dtype=np.float64)
        rc = self._lib.mdpp_upload_discrete_tables(self._h, capi.nptr(P), capi.nptr(rtable),
                                                   capi.nptr(rbits), capi.nptr(is_term),
                                                   capi.nptr(init_cdf), capi.nptr(noise))
        capi.check(self._lib, self._h, rc, "mdpp_upload_discrete_tables")
        if self._irr:
            P1 = _stack([m.P_irr for m in ms], np.uint8)
            cdf1 = _stack([m.init_cdf_irr() for m in ms], np.float64)
            noise1 = ms[0].noise_cdf(irrelevant=True)
            noise1 = None if noise1 is None else np.ascontiguousarray(noise1, dtype=np.float64)
            rc = self._lib.mdpp_upload_discrete_irrelevant(self._h, capi.nptr(P1), capi.nptr(cdf1),
                                                           capi.nptr(noise1))
            capi.check(self._lib, self._h, rc, "mdpp_upload_discrete_irrelevant")

    def _init_grid(self, cfg):
        """Grid envs (rl_toy_env.py:539-541, :780-811): int64 cell vectors, one-hot +-1 actions."""
        m = self.mdps[0]
        G = len(m.grid_shape)
        cfg.grid_dims = G
        for d in range(G):
            cfg.grid_shape[d] = int(m.grid_shape[d])
        cfg.grid_target[0], cfg.grid_target[1] = int(m.target_point[0]), int(m.target_point[1])
        cfg.make_denser = int(bool(m.make_denser))
        cfg.has_transition_noise = int(bool(m.transition_noise))
        cfg.transition_noise = float(m.transition_noise or 0.0)
        dtype_o = self.config.get("dtype_o", self.config.get("dtype_s", np.int64))
        self._obs_torch_dtype = torch.int32 if np.dtype(dtype_o) == np.int32 else torch.int64
        cfg.obs_dtype = capi.OBS_I32 if self._obs_torch_dtype == torch.int32 else capi.OBS_I64
        # Box(0, grid_shape, int64) / GridActionSpace(-1, 1) (:780-800)
        self.single_observation_space = BoxSpace(0, 1, (G,), dtype=np.int64, seed=m.seed_dict.get("state_space"))
        self.single_observation_space.high = np.asarray(m.grid_shape, dtype=np.int64)
        self.single_action_space = BoxSpace(-1, 1, (G,), dtype=np.int64, seed=m.seed_dict.get("action_space"))
        self._image = None
        if m.image is not None:
            # ImageContinuous with grid lines (:800-811): uint8 [n_sub * W][H][3]
            from . import image_obs
            im = m.image
            self._image = dict(im, disc=image_obs.disc_template(im["circle_radius"]), n_sub=G // 2,
                               lines=image_obs.grid_line_mask(im["width"], im["height"], list(m.grid_shape)))
            cfg.image, cfg.img_w, cfg.img_h, cfg.img_r0 = 1, im["width"], im["height"], im["circle_radius"]
            cells = m.terminal_states or []
            cfg.n_boxes = len(cells)
            for b, c in enumerate(cells):            # terminal cells (drawn, never terminating) ride in box_lo
                cfg.box_lo[2 * b], cfg.box_lo[2 * b + 1] = float(c[0]), float(c[1])
            cfg.obs_dtype = capi.OBS_IMAGE_U8
            self._obs_torch_dtype = torch.uint8
            self.single_observation_space = BoxSpace(0, 255, (self._image["n_sub"] * im["width"], im["height"], 3),
                                                     dtype=np.uint8)

    def _init_continuous(self, cfg):
        m = self.mdps[0]
        if self._per_env:
            # continuous MDPs carry no generated tables: per-env seeds only change the streams
            pass
        cfg.D, cfg.n_rel, cfg.order = m.D, len(m.relevant_indices), m.order
        self._line_L = 0
        if m.reward_function == "move_along_a_line":
            cfg.reward_function, cfg.L = capi.CREWARD_MOVE_ALONG_A_LINE, m.sequence_length
            self._line_L = int(m.sequence_length)
        for j, r in enumerate(m.relevant_indices):
            cfg.rel_idx[j] = int(r)
            cfg.target[j] = float(m.target_point[j])
        cfg.make_denser = int(bool(m.make_denser))
        cfg.target_f64 = int(bool(m.target_default))      # the default target_point: float64 zeros (:652-654)
        cfg.has_p_noise = int(m.transition_noise is not None)
        cfg.p_noise = float(m.transition_noise or 0.0)
        cfg.inertia, cfg.time_unit = float(m.inertia), float(m.time_unit)
        cfg.state_space_max, cfg.action_space_max = float(m.state_space_max), float(m.action_space_max)
        cfg.target_radius, cfg.action_loss_weight = float(m.target_radius), float(m.action_loss_weight)
        nb = 0 if m.box_lo is None else len(m.box_lo)
        # (the reference has no limit, rl_toy_env.py:891-956; here the cubes ride in the handle's argument block, [nb][n_rel]
        #  floats in arrays of MAX_BOXES * MAX_DIM: 64 cubes at four relevant dimensions; pictures draw them from a device list)
        if nb * cfg.n_rel > capi.MAX_BOXES * capi.MAX_DIM:
            raise NotImplementedError(f"at most {capi.MAX_BOXES * capi.MAX_DIM // max(cfg.n_rel, 1)} terminal hypercubes at "
                                      f"{cfg.n_rel} relevant dimensions")
        cfg.n_boxes = nb
        for b in range(nb):
            for j in range(cfg.n_rel):
                cfg.box_lo[b * cfg.n_rel + j] = float(m.box_lo[b][j])
                cfg.box_hi[b * cfg.n_rel + j] = float(m.box_hi[b][j])
        cfg.obs_dtype = capi.OBS_F32
        self._obs_torch_dtype = torch.float32
        self.single_observation_space = BoxSpace(-m.state_space_max, m.state_space_max, (m.D,),
                                                 seed=m.seed_dict.get("state_space"))
        self._image = None
        if m.image is not None:
            # ImageContinuous observations (:770-778): uint8 [n_sub * W][H][3]; no random transforms
            from . import image_obs
            im = m.image
            if not np.isfinite(m.state_space_max):
                raise AssertionError("ImageContinuous needs a bounded feature space")   # image_continuous.py:62-63
            self._image = dict(im, disc=image_obs.disc_template(im["circle_radius"]), n_sub=2 if m.D > 2 else 1)
            cfg.image, cfg.img_w, cfg.img_h, cfg.img_r0 = 1, im["width"], im["height"], im["circle_radius"]
            cfg.obs_dtype = capi.OBS_IMAGE_U8
            self._obs_torch_dtype = torch.uint8
            self.single_observation_space = BoxSpace(0, 255, (self._image["n_sub"] * im["width"], im["height"], 3),
                                                     dtype=np.uint8)
        self.single_action_space = BoxSpace(-m.action_space_max, m.action_space_max, (m.D,),
                                            seed=m.seed_dict.get("action_space"))

    def _alloc_buffers(self):
        N, dev = self.num_envs, self.device
        shape = self._obs_shape(N)
        self._obs = torch.zeros(shape, dtype=self._obs_torch_dtype, device=dev)
        self._final_obs = torch.zeros(shape, dtype=self._obs_torch_dtype, device=dev)
        self._reward = torch.zeros(N, dtype=torch.float32, device=dev)
        self._term = torch.zeros(N, dtype=torch.uint8, device=dev)
        self._trunc = torch.zeros(N, dtype=torch.uint8, device=dev)
        # batched spaces, as gymnasium's VectorEnv exposes them next to the single_* ones
        self.observation_space = BatchedSpace(self.single_observation_space, N)
        self.action_space = BatchedSpace(self.single_action_space, N)
        # everything step() passes on every call, prepared once (the call itself is the hot path)
        self._mdpp_step = self._lib.mdpp_step
        self._p_obs, self._p_final = self._obs.data_ptr(), self._final_obs.data_ptr()
        self._p_reward, self._p_term, self._p_trunc = (self._reward.data_ptr(), self._term.data_ptr(),
                                                        self._trunc.data_ptr())
        self._term_b, self._trunc_b = self._term.view(torch.bool), self._trunc.view(torch.bool)
        self._info = {"final_obs": self._final_obs} if self.autoreset == "same_step" else {}
        self._act_dtype = torch.float32 if self.kind == "continuous" else torch.int32
        if self.kind == "discrete":
            self._act_shape = torch.Size((N, 2) if self._irr else (N,))
        elif self.kind == "grid":
            self._act_shape = torch.Size((N, len(self.mdps[0].grid_shape)))
        else:
            self._act_shape = torch.Size((N, self.mdps[0].D))

    def _obs_shape(self, *lead):
        if self.kind == "continuous":
            if getattr(self, "_image", None) is not None:
                im = self._image
                return tuple(lead) + (im["n_sub"] * im["width"], im["height"], 3)
            return tuple(lead) + (self.mdps[0].D,)
        if self.kind == "grid":
            if getattr(self, "_image", None) is not None:
                im = self._image
                return tuple(lead) + (im["n_sub"] * im["width"], im["height"], 3)
            return tuple(lead) + (len(self.mdps[0].grid_shape),)
        if getattr(self, "_image", None) is not None:
            im = self.mdps[0].image
            return tuple(lead) + ((2 if getattr(self, "_irr", False) else 1) * im["width"], im["height"], 1)
        if getattr(self, "_irr", False):
            return tuple(lead) + (2,)
        return tuple(lead)

    def _seed_streams(self, env_seed, initial):
        """Env streams: PCG64(SeedSequence(env_seed + global id)), i.e. what reset(seed=...) does
        (gymnasium Env.reset -> seeding.np_random; rl_toy_env.py:2225).  Space streams are only
        (re)built at construction."""
        N, off = self.num_envs, self.env_id_offset
        if self._gen is not None:
            # device-generated handle: the generator seeded every stream; a re-seed runs SeedSequence on the device
            if initial:
                for st in (capi.STREAM_ENV, capi.STREAM_SPACE) + ((capi.STREAM_IMAGE,) if self._image is not None else ()):
                    self.seeded_streams[st] = self.get_rng_streams(st)
                return
            if env_seed + off + N - 1 < 2 ** 64:
                seeds = np.uint64(env_seed + off) + np.arange(N, dtype=np.uint64)
                rc = self._lib.mdpp_seed_streams_seedseq(self._h, capi.STREAM_ENV, capi.nptr(seeds))
                capi.check(self._lib, self._h, rc, "mdpp_seed_streams_seedseq")
                self.seeded_streams[capi.STREAM_ENV] = self.get_rng_streams(capi.STREAM_ENV)
            else:
                self._put_stream(capi.STREAM_ENV, np.stack([mdp_mod.pcg64_words(mdp_mod.new_generator(env_seed + off + i))
                                                            for i in range(N)]))
            return
        if self._per_env:
            env_words = np.stack([mdp_mod.pcg64_words(mdp_mod.new_generator(
                m.seed_dict["env"] if env_seed is None or initial else env_seed + off + i))
                for i, m in enumerate(self.mdps)])
        else:
            base = None if env_seed is None else env_seed + off
            env_words = mdp_mod.fresh_stream_words(base, N)
        self._put_stream(capi.STREAM_ENV, env_words)
        if not initial:
            return
        if self.kind == "discrete":
            if self._per_env:
                sp = np.stack([m.space_rng_words for m in self.mdps])
            else:
                # (with an irrelevant sub-space the Tuple re-seeded both state spaces: space_seeds)
                R = self.mdps[0].space_seeds[0]
                sp = mdp_mod.fresh_stream_words(R + off, N)
                if off == 0:
                    sp[0] = self.mdps[0].space_rng_words   # the reference's own generator, post-P
        else:
            if self._per_env:
                sp = np.stack([mdp_mod.pcg64_words(mdp_mod.new_generator(m.seed_dict["state_space"]))
                               for m in self.mdps])
            else:
                sp = mdp_mod.fresh_stream_words(self.seed_dict["state_space"] + off, N)
        self._put_stream(capi.STREAM_SPACE, sp)
        if self.kind == "grid":                      # GridActionSpace(seed=seed_dict["action_space"]), :793-797
            if self._per_env:
                ac = np.stack([mdp_mod.pcg64_words(mdp_mod.new_generator(m.seed_dict["action_space"]))
                               for m in self.mdps])
            else:
                ac = mdp_mod.fresh_stream_words(self.seed_dict["action_space"] + off, N)
            self._put_stream(capi.STREAM_ACTION, ac)
        if self.kind == "discrete" and self._irr:
            if self._per_env:
                sp1 = np.stack([m.space_irr_rng_words for m in self.mdps])
            else:
                sp1 = mdp_mod.fresh_stream_words(self.mdps[0].space_seeds[1] + off, N)
                if off == 0:
                    sp1[0] = self.mdps[0].space_irr_rng_words
            self._put_stream(capi.STREAM_SPACE_IRR, sp1)
        if self.kind == "discrete" and self._image is not None:
            if self._per_env:
                im = np.stack([mdp_mod.pcg64_words(mdp_mod.new_generator(m.image["seed"])) for m in self.mdps])
            else:
                im = mdp_mod.fresh_stream_words(self.mdps[0].image["seed"] + off, N)
            self._put_stream(capi.STREAM_IMAGE, im)

    def _put_stream(self, stream, words):
        words = np.ascontiguousarray(words, dtype=np.uint64)
        assert words.shape == (self.num_envs, 6)
        self.seeded_streams[stream] = words.copy()   # what was last uploaded (tests, checkpoints)
        rc = self._lib.mdpp_seed_streams(self._h, stream, capi.nptr(words))
        capi.check(self._lib, self._h, rc, "mdpp_seed_streams")

    # ------------------------------------------------------------------ Gym-style API
    def _stream(self):
        return C.c_void_p(self._raw_stream())

    def _raw_stream(self):
        """The caller's current HIP stream as an integer.  torch.cuda.current_stream() builds a Stream object (1.8 us per
        call on the GPU box, tools/host_cost.py) -- a third of a single step's host time; the raw getter takes 0.1 us."""
        get = getattr(torch._C, "_cuda_getCurrentRawStream", None)
        if get is not None:
            return get(self.device.index)
        return torch.cuda.current_stream(self.device).cuda_stream

    def _reset_all(self, mask=None):
        mptr = None
        if mask is not None:
            mask = mask.to(device=self.device, dtype=torch.uint8).contiguous()
            mptr = C.c_void_p(mask.data_ptr())
            src = getattr(self, "_obs_src", None)
            if src is _OBS_FROM_STATE and self.kind == "grid":   # (a grid summary launch: the cells in the state record)
                cells = self._get_augmented_state()["curr_obs"]
                self._obs.copy_(torch.from_numpy(cells).to(device=self.device, dtype=self._obs.dtype))
            elif src is _OBS_FROM_STATE:   # (a summary launch: the observation every env shows, from its state record)
                self._closed_call(self._lib.mdpp_current_obs(self._h, C.c_void_p(self._obs.data_ptr()), self._stream()), "mdpp_current_obs")
            elif src is not None:        # the rows of the envs NOT reset: their observation after the last rollout() / graph replay
                self._obs.copy_(src)
        self._obs_src = None
        rc = self._lib.mdpp_reset(self._h, mptr, C.c_void_p(self._obs.data_ptr()), self._stream())
        capi.check(self._lib, self._h, rc, "mdpp_reset")
        return self._obs

    def reset(self, seed=None, options=None, mask=None):
        """reset(seed=None) -> (obs, {}), rl_toy_env.py:2217.  ``seed`` re-seeds env i's generator
        with seed + i first, as the reference (gymnasium Env.reset) does.  ``mask`` (bool[N])
        restricts the reset to some envs."""
        if seed is not None:
            if self.rng != "numpy":
                raise capi.MdppError("reset(seed=...) re-seeds numpy streams; this env uses rng='philox'")
            if not isinstance(seed, int) or seed < 0:
                raise TypeError("seed must be a non-negative python int")
            self._seed_streams(seed, initial=False)
        return self._reset_all(mask), {}

    def seed(self, seed=None):
        """seed(seed) -> int, rl_toy_env.py:2379-2406: re-seeds the env generators (not the spaces') —
        env i of the batch gets seed + i, like reset(seed=...) — and returns the seed; None draws one
        from OS entropy as gymnasium's seeding.np_random does."""
        if self.rng != "numpy":
            raise capi.MdppError("seed() re-seeds numpy streams; this env uses rng='philox'")
        if seed is None:
            seed = int(np.random.SeedSequence().entropy)
        if not isinstance(seed, int) or seed < 0:
            raise TypeError("seed must be a non-negative python int")    # gymnasium.utils.seeding.np_random
        self._seed_streams(seed, initial=False)
        self.seed_ = seed
        return seed

    def step_graph(self, actions):
        """A replayable HIP graph of K single steps (K = actions.shape[0] mdpp_step launches captured
        once): the one-launch-per-step API without the per-call host cost.  actions: [K, N, ...] as for
        rollout(); the tensor is read at every replay, so writing new actions into it between replays
        steps with them.  Returns a StepGraph with .replay() and the output buffers
        .obs/.reward/.terminated/.truncated ([K, N, ...]).

        The handle's step counter travels BY VALUE into captured launches (include/mdpp.h).  Where that would not replay
        exactly -- Philox streams key their draws by the counter, a delay line kept in memory starts at counter mod delay --
        the launches are captured in the library's capture mode instead: they add a device word to the counter, which
        replay() sets to (counter now - counter at capture) right before the graph (mdpp_graph_capture /
        mdpp_graph_set_tick_offset, round 4; image handles too since round 5)."""
        self._noise_levels_refuse()
        K = int(actions.shape[0])
        ok = self._lib.mdpp_graph_replay_exact(self._h, K)
        if ok < 0:
            capi.check(self._lib, self._h, ok, "mdpp_graph_replay_exact")
        if ok == 0:
            raise capi.MdppError(
                "step_graph: a captured graph of %d steps does not replay exactly for this handle (delay = %d). "
                "Use rollout() (one fused launch) instead." % (K, self._cfg.delay))
        by_offset = ok == 2
        a = self._as_actions(actions, K)
        obs, rew, term, trunc = self.alloc_rollout(K)
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        g = torch.cuda.CUDAGraph()
        step, h = self._lib.mdpp_step, self._h

        def launches(stream):
            for k in range(K):
                rc = step(h, a[k].data_ptr(), obs[k].data_ptr(), rew[k].data_ptr(), term[k].data_ptr(),
                          trunc[k].data_ptr(), None, stream)
                if rc:
                    capi.check(self._lib, h, rc, "mdpp_step")
        tick0 = C.c_uint64()
        capi.check(self._lib, h, self._lib.mdpp_tick(h, 0, C.byref(tick0)), "mdpp_tick")
        try:
            if by_offset:
                capi.check(self._lib, h, self._lib.mdpp_graph_capture(h, 1), "mdpp_graph_capture")
            # (thread-local capture: the captured launches make no call that is unsafe during a capture, and in the default
            #  global mode a HIP call from ANY other thread of the process -- a process group's watchdog querying its events,
            #  RCCL's own threads -- invalidates the capture; the failed graph's destructor then aborts the process)
            with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
                launches(side.cuda_stream)
        finally:
            if by_offset:
                self._lib.mdpp_graph_capture(h, 0)
            # the capture advanced the counter although nothing ran
            now = C.c_uint64()
            self._lib.mdpp_tick(h, 0, C.byref(now))
            self._lib.mdpp_tick(h, int(tick0.value) - int(now.value), None)
        return StepGraph(self, g, K, int(tick0.value), a, obs, rew, term, trunc, by_offset)

    def step(self, actions):
        """step(actions) -> (obs, reward, terminated, truncated, info), rl_toy_env.py:1992.
        Returned tensors alias preallocated device buffers (valid until the next call)."""
        a = actions
        if not (torch.is_tensor(a) and a.dtype == self._act_dtype and a.device == self.device
                and a.shape == self._act_shape and a.is_contiguous()):
            a = self._as_actions(actions, None)
        rc = self._mdpp_step(self._h, a.data_ptr(), self._p_obs, self._p_reward, self._p_term,
                             self._p_trunc, self._p_final, self._raw_stream())
        if rc:
            capi.check(self._lib, self._h, rc, "mdpp_step")
        self._obs_src = None
        return self._obs, self._reward, self._term_b, self._trunc_b, self._info

    def rollout(self, actions, out=None):
        """K fused steps in ONE kernel launch (per-env state stays in registers).
        actions: [K, N] int32 or [K, N, D] float32, time-major.  Returns (obs, reward, terminated,
        truncated) with a leading K axis; equivalent to K step() calls."""
        self._noise_levels_refuse()
        K = int(actions.shape[0])
        a = self._as_actions(actions, K)
        if out is None:
            out = self.alloc_rollout(K)
        obs, rew, term, trunc = out
        rc = self._lib.mdpp_step_n(self._h, K, C.c_void_p(a.data_ptr()), C.c_void_p(obs.data_ptr()),
                                   C.c_void_p(rew.data_ptr()), C.c_void_p(term.data_ptr()),
                                   C.c_void_p(trunc.data_ptr()), self._stream())
        capi.check(self._lib, self._h, rc, "mdpp_step_n")
        self._obs_src = obs[K - 1]        # (a view: reset(mask=...) shows it for the envs it leaves alone)
        return obs, rew, term.view(torch.bool), trunc.view(torch.bool)

    # ------------------------------------------------------------------ closed-loop rollouts under a tabular policy
    def set_policy(self, policy=None, *, thresholds=None, seed=0):
        """The handle's tabular policy for rollout_policy(): ``policy`` float [S, A] probabilities or integer [S] actions
        (policy.policy_thresholds makes the kernel's thresholds from it on the host), or ``thresholds`` -- a device uint32
        [S, A] tensor with non-decreasing rows, used as given (copied on the current stream: a policy is replaced between
        rollouts without a host round trip).  ``seed``: the 64-bit key of the policy's own Philox stream.  Neither
        argument: the policy is cleared.  Handles the kernel does not serve raise NotImplementedError with the reason."""
        if policy is not None and thresholds is not None:
            raise ValueError("set_policy: give policy or thresholds, not both")
        if policy is None and thresholds is None:
            capi.check(self._lib, self._h, self._lib.mdpp_clear_policy(self._h), "mdpp_clear_policy")
            return
        self._policy_check_config()
        S, A = self.mdps[0].S, self.mdps[0].A
        if thresholds is None:
            thr = torch.from_numpy(policy_mod.policy_thresholds(policy, S, A).view(np.int32)).to(self.device).view(torch.uint32)
        else:
            thr = thresholds
            if not (torch.is_tensor(thr) and thr.dtype == torch.uint32 and thr.device == self.device
                    and tuple(thr.shape) == (S, A)):
                raise ValueError(f"set_policy: thresholds must be a uint32 tensor of shape ({S}, {A}) on {self.device}")
            thr = thr.contiguous()
        rc = self._lib.mdpp_set_policy(self._h, C.c_void_p(thr.data_ptr()), C.c_uint64(int(seed) & (2 ** 64 - 1)), self._stream())
        self._closed_call(rc, "mdpp_set_policy")
        self._policy_thr = thr           # (kept until the copy queued on the stream has certainly been made)

    def _policy_check_config(self):
        """What the config alone rules out, before the library is asked: the env kind, and a noise key -- a config that
        names transition_noise or reward_noise is refused even at 0 (the library sees no transition-noise key at 0.0)."""
        if self.kind != "discrete":
            raise NotImplementedError("policy rollouts serve discrete envs only (this env is %s)" % self.kind)
        for key in ("transition_noise", "reward_noise"):
            if self.config.get(key) is not None:
                raise NotImplementedError("policy rollouts do not serve a %s key (config[%r] = %r)" % (key, key, self.config[key]))

    def _closed_call(self, rc, what):
        """The return code of a closed-loop call: a handle the kernel does not serve raises NotImplementedError with the reason."""
        if rc == capi.EUNSUPPORTED:
            msg = self._lib.mdpp_last_error(self._h)
            raise NotImplementedError(msg.decode() if msg else what + ": unsupported")
        capi.check(self._lib, self._h, rc, what)

    def _alloc_rollout_closed(self, K):
        return self.alloc_rollout(K) + (torch.empty((K, self.num_envs), dtype=torch.int32, device=self.device),)

    def _rollout_closed(self, step_n, what, K, out):
        """K closed-loop steps through step_n (mdpp_step_n_policy / mdpp_step_n_learn)."""
        if out is None:
            out = self._alloc_rollout_closed(K)
        obs, rew, term, trunc, act = out
        rc = step_n(self._h, K, C.c_void_p(act.data_ptr()), C.c_void_p(obs.data_ptr()), C.c_void_p(rew.data_ptr()),
                    C.c_void_p(term.data_ptr()), C.c_void_p(trunc.data_ptr()), self._stream())
        self._closed_call(rc, what)
        self._obs_src = obs[K - 1]        # (a view: reset(mask=...) shows it for the envs it leaves alone)
        return obs, rew, term.view(torch.bool), trunc.view(torch.bool), act

    def _rollout_summary(self, step_n, what, K, summary, log=None):
        """K closed-loop steps through the entry point step_n, named ``what``, that keep ``summary`` and write no [K, N] array:
        mdpp_step_n_learn_summary / _eval_summary, or with ``log`` mdpp_step_n_learn_log, which keeps the episode log too
        (the caller picks the pair)."""
        if not isinstance(summary, EpisodeSummary):
            raise ValueError(f"{what}: summary must be an EpisodeSummary (env.episode_summary())")
        summary.check(self.num_envs, self.device, what)
        if log is None:
            rc = step_n(self._h, K, *(C.c_void_p(t.data_ptr()) for t in summary.tensors()), self._stream())
        else:
            if not isinstance(log, EpisodeLog):
                raise ValueError(f"{what}: log must be an EpisodeLog (env.episode_log(max_episodes))")
            log.check(self.num_envs, self.device, what)
            rc = step_n(self._h, K, *(C.c_void_p(t.data_ptr()) for t in summary.tensors() + log.tensors()),
                        log.max_episodes, self._stream())
        self._closed_call(rc, what)
        self._obs_src = _OBS_FROM_STATE
        return summary

    def episode_summary(self):
        """A new EpisodeSummary for this handle (summary.py): five zeroed [N] device tensors -- ret, len, episodes, return_sum,
        length_sum -- for rollout_learn(K, summary=) / rollout_eval(K, summary=); pop() reads and zeroes the finished episodes'
        three, clear() zeroes all five (call it after reset(): the handle knows nothing of the object)."""
        return EpisodeSummary(self.num_envs, self.device)

    def episode_log(self, max_episodes):
        """A new EpisodeLog for this handle (summary.py): count [N], ret and len [max_episodes, N], zeroed device tensors, for
        rollout_learn(K, summary=, log=) -- the return and length of every episode each env
        finishes, by the env's own episode index; curve() is the learning curve.  Nothing of it lives in the handle."""
        return EpisodeLog(self.num_envs, max_episodes, self.device)

    def alloc_rollout_policy(self, K):
        """Output buffers of rollout_policy(K): alloc_rollout(K) and the actions, int32 [K, N]."""
        return self._alloc_rollout_closed(K)

    def rollout_policy(self, K, out=None):
        """K closed-loop steps in ONE kernel launch: at every step each env draws its action from the policy's row of the
        state it is in and takes it.  Returns (obs, reward, terminated, truncated, actions), each with a leading K axis;
        rollout(actions) on an identically built env returns the same first four, bit for bit."""
        self._policy_check_config()
        return self._rollout_closed(self._lib.mdpp_step_n_policy, "mdpp_step_n_policy", int(K), out)

    def policy_kernel_name(self, K):
        """Name (with template arguments) of the kernel rollout_policy(K) launches (mdpp_policy_kernel_name; nothing is
        launched); empty for a handle it does not serve."""
        try:
            self._policy_check_config()
        except NotImplementedError:
            return ""
        name = self._lib.mdpp_policy_kernel_name(self._h, int(K))
        return name.decode() if name else ""

    # ------------------------------------------------------------------ closed-loop continuous rollouts under a linear policy
    def _linear_theta_arg(self, theta, history=1):
        """theta as a contiguous float32 device tensor and whether it is per-env; ValueError for anything but float32
        [D, C] or [N, D, C] with C = history * D + 1 (numpy or torch, any device), before any device work."""
        if self.kind != "continuous":
            raise NotImplementedError("linear-policy rollouts serve continuous envs only (this env is %s)" % self.kind)
        D, N = self.mdps[0].D, self.num_envs
        cols = history * D + 1
        if isinstance(theta, np.ndarray):
            t = torch.from_numpy(np.ascontiguousarray(theta)) if theta.dtype == np.float32 else None
        else:
            t = theta if torch.is_tensor(theta) and theta.dtype == torch.float32 else None
        if t is None or tuple(t.shape) not in ((D, cols), (N, D, cols)):
            raise ValueError(f"set_linear_policy: theta must be float32 of shape ({D}, {cols}) or ({N}, {D}, {cols})")
        return t.to(self.device).contiguous(), t.dim() == 3

    def set_linear_policy(self, theta=None, history=1):
        """The handle's linear policy for rollout_linear(): float32 ``theta`` of shape [D, D + 1] -- one policy shared by every
        env -- or [N, D, D + 1] -- one per env --, numpy or torch on any device; theta[..., r, :D] is row r of W and
        theta[..., r, D] is b[r] of  a = clip(W o + b, +-action_space_max)  (include/mdpp.h "Linear policies").  Copied on
        the current stream: parameters are replaced between rollouts without a host round trip.  None clears the policy.
        Handles the kernel does not serve raise NotImplementedError with the reason.
        ``history=2``: a policy with memory, a = clip(W o + V p + b) with p the observation the env acted on at its previous
        step (o itself on the first step of an episode); theta is [D, 2 D + 1] or [N, D, 2 D + 1], theta[..., r, D:2 D] row r
        of V and theta[..., r, 2 D] b[r] (include/mdpp.h "Linear policies with memory").  Setting one sets every env's memory
        to its current state.  Any other history raises ValueError."""
        if theta is None:
            capi.check(self._lib, self._h, self._lib.mdpp_clear_linear_policy(self._h), "mdpp_clear_linear_policy")
            self._linear_per_env = None
            return
        if isinstance(history, bool) or history not in (1, 2):
            raise ValueError("set_linear_policy: history must be 1 or 2")
        t, per_env = self._linear_theta_arg(theta, int(history))
        if history == 1:
            rc, what = self._lib.mdpp_set_linear_policy(self._h, C.c_void_p(t.data_ptr()), int(per_env), self._stream()), "mdpp_set_linear_policy"
        else:
            rc = self._lib.mdpp_set_linear_policy_history(self._h, C.c_void_p(t.data_ptr()), int(per_env), 2, self._stream())
            what = "mdpp_set_linear_policy_history"
        self._closed_call(rc, what)
        self._linear_theta = t           # (kept until the copy queued on the stream has certainly been made)
        self._linear_per_env = per_env

    @property
    def linear_policy_history(self):
        """The history of the linear policy in force, 1 or 2, as the handle itself says (mdpp_linear_policy_history); 0 without
        a policy."""
        return int(self._lib.mdpp_linear_policy_history(self._h)) if self.kind == "continuous" else 0

    def _linear_cols(self):
        """The columns of one row of theta: D + 1, or 2 D + 1 under a policy with memory."""
        return max(1, self.linear_policy_history) * self.mdps[0].D + 1

    def get_linear_policy(self):
        """The handle's parameters as a device tensor, in the shape they were set in."""
        if getattr(self, "_linear_per_env", None) is None:
            raise capi.MdppError("get_linear_policy: no linear policy set")
        D = self.mdps[0].D
        out = torch.empty(((self.num_envs,) if self._linear_per_env else ()) + (D, self._linear_cols()), dtype=torch.float32, device=self.device)
        self._closed_call(self._lib.mdpp_get_linear_policy(self._h, C.c_void_p(out.data_ptr()), self._stream()), "mdpp_get_linear_policy")
        return out

    def get_linear_memory(self):
        """The memory of a history=2 policy -- per env the observation it last acted on -- as a float32 device tensor [N, D]."""
        out = torch.empty((self.num_envs, self.mdps[0].D), dtype=torch.float32, device=self.device)
        self._closed_call(self._lib.mdpp_linear_memory(self._h, C.c_void_p(out.data_ptr()), 0, self._stream()), "mdpp_linear_memory")
        return out

    def set_linear_memory(self, p):
        """Replace the memory of a history=2 policy: float32 [N, D], numpy or torch on any device (checkpoints)."""
        D, N = self.mdps[0].D, self.num_envs
        t = torch.from_numpy(np.ascontiguousarray(p)) if isinstance(p, np.ndarray) else p
        if not (torch.is_tensor(t) and t.dtype == torch.float32 and tuple(t.shape) == (N, D)):
            raise ValueError(f"set_linear_memory: p must be float32 of shape ({N}, {D})")
        t = t.to(self.device).contiguous()
        self._closed_call(self._lib.mdpp_linear_memory(self._h, C.c_void_p(t.data_ptr()), 1, self._stream()), "mdpp_linear_memory")
        self._linear_memory_arg = t      # (kept until the copy queued on the stream has certainly been made)

    def alloc_rollout_linear(self, K):
        """Output buffers of rollout_linear(K): alloc_rollout(K) and the actions, float32 [K, N, D]."""
        return self.alloc_rollout(K) + (torch.empty((K, self.num_envs, self.mdps[0].D), dtype=torch.float32, device=self.device),)

    def linear_search(self, sigma, *, seed, episodes_per_trial=1, sigma_up=1.0, sigma_down=1.0, sigma_max=float("inf")):
        """A new LinearSearch (linear_search.py) for rollout_linear(K, search=): one (1+1)-ES per env on the per-env linear policy
        this handle holds, which becomes each env's trial 0 and first incumbent.  ``sigma``: the step size, a scalar or a float32
        array [N]; after trial 0 an accepted trial multiplies an env's sigma by ``sigma_up`` (clamped to ``sigma_max``), a
        rejected one by ``sigma_down``; a trial is ``episodes_per_trial`` whole episodes of the env's own.  ValueError for bad
        shapes, dtypes or values; NotImplementedError for a shared policy or a handle the kernel does not serve."""
        if self.kind != "continuous":
            raise NotImplementedError("linear-policy rollouts serve continuous envs only (this env is %s)" % self.kind)
        if not self._lib.mdpp_linear_search_kernel_name(self._h, 1, 0):       # (a dry run: the C side's own refusals and their text)
            msg = (self._lib.mdpp_last_error(self._h) or b"").decode()
            if "no linear policy set" in msg:
                raise capi.MdppError(msg)
            raise NotImplementedError(msg or "linear_search: this handle is not served")
        return LinearSearch(self.get_linear_policy(), sigma, seed=seed, episodes_per_trial=episodes_per_trial, sigma_up=sigma_up,
                            sigma_down=sigma_down, sigma_max=sigma_max)

    def _linear_search_arg(self, search, what):
        if not isinstance(search, LinearSearch):
            raise ValueError(f"{what}: search must be a LinearSearch (env.linear_search(sigma, seed=...))")
        search.check(self.num_envs, self.mdps[0].D, self.device, what, cols=self._linear_cols())
        return C.byref(search.c_struct())

    def linear_es(self, mean_theta, sigma, lr, *, seed, episodes_per_member=1, log_generations=0):
        """A new LinearES (linear_es.py) for rollout_linear(K, es=): one antithetic ES per group of 64 envs on the per-env linear
        policy this handle holds.  ``mean_theta``: the start means, float32 [G, D, D + 1] with G = N / 64, or one [D, D + 1]
        start for every group (numpy or torch); ``sigma`` (> 0) and ``lr`` (>= 0): scalars or float32 arrays [G]; a member is
        judged on ``episodes_per_member`` whole episodes; ``log_generations`` rows of the per-generation mean score are kept.
        The candidates of generation 0 are written into the handle's parameters (mdpp_linear_es_init): call it after
        reset().  ValueError for bad shapes, dtypes or values; NotImplementedError for a shared policy, N % 64 != 0 or a
        handle the kernel does not serve."""
        if self.kind != "continuous":
            raise NotImplementedError("linear-policy rollouts serve continuous envs only (this env is %s)" % self.kind)
        if not self._lib.mdpp_linear_es_kernel_name(self._h, 1, 0):           # (a dry run: the C side's own refusals and their text)
            msg = (self._lib.mdpp_last_error(self._h) or b"").decode()
            if "no linear policy set" in msg:
                raise capi.MdppError(msg)
            raise NotImplementedError(msg or "linear_es: this handle is not served")
        D, G, cols = self.mdps[0].D, self.num_envs // 64, self._linear_cols()
        m = torch.from_numpy(np.ascontiguousarray(mean_theta)) if isinstance(mean_theta, np.ndarray) else mean_theta
        if not (torch.is_tensor(m) and m.dtype == torch.float32 and tuple(m.shape) in ((D, cols), (G, D, cols))):
            raise ValueError(f"linear_es: mean_theta must be float32 of shape ({D}, {cols}) or ({G}, {D}, {cols})")
        if m.dim() == 2:
            m = m.unsqueeze(0).expand(G, D, cols)
        es = LinearES(m.to(self.device).contiguous(), sigma, lr, seed=seed, episodes_per_member=episodes_per_member,
                      log_generations=log_generations)
        self.linear_es_init(es)
        return es

    def linear_es_init(self, es):
        """mdpp_linear_es_init: write the candidates of ``es``'s current generation (mean +- sigma z) into the handle's
        parameters and start every member on a fresh episode count (acc = ret = 0, eps = 0), on the current stream.  After
        reset(), and after LinearES.load_state_dict()."""
        sr = self._linear_es_arg(es, "mdpp_linear_es_init")
        self._closed_call(self._lib.mdpp_linear_es_init(self._h, sr, self._stream()), "mdpp_linear_es_init")

    def _linear_es_arg(self, es, what):
        if not isinstance(es, LinearES):
            raise ValueError(f"{what}: es must be a LinearES (env.linear_es(mean_theta, sigma, lr, seed=...))")
        es.check(self.num_envs, self.mdps[0].D, self.device, what, cols=self._linear_cols())
        return C.byref(es.c_struct())

    def rollout_linear(self, K, out=None, *, summary=None, search=None, es=None):
        """K closed-loop steps in ONE kernel launch: at every step each env forms its action from the state it shows with its
        linear policy and takes it.  Returns (obs, reward, terminated, truncated, actions), each with a leading K axis;
        rollout(actions) on an identically built env returns the same first four, bit for bit.  ``summary`` (an
        EpisodeSummary from env.episode_summary()): the same K steps with no [K, N] output -- the summary is updated and
        returned.  ``search`` (a LinearSearch from env.linear_search()): every env also runs its (1+1)-ES in the launch --
        trials end with the env's own episodes, accepted candidates become ``search.best`` and the next candidate replaces the
        env's parameters (get_linear_policy()); what is returned is the same.  ``es`` (a LinearES from env.linear_es()): every
        group of 64 envs runs one antithetic ES in the launch -- ``es.mean`` moves at every generation end and the next
        candidates replace the envs' parameters; exclusive with ``search``."""
        if self.kind != "continuous":
            raise NotImplementedError("linear-policy rollouts serve continuous envs only (this env is %s)" % self.kind)
        if search is not None and es is not None:
            raise ValueError("rollout_linear: search and es are exclusive")
        K = int(K)
        agent = search is not None or es is not None
        if agent:
            stem = "mdpp_step_n_linear_search" if search is not None else "mdpp_step_n_linear_es"
            what = stem + "_summary" if summary is not None else stem
            sr = self._linear_search_arg(search, what) if search is not None else self._linear_es_arg(es, what)
            step_n = getattr(self._lib, what)
            bound = lambda h, k, *rest: step_n(h, k, sr, *rest)      # (the struct goes before the outputs)
        if summary is not None:
            if out is not None:
                raise ValueError("rollout_linear: a summary launch writes no [K, N] output (out must be None)")
            if agent:
                return self._rollout_summary(bound, what, K, summary)
            return self._rollout_summary(self._lib.mdpp_step_n_linear_summary, "mdpp_step_n_linear_summary", K, summary)
        if out is None:
            out = self.alloc_rollout_linear(K)
        if agent:
            return self._rollout_closed(bound, what, K, out)
        return self._rollout_closed(self._lib.mdpp_step_n_linear, "mdpp_step_n_linear", K, out)

    def linear_kernel_name(self, K, summary=False, search=False, es=False):
        """Name (with template arguments) of the kernel rollout_linear(K) launches (mdpp_linear_kernel_name, with ``search``
        mdpp_linear_search_kernel_name, with ``es`` mdpp_linear_es_kernel_name; nothing is launched); empty for a handle it
        does not serve or without a policy."""
        if self.kind != "continuous":
            return ""
        if search and es:
            raise ValueError("linear_kernel_name: search and es are exclusive")
        fn = (self._lib.mdpp_linear_search_kernel_name if search else self._lib.mdpp_linear_es_kernel_name if es
              else self._lib.mdpp_linear_kernel_name)
        name = fn(self._h, int(K), int(bool(summary)))
        return name.decode() if name else ""

    # ------------------------------------------------------------------ in-kernel tabular TD learners
    def _learn_check_kind(self):
        if self.kind != "discrete":
            raise NotImplementedError("learner rollouts serve discrete envs only (this env is %s)" % self.kind)

    def _learn_q_shape(self, algo=None):
        S, A = self.mdps[0].S, self.mdps[0].A
        return (self.num_envs, 2, S, A) if (algo or self._learn_algo) == "double_q" else (self.num_envs, S, A)

    def _learn_q_arg(self, q, what, algo=None):
        shape = self._learn_q_shape(algo)
        if not (torch.is_tensor(q) and q.dtype == torch.float32 and q.device == self.device and tuple(q.shape) == shape):
            raise ValueError(f"{what}: q must be a float32 tensor of shape {shape} on {self.device}")
        return q.contiguous()

    def _learn_send_arrays(self, alpha, gamma, epsilon):
        """per-env parameters (validated float32 arrays, or None) -> mdpp_set_learner_params"""
        if alpha is None and gamma is None and epsilon is None:
            return
        rc = self._lib.mdpp_set_learner_params(self._h, capi.nptr(alpha), capi.nptr(gamma), capi.nptr(epsilon), self._stream())
        self._closed_call(rc, "mdpp_set_learner_params")

    def set_learner(self, algo="q_learning", *, alpha=None, gamma=None, epsilon=None, seed=0, q=None, per_env_mdp=False):
        """The handle's tabular TD learner for rollout_learn(): one independent agent PER ENV, ``algo`` "q_learning", "sarsa" or
        "double_q", float32 ``alpha`` in (0, 1], ``gamma`` and ``epsilon`` in [0, 1] -- each a scalar (uniform) or a 1-D array of
        num_envs entries (numpy, or a torch tensor on any device; env i of THIS handle learns with entry i), ``seed`` the 64-bit
        key of the learner's own Philox streams, ``q`` the initial tables (float32 [N, S, A] on the device, [N, 2, S, A] -- A
        then B -- for "double_q"; zeros when None).  ``set_learner(None)`` clears the learner.  Handles the kernel does not
        serve raise NotImplementedError with the reason (include/mdpp.h: the rule).
        ``per_env_mdp=True`` on a handle built with ``seeds=[...]`` or ``mdps=[...]``: every agent learns on its OWN env's
        MDP -- a seed sweep in one launch; rollout_learn, rollout_eval, their summary= forms, get_q / set_q
        and set_learner_rates then serve the handle, set_policy and set_noise_levels still refuse it.  Without it such a
        handle is refused as ever -- also while a per_env_mdp learner is in force: that refused call leaves learner and tables as
        they are (``set_learner(None)`` is how to drop them).  A call the library refuses leaves the opt-in as it was.
        ValueError on a handle with one shared MDP; ``set_learner(None)`` clears it too.
        Every successful call, ``set_learner(None)`` included, also drops a schedule (set_learner_schedule) and its counters."""
        if algo is None:
            capi.check(self._lib, self._h, self._lib.mdpp_clear_learner(self._h), "mdpp_clear_learner")
            capi.check(self._lib, self._h, self._lib.mdpp_learner_per_env_mdp(self._h, 0), "mdpp_learner_per_env_mdp")
            self._learn_rates = None
            self._learn_pm = False
            self._learn_sched = None
            self._drop_noise_levels_per_env_mdp()
            RLToyVectorEnv._drop_traces_per_env_mdp(self)
            return
        if alpha is None or gamma is None or epsilon is None:
            raise ValueError("set_learner: alpha, gamma and epsilon are required")
        policy_mod.check_learner_params(algo, alpha, gamma, epsilon, self.num_envs)
        arrays = [policy_mod.learner_param_array(n, v, self.num_envs) for n, v in (("alpha", alpha), ("gamma", gamma), ("epsilon", epsilon))]
        if per_env_mdp and not self._per_env:
            raise ValueError("set_learner: per_env_mdp=True needs one MDP per env (seeds=[...] or mdps=[...]); this handle has one shared MDP")
        self._learn_check_kind()
        if q is not None:
            q = self._learn_q_arg(q, "set_learner", algo)
        if self._learn_pm and not per_env_mdp:
            # (the call without the opt-in, refused as on a handle that never had it -- before the handle is touched)
            raise NotImplementedError("mdpp_set_learner: learner rollouts need one shared MDP (this handle has one MDP per env: "
                                      "seeds=[...]); the per_env_mdp=True learner in force stays as it is")
        if per_env_mdp and not self._learn_pm:
            capi.check(self._lib, self._h, self._lib.mdpp_learner_per_env_mdp(self._h, 1), "mdpp_learner_per_env_mdp")
        # (a per-env parameter's scalar slot: any valid value -- the kernel's PE form does not read it)
        scalars = [float(v) if a is None else float(a[0]) for v, a in zip((alpha, gamma, epsilon), arrays)]
        code = dict(capi.LEARN_ALGOS, double_q=capi.MDPP_LEARN_DOUBLE_Q)[algo]
        rc = self._lib.mdpp_set_learner(self._h, code, *scalars, C.c_uint64(int(seed) & (2 ** 64 - 1)),
                                        C.c_void_p(q.data_ptr()) if q is not None else None, self._stream())
        if rc == capi.EUNSUPPORTED and per_env_mdp and not self._learn_pm:
            # (refused for another reason: the opt-in goes back to what it was.  Read the reason first: the flag call keeps it)
            msg = self._lib.mdpp_last_error(self._h)
            capi.check(self._lib, self._h, self._lib.mdpp_learner_per_env_mdp(self._h, 0), "mdpp_learner_per_env_mdp")
            raise NotImplementedError(msg.decode() if msg else "mdpp_set_learner: unsupported")
        self._closed_call(rc, "mdpp_set_learner")
        RLToyVectorEnv._drop_traces_per_env_mdp(self)      # (mdpp_set_learner has dropped the traces: their opt-in ends with them)
        self._learn_pm = bool(per_env_mdp)
        self._learn_sched = None         # (mdpp_set_learner drops the schedule and its counters)
        self._learn_q_init = q           # (kept until the copy queued on the stream has certainly been made)
        self._learn_rates = [scalars[0], scalars[2]]
        self._learn_algo = algo
        self._learn_pe = dict(zip(("alpha", "gamma", "epsilon"), arrays))     # the per-env arrays in force (None: uniform)
        self._learn_send_arrays(*arrays)

    def set_learner_rates(self, alpha=None, epsilon=None, *, gamma=None):
        """New alpha, epsilon and / or gamma for the learner, each a scalar (uniform from now on) or a per-env array as in
        set_learner (scalars: parameters only, no device work; arrays: one small copy on the current stream).  A new value
        holds from the next LAUNCH on, for every env alike: rates that follow each env's own episode count are
        set_learner_schedule's.  While a schedule is in force the parameter it schedules is refused here (MdppError;
        clear_learner_schedule() first) and what is in force stays; the other one and gamma are set as ever (a scalar for the
        other one travels as an array of equal entries: the library's scalar call carries both parameters)."""
        policy_mod.check_learner_params(None, alpha, gamma, epsilon, self.num_envs)
        if self._learn_rates is None:
            raise capi.MdppError("set_learner_rates: no learner set (set_learner)")
        if self._learn_sched is not None:
            for n, v in (("alpha", alpha), ("epsilon", epsilon)):
                if v is not None and self._learn_sched[n] is not None:
                    raise capi.MdppError(f"set_learner_rates: {n} follows the schedule in force; clear_learner_schedule() "
                                         "(mdpp_clear_learner_schedule) first")
            # (mdpp_set_learner_rates carries both parameters and is refused under a schedule: the free one goes out as an array)
            if alpha is not None and not policy_mod._is_array(alpha):
                alpha = np.full(self.num_envs, alpha, np.float32)
            if epsilon is not None and not policy_mod._is_array(epsilon):
                epsilon = np.full(self.num_envs, epsilon, np.float32)
        given = {"alpha": alpha, "gamma": gamma, "epsilon": epsilon}
        arrays = {n: policy_mod.learner_param_array(n, v, self.num_envs) for n, v in given.items()}
        scalar = {n: v is not None and arrays[n] is None for n, v in given.items()}
        for n, v in given.items():
            if v is not None:
                self._learn_pe[n] = arrays[n]
        if scalar["alpha"]:
            self._learn_rates[0] = float(alpha)
        if scalar["epsilon"]:
            self._learn_rates[1] = float(epsilon)
        if scalar["alpha"] or scalar["epsilon"]:
            # (mdpp_set_learner_rates makes BOTH uniform: the one of the two that stays per-env goes out again below)
            self._closed_call(self._lib.mdpp_set_learner_rates(self._h, *self._learn_rates), "mdpp_set_learner_rates")
            arrays["alpha"], arrays["epsilon"] = self._learn_pe["alpha"], self._learn_pe["epsilon"]
        if scalar["gamma"]:
            self._closed_call(self._lib.mdpp_set_learner_gamma(self._h, float(gamma)), "mdpp_set_learner_gamma")
        self._learn_send_arrays(arrays["alpha"], arrays["gamma"], arrays["epsilon"])

    # ------------------------------------------------------------------ eligibility traces: SARSA(lambda) and Q(lambda)
    def _drop_traces_per_env_mdp(self):
        # (the traces are gone: the opt-in of set_learner_traces(per_env_mdp=True) goes with them.  set_learner calls this unbound
        #  and the flag is read with a default: an object that carries the learner's attributes alone never had the opt-in)
        if getattr(self, "_trace_pm", False):
            capi.check(self._lib, self._h, self._lib.mdpp_learner_traces_per_env_mdp(self._h, 0), "mdpp_learner_traces_per_env_mdp")
            self._trace_pm = False

    def set_learner_traces(self, lam, kind="replacing", per_env_mdp=False):
        """Eligibility traces for the "q_learning" / "sarsa" learner in force (include/mdpp.h "Eligibility
        traces"): rollout_learn then runs Watkins's Q(lambda) / SARSA(lambda) -- a second table Z [S, A] per env beside Q,
        zeros after this call; every step cuts (q_learning, on an exploring step), marks (``kind`` "accumulating": Z[s, a] += 1;
        "replacing": Z[s, a] = 1), sweeps Q += alpha (y - Q[s, a]) Z, Z *= gamma lambda over the whole table, and zeroes Z
        where an episode ends.  ``lam`` is a float32 scalar in [0, 1] or a 1-D array of num_envs entries (numpy, or a torch
        tensor on any device; env i of THIS handle learns with entry i): a lambda sweep in one launch.  Z crosses launches
        and graph replays like Q; rollout_eval neither reads nor writes it; set_q leaves it alone; set_learner drops the
        traces.  rollout_learn (summary= and log= too), learn_kernel_name, set_learner_rates and set_learner_schedule serve
        the handle as it stands.  NotImplementedError, nothing changed, for "double_q", per-env noise levels, a per_env_mdp
        learner and a sweep=True schedule (not built) -- and for turning any of those on while traces are set.
        ``per_env_mdp=True`` on a handle built with ``seeds=[...]`` or ``mdps=[...]`` whose learner was set with
        ``per_env_mdp=True``: the traces are accepted on one MDP per env, and together with a ``sweep=True``
        schedule there, in either order -- a lambda x seed sweep with per-episode decay in ONE launch; env i learns bit for bit
        like env i of a shared-MDP handle built on its seed.  get_traces / set_traces, set_learner_rates, per-env ``lam``,
        summary= and log=, rollout_eval and learn_kernel_name ("...,PE=1,PM=1|2[,SCHED=1]>") serve the handle unchanged;
        "double_q", per-env noise levels and a sweep=True schedule on a shared MDP stay refused.  ValueError on a handle with
        one shared MDP, before any device work; a one-MDP-per-env handle whose learner lacks per_env_mdp=True raises the
        learner's refusal.  While such traces are in force a call without ``per_env_mdp=True`` is refused
        (NotImplementedError) and what is in force stays; a call the library refuses leaves the opt-in as it was.  The opt-in
        ends with clear_learner_traces() and set_learner(...)."""
        if per_env_mdp and not self._per_env:
            raise ValueError("set_learner_traces: per_env_mdp=True needs one MDP per env (seeds=[...] or mdps=[...]); this handle has one shared MDP")
        self._learn_check_kind()
        if kind not in capi.TRACE_KINDS:
            raise ValueError(f"set_learner_traces: kind must be one of {sorted(capi.TRACE_KINDS)}, got {kind!r}")
        arr = policy_mod.learner_param_array("lam", lam, self.num_envs)
        if arr is None and not 0.0 <= float(np.float32(lam)) <= 1.0:
            raise ValueError(f"lam must lie in [0, 1], got {lam!r}")
        want_pm = bool(per_env_mdp) and self._per_env
        if want_pm and not self._learn_pm:
            # (no learner can be in force here: set_learner refuses this handle without its own opt-in, in these words)
            raise NotImplementedError("mdpp_set_learner_traces: learner rollouts need one shared MDP (this handle has one MDP per env: "
                                      "seeds=[...]); set_learner(..., per_env_mdp=True) first")
        if self._learn_rates is None:
            raise capi.MdppError("set_learner_traces: no learner set (set_learner)")
        scalar = float(lam) if arr is None else float(arr[0])
        if self._trace_pm and not want_pm:
            # (the call without the opt-in, refused as on a handle that never had it -- before the handle is touched)
            raise NotImplementedError("mdpp_set_learner_traces: eligibility traces with one MDP per env: not built; the per_env_mdp=True "
                                      "traces in force stay as they are")
        flipped = want_pm and not self._trace_pm
        if flipped:
            capi.check(self._lib, self._h, self._lib.mdpp_learner_traces_per_env_mdp(self._h, 1), "mdpp_learner_traces_per_env_mdp")
        rc = self._lib.mdpp_set_learner_traces(self._h, capi.TRACE_KINDS[kind], C.c_float(scalar), self._stream())
        if rc != 0 and flipped:
            # (the opt-in goes back to what it was.  Read the reason first: the flag call keeps it)
            msg = self._lib.mdpp_last_error(self._h)
            capi.check(self._lib, self._h, self._lib.mdpp_learner_traces_per_env_mdp(self._h, 0), "mdpp_learner_traces_per_env_mdp")
            if rc == capi.EUNSUPPORTED:
                raise NotImplementedError(msg.decode() if msg else "mdpp_set_learner_traces: unsupported")
            raise capi.MdppError("mdpp_set_learner_traces failed (%d): %s" % (rc, msg.decode() if msg else ""))
        self._closed_call(rc, "mdpp_set_learner_traces")
        self._trace_pm = want_pm
        if arr is not None:
            self._closed_call(self._lib.mdpp_set_learner_lambda(self._h, capi.nptr(arr), self._stream()), "mdpp_set_learner_lambda")

    def clear_learner_traces(self):
        """Drop the traces: rollout_learn is the one-step learner again (Q stays as it is).  The ``per_env_mdp=True`` opt-in of
        set_learner_traces goes with them."""
        capi.check(self._lib, self._h, self._lib.mdpp_clear_learner_traces(self._h), "mdpp_clear_learner_traces")
        self._drop_traces_per_env_mdp()

    @property
    def learner_traces(self):
        """None, "accumulating" or "replacing": the traces in force (set_learner_traces)."""
        if self.kind != "discrete":
            return None
        code = self._lib.mdpp_learner_traces(self._h)
        return {v: k for k, v in capi.TRACE_KINDS.items()}.get(code)

    def _trace_shape(self):
        return (self.num_envs, self.mdps[0].S, self.mdps[0].A)

    def get_traces(self):
        """The traces Z, float32 [N, S, A]; a copy, made on the current stream."""
        self._learn_check_kind()
        z = torch.empty(self._trace_shape(), dtype=torch.float32, device=self.device)
        self._closed_call(self._lib.mdpp_get_traces(self._h, C.c_void_p(z.data_ptr()), self._stream()), "mdpp_get_traces")
        return z

    def set_traces(self, z):
        """Replace the traces: float32 [N, S, A] on the device (copied on the current stream)."""
        self._learn_check_kind()
        shape = self._trace_shape()
        if not (torch.is_tensor(z) and z.dtype == torch.float32 and z.device == self.device and tuple(z.shape) == shape):
            raise ValueError(f"set_traces: z must be a float32 tensor of shape {shape} on {self.device}")
        z = z.contiguous()
        self._closed_call(self._lib.mdpp_set_traces(self._h, C.c_void_p(z.data_ptr()), self._stream()), "mdpp_set_traces")
        self._learn_z_init = z           # (kept until the copy queued on the stream has certainly been made)

    # ------------------------------------------------------------------ per-episode epsilon / alpha schedules
    def set_learner_schedule(self, epsilon=None, alpha=None, row=None, sweep=False):
        """Per-EPISODE epsilon and / or alpha for rollout_learn.  ``epsilon`` and ``alpha`` are tables [M] or
        [R, M] (numpy, or a torch tensor on any device; epsilon in [0, 1], alpha as float32 in (0, 1]; R M <= 2^22), ``row`` an
        integer array [N] in [0, R) -- the table row env i of THIS handle follows (its local index, like the per-env
        parameters); required iff R > 1.  The kernel keeps an int32 episode counter per env, zero after this call: the env
        learns with entry min(counter, M - 1) of its row, and the counter moves, after the update, at every step that is
        ``terminated or truncated`` and is not the reset call of a next-step-autoreset env -- the rule by which
        summary.episodes moves -- so the envs of one launch each follow their own episode count.  Past M - 1 the last entry
        holds.  A parameter without a table stays what set_learner / set_learner_rates made it.  policy.epsilon_decay makes
        the rows "linear", "log" and "const".  rollout_eval reads no table and moves no counter.
        ValueError (policy.learner_schedule_arrays) before any device work; MdppError without a learner;
        NotImplementedError, nothing changed, on a handle with per-env noise levels or a per_env_mdp learner (not built)
        unless ``sweep=True``.  set_learner drops the schedule; while it is in force set_noise_levels is refused, again
        unless the schedule was set with ``sweep=True``.
        ``sweep=True``: the schedule is also served on a handle with per-env noise levels
        (set_noise_levels), with a per_env_mdp learner, or with both -- the same learner, step and placements as without a
        schedule, with E and alpha taken from (row[i], counter[i]) by the rules above -- so an agent with a decay schedule
        trains over noise levels x seeds in ONE launch.  Schedule and levels may be given in either order; on a plain
        shared-MDP handle without levels ``sweep=True`` changes nothing.  The opt-in stays until clear_learner_schedule().
        While a sweep schedule is in force together with levels or a per_env_mdp learner, a call without ``sweep=True`` is
        refused (NotImplementedError) and what is in force stays; a call the library refuses leaves the opt-in as it was.
        Like noise levels the schedule is
        configuration, and its counters are the learner's, not the env's: get_augmented_state / set_augmented_state carry
        neither -- a checkpoint keeps learner_episodes() beside get_q() and gives both back (set_learner_episodes, set_q).
        With eligibility traces: a plain schedule is served on a shared MDP, a ``sweep=True`` one on a per_env_mdp learner whose
        traces were set with ``per_env_mdp=True``, in either order; a ``sweep=True`` schedule with traces on a
        shared MDP is refused."""
        eps, al, rows, R, M = policy_mod.learner_schedule_arrays(epsilon, alpha, row, self.num_envs)
        self._learn_check_kind()
        sweep = bool(sweep)
        if self._sched_sweep and not sweep and self._learn_sched is not None and (self._noise_levels_set or self._learn_pm):
            # (the call without the opt-in, refused as on a handle that never had it -- before the handle is touched)
            raise NotImplementedError("mdpp_set_learner_schedule: an epsilon/alpha schedule with per-env noise levels / one MDP per env: "
                                      "not built; the sweep=True schedule in force stays as it is")
        was = self._sched_sweep
        if sweep != was:
            # (refused while eligibility traces are set on a shared MDP -- not built: NotImplementedError, nothing changed; with
            #  set_learner_traces(..., per_env_mdp=True) traces it is accepted)
            self._closed_call(self._lib.mdpp_learner_schedule_sweep(self._h, int(sweep)), "mdpp_learner_schedule_sweep")
            self._sched_sweep = sweep
        rc = self._lib.mdpp_set_learner_schedule(self._h, capi.nptr(eps), capi.nptr(al), R, M, capi.nptr(rows), self._stream())
        if rc != 0 and sweep and not was:
            # (the opt-in goes back to what it was.  Read the reason first: the flag call keeps it)
            msg = self._lib.mdpp_last_error(self._h)
            capi.check(self._lib, self._h, self._lib.mdpp_learner_schedule_sweep(self._h, 0), "mdpp_learner_schedule_sweep")
            self._sched_sweep = False
            if rc == capi.EUNSUPPORTED:
                raise NotImplementedError(msg.decode() if msg else "mdpp_set_learner_schedule: unsupported")
            raise capi.MdppError("mdpp_set_learner_schedule failed (%d): %s" % (rc, msg.decode() if msg else ""))
        self._closed_call(rc, "mdpp_set_learner_schedule")
        self._learn_sched = dict(epsilon=eps, alpha=al, row=rows)

    def clear_learner_schedule(self):
        """Drop the schedule: epsilon and alpha are again what set_learner / set_learner_rates made them (the scheduled
        parameter's last uniform or per-env value).  The counters are zeroed by the next set_learner_schedule.  The
        ``sweep=True`` opt-in of set_learner_schedule goes with it."""
        capi.check(self._lib, self._h, self._lib.mdpp_clear_learner_schedule(self._h), "mdpp_clear_learner_schedule")
        if self._sched_sweep:
            capi.check(self._lib, self._h, self._lib.mdpp_learner_schedule_sweep(self._h, 0), "mdpp_learner_schedule_sweep")
            self._sched_sweep = False
        self._learn_sched = None

    def learner_schedule(self):
        """The schedule in force -- dict(epsilon=float32 [R, M] or None, alpha=likewise, row=int32 [N] or None), copies -- or
        None."""
        if self._learn_sched is None:
            return None
        return {k: None if v is None else v.copy() for k, v in self._learn_sched.items()}

    def learner_episodes(self):
        """The schedule's per-env episode counters, int32 [N] on the device; a copy, made on the current stream."""
        self._learn_check_kind()
        ep = torch.empty(self.num_envs, dtype=torch.int32, device=self.device)
        self._closed_call(self._lib.mdpp_get_learner_episodes(self._h, C.c_void_p(ep.data_ptr()), self._stream()), "mdpp_get_learner_episodes")
        return ep

    def set_learner_episodes(self, x=None):
        """Replace the schedule's counters: an integer array [N] of values >= 0 (numpy, or a torch tensor on any device), or
        None for zeros -- the schedule starts again.  Copied on the current stream."""
        self._learn_check_kind()
        ep = None
        if x is not None:
            a = policy_mod._to_numpy(x)
            if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer) or a.shape != (self.num_envs,):
                raise ValueError(f"set_learner_episodes: need an integer array of shape ({self.num_envs},), got {a.dtype} {a.shape}")
            if a.size and (a.min() < 0 or a.max() > 2 ** 31 - 1):
                raise ValueError("set_learner_episodes: every counter must lie in [0, 2^31)")
            ep = torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).to(self.device)
        rc = self._lib.mdpp_set_learner_episodes(self._h, C.c_void_p(ep.data_ptr()) if ep is not None else None, self._stream())
        self._closed_call(rc, "mdpp_set_learner_episodes")
        self._learn_ep_init = ep         # (kept until the copy queued on the stream has certainly been made)

    def alloc_rollout_learn(self, K):
        """Output buffers of rollout_learn(K): alloc_rollout(K) and the actions, int32 [K, N]."""
        return self._alloc_rollout_closed(K)

    def rollout_learn(self, K, out=None, *, summary=None, log=None):
        """K steps of "select epsilon-greedily from the env's own Q, step, update that Q" in ONE kernel launch.  Returns (obs,
        reward, terminated, truncated, actions), each with a leading K axis; rollout(actions) on an identically built env
        returns the same first four, bit for bit.  SARSA carries its next action from step to step inside a call only: the
        first step of every call selects afresh.  With a schedule (set_learner_schedule) every env selects and
        updates with the epsilon / alpha of its own episode count, looked up again inside the launch at each episode end.
        ``summary`` (episode_summary()): the same K steps with the same effect on the env and the tables, but NO [K, N] array
        is written -- the kernel keeps the per-env episode numbers in ``summary`` and that object is returned.
        ``log`` (episode_log(M), with ``summary`` only): the same launch also writes the return and length of every episode that
        ends into the log, at the env's own episode index; ``summary`` is still what is returned."""
        self._learn_check_kind()
        if log is not None and (summary is None or out is not None):
            raise ValueError("rollout_learn: log goes with summary (and without out)")
        if summary is not None:
            if out is not None:
                raise ValueError("rollout_learn: give out or summary, not both")
            if log is not None:
                return self._rollout_summary(self._lib.mdpp_step_n_learn_log, "mdpp_step_n_learn_log", int(K), summary, log)
            return self._rollout_summary(self._lib.mdpp_step_n_learn_summary, "mdpp_step_n_learn_summary", int(K), summary)
        return self._rollout_closed(self._lib.mdpp_step_n_learn, "mdpp_step_n_learn", int(K), out)

    def alloc_rollout_eval(self, K):
        """Output buffers of rollout_eval(K): alloc_rollout(K) and the actions, int32 [K, N]."""
        return self._alloc_rollout_closed(K)

    def rollout_eval(self, K, out=None, *, summary=None):
        """K steps of GREEDY evaluation of the learner's tables in ONE kernel launch: every env takes the lowest action that
        maximises its own Q[s] (QA[s] + QB[s] for "double_q").  No exploration and no update: the tables stay bit for bit what
        they were, the learner's Philox streams are not consumed, alpha, gamma and epsilon are not read.  Needs a learner
        (set_learner, any algorithm).  Returns (obs, reward, terminated, truncated, actions) like rollout_learn; with
        ``summary`` the episode numbers instead, as there (an episode log is kept by rollout_learn only: DESIGN.md 3.24).  The steps are steps of THIS env: to evaluate on a separate one,
        build a second handle and give it the tables -- set_learner(..., q=train.get_q()) or set_q(train.get_q())."""
        self._learn_check_kind()
        if summary is not None:
            if out is not None:
                raise ValueError("rollout_eval: give out or summary, not both")
            return self._rollout_summary(self._lib.mdpp_step_n_eval_summary, "mdpp_step_n_eval_summary", int(K), summary)
        return self._rollout_closed(self._lib.mdpp_step_n_eval, "mdpp_step_n_eval", int(K), out)

    def eval_kernel_name(self, K):
        """Name (with template arguments) of the kernel rollout_eval(K) launches (mdpp_eval_kernel_name; nothing is launched;
        QLDS=1: the Q-tables are staged in LDS; DOUBLE=1: two tables per env; NLEV=1: per-env noise levels); empty for a handle
        it does not serve or one without a learner."""
        if self.kind != "discrete":
            return ""
        name = self._lib.mdpp_eval_kernel_name(self._h, int(K))
        return name.decode() if name else ""

    def get_q(self):
        """The learner's tables, float32 [N, S, A] ([N, 2, S, A], A then B, for "double_q"); a copy, made on the current stream."""
        self._learn_check_kind()
        q = torch.empty(self._learn_q_shape(), dtype=torch.float32, device=self.device)
        self._closed_call(self._lib.mdpp_get_q(self._h, C.c_void_p(q.data_ptr()), self._stream()), "mdpp_get_q")
        return q

    def set_q(self, q):
        """Replace the learner's tables: float32 [N, S, A] ([N, 2, S, A] for "double_q") on the device (copied on the current
        stream)."""
        self._learn_check_kind()
        q = self._learn_q_arg(q, "set_q")
        self._closed_call(self._lib.mdpp_set_q(self._h, C.c_void_p(q.data_ptr()), self._stream()), "mdpp_set_q")
        self._learn_q_init = q

    def learn_kernel_name(self, K):
        """Name (with template arguments) of the kernel rollout_learn(K) launches (mdpp_learn_kernel_name; nothing is
        launched; QLDS=1: the Q-tables are staged in LDS; PE=1: per-env parameters; DOUBLE=1: double Q-learning; NLEV=1: per-env
        noise levels, set_noise_levels; with set_learner_traces the kernel is k_discrete_trace_rollout / _summary<PHILOX, NOISE, UNIT,
        QLDS[, PE=1][, PM=1|2][, SCHED=1]>, QLDS=1: Q and Z are both staged in LDS; SCHED=1, always last: a per-episode schedule, set_learner_schedule; PM=2 / PM=1: one MDP per env, staged in LDS / read in global memory; NLEV=1 with PM:
        per-env noise levels on one MDP per env, set_noise_levels(..., per_env_mdp=True) -- the arguments come in template order,
        "...,PE=1[,DOUBLE=1],NLEV=1,PM=1|2>", and a set_learner_schedule(..., sweep=True) schedule on any of these appends
        ",SCHED=1" after everything else: "...,NLEV=1,PM=2,SCHED=1>"); empty for a handle it does not serve."""
        if self.kind != "discrete":
            return ""
        name = self._lib.mdpp_learn_kernel_name(self._h, int(K))
        return name.decode() if name else ""

    # ------------------------------------------------------------------ in-kernel tabular TD learners on grid envs
    def _grid_learn_check_kind(self):
        if self.kind != "grid":
            raise NotImplementedError("grid learners serve grid envs only (this env is %s)" % self.kind)

    def _grid_q_shape(self, n_actions=None):
        g = self.mdps[0].grid_shape
        return (self.num_envs, int(g[0]) + 1, int(g[1]) + 1, int(n_actions or self._grid_learn_A))

    def _grid_q_arg(self, q, what, n_actions=None):
        shape = self._grid_q_shape(n_actions)
        if not (torch.is_tensor(q) and q.dtype == torch.float32 and q.device == self.device and tuple(q.shape) == shape):
            raise ValueError(f"{what}: q must be a float32 tensor of shape {shape} on {self.device}")
        return q.contiguous()

    def _grid_param_arrays(self, alpha, gamma, epsilon):
        """float32 [N] per parameter (a scalar is broadcast), or None for None, after policy.check_learner_params"""
        policy_mod.check_learner_params(None, alpha, gamma, epsilon, self.num_envs)
        out = []
        for name, v in (("alpha", alpha), ("gamma", gamma), ("epsilon", epsilon)):
            a = policy_mod.learner_param_array(name, v, self.num_envs)
            out.append(a if a is not None or v is None else np.full(self.num_envs, np.float32(v), np.float32))
        return out

    def set_grid_learner(self, algo="q_learning", *, alpha=None, gamma=None, epsilon=None, seed=0, q=None, noop=False):
        """The tabular TD learner of a GRID handle for rollout_grid_learn(): one independent agent PER GRIDWORLD, ``algo``
        "q_learning" or "sarsa", float32 ``alpha`` in (0, 1], ``gamma`` and ``epsilon`` in [0, 1] -- each a scalar (broadcast) or a
        1-D array of num_envs entries (env i of THIS handle learns with entry i) --, ``seed`` the 64-bit key of the learner's own
        Philox streams, ``q`` the initial tables (float32 [N, g0 + 1, g1 + 1, A] on the device; zeros when None).  The agent's
        actions are (+1,0), (-1,0), (0,+1), (0,-1) and, with ``noop=True``, (0,0): A = 4 or 5.  The state of cell (c0, c1) is the
        table's row [c0, c1]; row g, one past the grid, is an episode's possible first cell (include/mdpp.h "Grid learners").
        ``set_grid_learner(None)`` clears the learner.  Handles the kernel does not serve raise NotImplementedError with the
        reason."""
        if algo is None:
            capi.check(self._lib, self._h, self._lib.mdpp_clear_grid_learner(self._h), "mdpp_clear_grid_learner")
            self._grid_sched = None
            return
        if alpha is None or gamma is None or epsilon is None:
            raise ValueError("set_grid_learner: alpha, gamma and epsilon are required")
        if algo not in capi.LEARN_ALGOS:
            raise ValueError(f"set_grid_learner: algo must be one of {tuple(capi.LEARN_ALGOS)}, got {algo!r}")
        arrays = self._grid_param_arrays(alpha, gamma, epsilon)
        self._grid_learn_check_kind()
        A = 5 if noop else 4
        if q is not None and len(self.mdps[0].grid_shape) == 2:
            q = self._grid_q_arg(q, "set_grid_learner", A)
        rc = self._lib.mdpp_set_grid_learner(self._h, capi.LEARN_ALGOS[algo], A, C.c_uint64(int(seed) & (2 ** 64 - 1)),
                                             *(capi.nptr(a) for a in arrays),
                                             C.c_void_p(q.data_ptr()) if q is not None else None, self._stream())
        self._closed_call(rc, "mdpp_set_grid_learner")
        self._grid_learn_A = A
        self._grid_sched = None          # (mdpp_set_grid_learner drops the schedule and its counters)
        self._grid_q_init = q            # (kept until the copy queued on the stream has certainly been made)

    def set_grid_learner_rates(self, alpha=None, gamma=None, epsilon=None):
        """New alpha, gamma and / or epsilon for the grid learner, each a scalar (broadcast) or a per-env array as in
        set_grid_learner; None keeps the current values.  One small copy per parameter on the current stream; the new values
        hold from the next launch on.  While a schedule is in force (set_grid_learner_schedule) the parameter it schedules is
        refused (MdppError, nothing changed; clear_grid_learner_schedule() first); gamma is always accepted."""
        arrays = self._grid_param_arrays(alpha, gamma, epsilon)
        self._grid_learn_check_kind()
        rc = self._lib.mdpp_set_grid_learner_params(self._h, *(capi.nptr(a) for a in arrays), self._stream())
        self._closed_call(rc, "mdpp_set_grid_learner_params")

    def alloc_rollout_grid(self, K):
        """Output buffers of rollout_grid_learn(K) / rollout_grid_eval(K): alloc_rollout(K) and the action vectors, int32 [K, N, 2]."""
        return self.alloc_rollout(K) + (torch.empty((K, self.num_envs, 2), dtype=torch.int32, device=self.device),)

    def _rollout_grid(self, stem, K, out, summary, log=None):
        self._grid_learn_check_kind()
        K = int(K)
        if log is not None and (summary is None or out is not None):
            raise ValueError("rollout_grid_learn: log goes with summary (and without out)")
        if summary is not None:
            if out is not None:
                raise ValueError("a summary launch writes no [K, N] output (out must be None)")
            if log is not None:
                return self._rollout_summary(getattr(self._lib, stem + "_log"), stem + "_log", K, summary, log)
            return self._rollout_summary(getattr(self._lib, stem + "_summary"), stem + "_summary", K, summary)
        if out is None:
            out = self.alloc_rollout_grid(K)
        return self._rollout_closed(getattr(self._lib, stem), stem, K, out)

    def rollout_grid_learn(self, K, out=None, *, summary=None, log=None):
        """K steps of "select epsilon-greedily from the gridworld's own Q, move, update that Q" in ONE kernel launch.  Returns
        (obs, reward, terminated, truncated, actions), each with a leading K axis, ``actions`` the int32 [K, N, 2] action vectors
        taken: rollout(actions) on an identically built env returns the same first four, bit for bit.  SARSA carries its next
        action from step to step inside a call only.  ``summary`` (episode_summary()): the same K steps with the same effect on
        the env and the tables, but NO [K, N] array is written -- the summary is updated and returned.  With a schedule
        (set_grid_learner_schedule) every env selects and updates with the epsilon / alpha of its own episode count, looked up
        again inside the launch at each of its episode ends.  ``log`` (episode_log(M), with ``summary`` only): the same launch
        also writes the return and length of every episode that ends into the log, at the env's own episode index
        (DESIGN.md 3.32); ``summary`` is still what is returned."""
        return self._rollout_grid("mdpp_step_n_grid_learn", K, out, summary, log)

    def rollout_grid_eval(self, K, out=None, *, summary=None):
        """K steps of GREEDY evaluation of the grid learner's tables in ONE kernel launch: every env takes the lowest action that
        maximises its own Q[s].  Nothing is drawn, nothing is updated: the tables stay bit for bit what they were.  Returns as
        rollout_grid_learn; with ``summary`` the episode numbers instead."""
        return self._rollout_grid("mdpp_step_n_grid_eval", K, out, summary)

    # ---- per-episode epsilon / alpha schedules of the grid learner
    def set_grid_learner_schedule(self, epsilon=None, alpha=None, row=None):
        """Per-EPISODE epsilon and / or alpha for rollout_grid_learn (include/mdpp.h "Grid learner schedules and
        the episode log").  ``epsilon`` and ``alpha`` are tables [M] or [R, M] (numpy, or a torch tensor on any device; epsilon
        in [0, 1], alpha as float32 in (0, 1]; R M <= 2^22), ``row`` an integer array [N] in [0, R) -- the table row env i of
        THIS handle follows; required iff R > 1.  The kernel keeps an int32 episode counter per env, zero after this call: the
        env learns with entry min(counter, M - 1) of its row, and the counter moves, after the update, at every step that is
        ``terminated or truncated`` and is not the reset call of a next-step-autoreset env -- the rule by which
        summary.episodes moves.  Past M - 1 the last entry holds.  A parameter without a table stays what set_grid_learner /
        set_grid_learner_rates made it; gamma is never scheduled.  policy.epsilon_decay makes the rows "linear", "log" and
        "const".  rollout_grid_eval reads no table and moves no counter.  ValueError (policy.learner_schedule_arrays) before
        any device work; MdppError without a learner; set_grid_learner drops the schedule."""
        eps, al, rows, R, M = policy_mod.learner_schedule_arrays(epsilon, alpha, row, self.num_envs)
        self._grid_learn_check_kind()
        rc = self._lib.mdpp_set_grid_learner_schedule(self._h, capi.nptr(eps), capi.nptr(al), R, M, capi.nptr(rows), self._stream())
        self._closed_call(rc, "mdpp_set_grid_learner_schedule")
        self._grid_sched = dict(epsilon=eps, alpha=al, row=rows)

    def clear_grid_learner_schedule(self):
        """Drop the grid learner's schedule: epsilon and alpha are again what set_grid_learner / set_grid_learner_rates made
        them.  The counters are zeroed by the next set_grid_learner_schedule."""
        self._grid_learn_check_kind()
        self._closed_call(self._lib.mdpp_clear_grid_learner_schedule(self._h), "mdpp_clear_grid_learner_schedule")
        self._grid_sched = None

    def grid_learner_schedule(self):
        """The grid learner's schedule in force -- dict(epsilon=float32 [R, M] or None, alpha=likewise, row=int32 [N] or
        None), copies -- or None."""
        if self._grid_sched is None:
            return None
        return {k: None if v is None else v.copy() for k, v in self._grid_sched.items()}

    def grid_learner_episodes(self):
        """The grid schedule's per-env episode counters, int32 [N] on the device; a copy, made on the current stream."""
        self._grid_learn_check_kind()
        ep = torch.empty(self.num_envs, dtype=torch.int32, device=self.device)
        self._closed_call(self._lib.mdpp_get_grid_learner_episodes(self._h, C.c_void_p(ep.data_ptr()), self._stream()),
                          "mdpp_get_grid_learner_episodes")
        return ep

    def set_grid_learner_episodes(self, x=None):
        """Replace the grid schedule's counters: an integer array [N] of values >= 0 (numpy, or a torch tensor on any device),
        or None for zeros -- the schedule starts again.  Copied on the current stream."""
        self._grid_learn_check_kind()
        ep = None
        if x is not None:
            a = policy_mod._to_numpy(x)
            if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer) or a.shape != (self.num_envs,):
                raise ValueError(f"set_grid_learner_episodes: need an integer array of shape ({self.num_envs},), got {a.dtype} {a.shape}")
            if a.size and (a.min() < 0 or a.max() > 2 ** 31 - 1):
                raise ValueError("set_grid_learner_episodes: every counter must lie in [0, 2^31)")
            ep = torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).to(self.device)
        rc = self._lib.mdpp_set_grid_learner_episodes(self._h, C.c_void_p(ep.data_ptr()) if ep is not None else None, self._stream())
        self._closed_call(rc, "mdpp_set_grid_learner_episodes")
        self._grid_ep_init = ep          # (kept until the copy queued on the stream has certainly been made)

    def get_grid_q(self):
        """The grid learner's tables, float32 [N, g0 + 1, g1 + 1, A]; a copy, made on the current stream."""
        self._grid_learn_check_kind()
        if self._grid_learn_A is None:
            raise capi.MdppError("mdpp_get_grid_q failed (%d): no learner set (set_grid_learner)" % capi.ESTATE)
        q = torch.empty(self._grid_q_shape(), dtype=torch.float32, device=self.device)
        self._closed_call(self._lib.mdpp_get_grid_q(self._h, C.c_void_p(q.data_ptr()), self._stream()), "mdpp_get_grid_q")
        return q

    def set_grid_q(self, q):
        """Replace the grid learner's tables: float32 [N, g0 + 1, g1 + 1, A] on the device (copied on the current stream)."""
        self._grid_learn_check_kind()
        if self._grid_learn_A is None:
            raise capi.MdppError("mdpp_set_grid_q failed (%d): no learner set (set_grid_learner)" % capi.ESTATE)
        q = self._grid_q_arg(q, "set_grid_q")
        self._closed_call(self._lib.mdpp_set_grid_q(self._h, C.c_void_p(q.data_ptr()), self._stream()), "mdpp_set_grid_q")
        self._grid_q_init = q

    def grid_learn_kernel_name(self, K, eval=False, summary=False):
        """Name (with template arguments) of the kernel rollout_grid_learn(K) (``eval``: rollout_grid_eval(K); ``summary``: their
        summary= forms) launches (mdpp_grid_learn_kernel_name; nothing is launched; QLDS=1: the Q-tables are staged in LDS;
        ",NLEV=1" after SUMMARY= while set_grid_noise_levels is in force, then ",SCHED=1" on the learning forms while a
        schedule is in force; a log= launch reports this name too);
        empty for a handle it does not serve or one without a learner."""
        if self.kind != "grid":
            return ""
        name = self._lib.mdpp_grid_learn_kernel_name(self._h, int(K), int(bool(eval)), int(bool(summary)))
        return name.decode() if name else ""

    # ---- per-env noise levels of a grid handle
    _GRID_NOISE_LEVELS_ONLY = "grid noise levels: learner and evaluation launches only; clear_grid_noise_levels() first"

    def set_grid_noise_levels(self, transition_noise=None, reward_noise=None):
        """Per-env noise levels for rollout_grid_learn / rollout_grid_eval (their summary= and log= forms, with or without a
        schedule; include/mdpp.h "Grid noise levels"): env i of THIS handle (its local index) steps with
        ``transition_noise[i]`` in [0, 1] -- any number of distinct values -- and ``reward_noise[i]`` finite and >= 0, bit for
        bit like env i of a handle created with those two values.  Each argument is None (that key stays as it is), a scalar
        (broadcast) or a 1-D array of num_envs entries (numpy, or a torch tensor on any device; converted to float64).  The
        handle must be one set_grid_learner serves (a learner need not be set) and must have been created with the key:
        ``reward_noise`` present in the config (any value), ``transition_noise`` > 0.  A noise sweep then runs as ONE launch.
        ValueError naming the key for a bad array or a key the handle lacks, before any device work; NotImplementedError with
        the library's reason for a handle not served.  While levels are set step(), rollout() and step_graph() raise; reset()
        is unaffected.  Levels are configuration, not state: set_grid_learner, the schedule calls, set_grid_q,
        get_augmented_state / set_augmented_state neither carry nor disturb them."""
        arrays = {}
        for key, v in (("transition_noise", transition_noise), ("reward_noise", reward_noise)):
            arrays[key] = policy_mod.grid_noise_level_array(key, v, self.num_envs)
        self._grid_learn_check_kind()
        for key, a in arrays.items():
            if a is None:
                continue
            created = self.config.get(key)
            if created is None or (key == "transition_noise" and not created):
                raise ValueError("set_grid_noise_levels: %s: the handle was created without the key%s" %
                                 (key, " (it needs transition_noise > 0)" if key == "transition_noise" else ""))
        if all(a is None for a in arrays.values()):
            return
        rc = self._lib.mdpp_set_grid_noise_levels(self._h, capi.nptr(arrays["transition_noise"]), capi.nptr(arrays["reward_noise"]), self._stream())
        self._closed_call(rc, "mdpp_set_grid_noise_levels")
        self._grid_noise_levels_set = True

    def grid_noise_levels(self):
        """(transition_noise, reward_noise) in force on a grid handle, float64 numpy [N] each: what set_grid_noise_levels gave,
        else the creation values (0 for a key the config does not have)."""
        self._grid_learn_check_kind()
        tn, rn = np.empty(self.num_envs, np.float64), np.empty(self.num_envs, np.float64)
        capi.check(self._lib, self._h, self._lib.mdpp_get_grid_noise_levels(self._h, capi.nptr(tn), capi.nptr(rn)), "mdpp_get_grid_noise_levels")
        return tn, rn

    def clear_grid_noise_levels(self):
        """Back to the creation values of both keys: the handle launches the kernels it launched before set_grid_noise_levels."""
        self._grid_learn_check_kind()
        capi.check(self._lib, self._h, self._lib.mdpp_clear_grid_noise_levels(self._h), "mdpp_clear_grid_noise_levels")
        self._grid_noise_levels_set = False

    # ------------------------------------------------------------------ per-env noise levels
    _NOISE_LEVELS_ONLY = "per-env noise levels: learner and evaluation launches only; clear_noise_levels() first"

    def _noise_levels_refuse(self):
        if self._noise_levels_set:
            raise capi.MdppError(self._NOISE_LEVELS_ONLY)
        if self._grid_noise_levels_set:
            raise capi.MdppError(self._GRID_NOISE_LEVELS_ONLY)

    def _drop_noise_levels_per_env_mdp(self):
        # (the library has dropped the levels and the opt-in with the learner's per-env-MDP flag)
        if self._nl_pm:
            self._nl_pm = False
            self._noise_levels_set = False

    def set_noise_levels(self, transition_noise=None, reward_noise=None, per_env_mdp=False):
        """Per-env noise levels for rollout_learn / rollout_eval (and their summary= forms): env i of THIS handle (its local
        index, like the per-env learner parameters: a sharded run gives each shard its slice) steps with
        ``transition_noise[i]`` in [0, 1] -- at most 16 distinct values per handle -- and ``reward_noise[i]`` finite and >= 0,
        bit for bit like env i of a handle created with those two values.  Each argument is None (that key stays as it is), a
        scalar (broadcast) or a 1-D array of num_envs entries (numpy, or a torch tensor on any device; converted to float64).
        The handle must be one set_learner serves and must have been created with the key: ``reward_noise`` present in the
        config (any value), ``transition_noise`` > 0.  A noise sweep then runs as ONE launch.  ValueError for a
        bad array or a key the handle lacks, before any device work.  While levels are set step(), rollout() and step_graph()
        raise; reset() is unaffected.  Levels are configuration, not state: get_augmented_state / set_augmented_state and
        checkpoints neither carry nor disturb them -- set them again on a restored handle.
        ``per_env_mdp=True`` on a handle built with ``seeds=[...]`` or ``mdps=[...]`` whose learner was set with
        ``per_env_mdp=True``: the levels are accepted on one MDP per env -- a noise x seed sweep in ONE launch;
        env i behaves bit for bit like env i of such a handle created uniformly at its two values.  Without it that handle is
        refused as ever; the opt-in stays until clear_noise_levels(), ``set_learner(None)`` or a call without it.  ValueError
        on a handle with one shared MDP; a one-MDP-per-env handle without the per_env_mdp learner raises the learner's
        refusal.  While a schedule (set_learner_schedule) is in force the call is refused (NotImplementedError, nothing
        changed) unless the schedule was set with ``sweep=True``: then the levels are accepted and the launch is the
        scheduled learner on them."""
        if per_env_mdp and not self._per_env:
            raise ValueError("set_noise_levels: per_env_mdp=True needs one MDP per env (seeds=[...] or mdps=[...]); this handle has one shared MDP")
        arrays = {}
        for key, v in (("transition_noise", transition_noise), ("reward_noise", reward_noise)):
            arrays[key] = policy_mod.noise_level_array(key, v, self.num_envs)
        self._learn_check_kind()
        for key, a in arrays.items():
            if a is None:
                continue
            created = self.config.get(key)
            if created is None or (key == "transition_noise" and not created):
                raise ValueError("set_noise_levels: %s: the handle was created without the key%s" %
                                 (key, " (it needs transition_noise > 0)" if key == "transition_noise" else ""))
        if all(a is None for a in arrays.values()):
            return
        want_pm = bool(per_env_mdp) and self._per_env
        if self._nl_pm and not want_pm:
            # (the call without the opt-in, refused as on a handle that never had it -- before the handle is touched)
            raise NotImplementedError("mdpp_set_noise_levels: per-env noise levels on one MDP per env: not built; the per_env_mdp=True "
                                      "levels in force stay as they are")
        flipped = want_pm and not self._nl_pm
        if flipped:
            capi.check(self._lib, self._h, self._lib.mdpp_noise_levels_per_env_mdp(self._h, 1), "mdpp_noise_levels_per_env_mdp")
        rc = self._lib.mdpp_set_noise_levels(self._h, capi.nptr(arrays["transition_noise"]), capi.nptr(arrays["reward_noise"]), self._stream())
        if rc in (-4, capi.EUNSUPPORTED):    # MDPP_ESTATE: a handle the learner kernels do not serve; ... or one MDP per env
            msg = self._lib.mdpp_last_error(self._h)
            if flipped:                      # (the opt-in goes back to what it was.  The reason was read first: the flag call keeps it)
                capi.check(self._lib, self._h, self._lib.mdpp_noise_levels_per_env_mdp(self._h, int(self._nl_pm)), "mdpp_noise_levels_per_env_mdp")
            raise NotImplementedError(msg.decode() if msg else "mdpp_set_noise_levels: unsupported")
        if rc != 0 and flipped:
            msg = self._lib.mdpp_last_error(self._h)
            capi.check(self._lib, self._h, self._lib.mdpp_noise_levels_per_env_mdp(self._h, int(self._nl_pm)), "mdpp_noise_levels_per_env_mdp")
            raise capi.MdppError("mdpp_set_noise_levels failed (%d): %s" % (rc, msg.decode() if msg else ""))
        capi.check(self._lib, self._h, rc, "mdpp_set_noise_levels")
        self._nl_pm = want_pm
        self._noise_levels_set = True

    def noise_levels(self):
        """(transition_noise, reward_noise) in force, float64 numpy [N] each: what set_noise_levels gave, else the creation
        values (0 for a key the config does not have)."""
        self._learn_check_kind()
        tn, rn = np.empty(self.num_envs, np.float64), np.empty(self.num_envs, np.float64)
        capi.check(self._lib, self._h, self._lib.mdpp_get_noise_levels(self._h, capi.nptr(tn), capi.nptr(rn)), "mdpp_get_noise_levels")
        return tn, rn

    def clear_noise_levels(self):
        """Back to the creation values of both keys: the handle launches the kernels it launched before set_noise_levels."""
        capi.check(self._lib, self._h, self._lib.mdpp_clear_noise_levels(self._h), "mdpp_clear_noise_levels")
        if self._nl_pm:
            capi.check(self._lib, self._h, self._lib.mdpp_noise_levels_per_env_mdp(self._h, 0), "mdpp_noise_levels_per_env_mdp")
            self._nl_pm = False
        self._noise_levels_set = False

    def rollout_kernel_name(self, K):
        """Name (with template arguments) of the kernel mdpp_step_n(K) launches for this handle, as
        decided by the library's own dispatch code (mdpp_kernel_name; nothing is launched)."""
        name = self._lib.mdpp_kernel_name(self._h, int(K))
        return name.decode() if name else ""

    def set_kernel_options(self, *disable):
        """Take specialised kernels out of the dispatch (names of capi.OPTIONS and capi.GRID_OPTIONS, e.g. "NO_PIPE"): the
        handle then runs on the more general kernel of the same arithmetic.  Tests / profiling only;
        results do not depend on it.  No arguments = default dispatch."""
        mask = 0
        for d in disable:
            mask |= capi.GRID_OPTIONS[d] if d in capi.GRID_OPTIONS else capi.OPTIONS[d]
        capi.check(self._lib, self._h, self._lib.mdpp_set_options(self._h, mask), "mdpp_set_options")

    def alloc_rollout(self, K):
        N, dev = self.num_envs, self.device
        shape = self._obs_shape(K, N)
        return (torch.empty(shape, dtype=self._obs_torch_dtype, device=dev),
                torch.empty((K, N), dtype=torch.float32, device=dev),
                torch.empty((K, N), dtype=torch.uint8, device=dev),
                torch.empty((K, N), dtype=torch.uint8, device=dev))

    def _as_actions(self, actions, K):
        want = torch.float32 if self.kind == "continuous" else torch.int32
        if not torch.is_tensor(actions):
            actions = torch.as_tensor(np.asarray(actions), device=self.device)
        if self.kind == "continuous" and actions.dtype != torch.float32:
            # the reference rejects non-float32 actions (Box.contains -> "stay", :1640,:1671);
            # a batched API cannot flag dtype per env, so raise instead of silently staying
            raise TypeError(f"continuous actions must be float32, got {actions.dtype}")
        a = actions.to(device=self.device, dtype=want).contiguous()
        lead = (self.num_envs,) if K is None else (K, self.num_envs)
        if self.kind == "discrete":
            shape = lead + (2,) if self._irr else lead
        elif self.kind == "grid":
            # the reference treats a non-integer action as outside the action space (noop, :1731);
            # a batched API cannot flag dtype per env, so raise instead of silently staying
            if actions.dtype.is_floating_point:
                raise TypeError(f"grid actions must be integers, got {actions.dtype}")
            shape = lead + (len(self.mdps[0].grid_shape),)
        else:
            shape = lead + (self.mdps[0].D,)
        if tuple(a.shape) != shape:
            raise ValueError(f"actions must have shape {shape}, got {tuple(a.shape)}")
        return a

    # ------------------------------------------------------------------ state access
    def get_augmented_state(self):
        """Batched get_augmented_state() (rl_toy_env.py:2127) plus what the reference leaves out:
        reward ring, step counters, reached flags, and with autoreset="next_step" the per-env flag
        "the next call is the reset" (`reset_pending`).  Host numpy arrays (synchronises)."""
        st = self._get_augmented_state()
        if self.autoreset == "next_step":
            pend = np.zeros(self.num_envs, np.uint8)
            rc = self._lib.mdpp_get_reset_pending(self._h, capi.nptr(pend))
            capi.check(self._lib, self._h, rc, "mdpp_get_reset_pending")
            st["reset_pending"] = pend.astype(bool)
        return st

    def _get_augmented_state(self):
        N = self.num_envs
        if self.kind == "discrete":
            L, d = self._cfg.L, self._cfg.delay
            hist = np.zeros((N, L + 1), np.int32)
            steps = np.zeros(N, np.int32)
            ring = np.zeros((N, d), np.float64)
            rc = self._lib.mdpp_get_state_discrete(self._h, capi.nptr(hist), capi.nptr(steps), capi.nptr(ring))
            capi.check(self._lib, self._h, rc, "mdpp_get_state_discrete")
            cur = hist[:, -1].astype(np.int64)
            if self._irr:                              # curr_state = (relevant, irrelevant), :2089
                irr = np.zeros(N, np.int32)
                rc = self._lib.mdpp_get_state_irrelevant(self._h, capi.nptr(irr))
                capi.check(self._lib, self._h, rc, "mdpp_get_state_irrelevant")
                cur = np.stack([cur, irr.astype(np.int64)], axis=1)
            return {"curr_state": cur, "curr_obs": cur,
                    "augmented_state": hist, "total_transitions_episode": steps, "reward_buffer": ring}
        if self.kind == "grid":
            G = self._cfg.grid_dims
            cells = np.zeros((N, G), np.int32)
            steps = np.zeros(N, np.int32)
            reached = np.zeros(N, np.uint8)
            rc = self._lib.mdpp_get_state_grid(self._h, capi.nptr(cells), capi.nptr(steps), capi.nptr(reached))
            capi.check(self._lib, self._h, rc, "mdpp_get_state_grid")
            cur = cells.astype(np.int64)
            return {"curr_state": cur, "curr_obs": cur, "augmented_state": cur[:, :2],
                    "total_transitions_episode": steps, "reached_terminal": reached.astype(bool)}
        D, n, d = self._cfg.D, self._cfg.order, self._cfg.delay
        sd = np.zeros((N, n + 1, D), np.float32)
        cur = np.zeros((N, D), np.float32)
        steps = np.zeros(N, np.int32)
        ring = np.zeros((N, d), np.float64)
        is32 = np.zeros((N, d), np.uint8)
        reached = np.zeros(N, np.uint8)
        rc = self._lib.mdpp_get_state_continuous(self._h, capi.nptr(sd), capi.nptr(cur), capi.nptr(steps),
                                                 capi.nptr(ring), capi.nptr(is32), capi.nptr(reached))
        capi.check(self._lib, self._h, rc, "mdpp_get_state_continuous")
        aug = cur
        if self._line_L:
            # move_along_a_line: what the reference's augmented_state is read for (rl_toy_env.py:1865-1872, :2147-2156) --
            # the last sequence_length states' relevant coordinates, oldest first, NaN before the episode's reset
            aug = np.zeros((N, self._line_L, self._cfg.n_rel), np.float32)
            rc = self._lib.mdpp_get_line_history(self._h, capi.nptr(aug))
            capi.check(self._lib, self._h, rc, "mdpp_get_line_history")
        return {"curr_state": cur, "curr_obs": cur, "augmented_state": aug, "state_derivatives": sd,
                "total_transitions_episode": steps, "reward_buffer": ring, "reward_buffer_is32": is32,
                "reached_terminal": reached.astype(bool)}

    def set_augmented_state(self, state):
        """Inverse of get_augmented_state() (rl_toy_env.py:2168).  `reset_pending` (next-step autoreset) is
        restored when present and cleared when absent."""
        self._set_augmented_state(state)
        pend = state.get("reset_pending") if isinstance(state, dict) else None
        pend = np.zeros(self.num_envs, np.uint8) if pend is None else np.ascontiguousarray(pend, dtype=np.uint8)
        if pend.shape != (self.num_envs,):
            raise ValueError("reset_pending must have shape (num_envs,)")
        if self.autoreset == "next_step" or pend.any():
            rc = self._lib.mdpp_set_reset_pending(self._h, capi.nptr(pend))
            capi.check(self._lib, self._h, rc, "mdpp_set_reset_pending")

    def _set_augmented_state(self, state):
        if self.kind == "discrete":
            hist = np.ascontiguousarray(state["augmented_state"], dtype=np.int32)
            steps = np.ascontiguousarray(state["total_transitions_episode"], dtype=np.int32)
            ring = state.get("reward_buffer")       # (absent: the delay line stays as it is, like the reference)
            ring = None if ring is None else np.ascontiguousarray(ring, np.float64)
            rc = self._lib.mdpp_set_state_discrete(self._h, capi.nptr(hist), capi.nptr(steps), capi.nptr(ring))
            capi.check(self._lib, self._h, rc, "mdpp_set_state_discrete")
            if self._irr:
                irr = np.ascontiguousarray(np.asarray(state["curr_state"])[:, 1], dtype=np.int32)
                rc = self._lib.mdpp_set_state_irrelevant(self._h, capi.nptr(irr))
                capi.check(self._lib, self._h, rc, "mdpp_set_state_irrelevant")
            return
        if self.kind == "grid":
            cells = np.ascontiguousarray(state["curr_state"], dtype=np.int32)
            steps = np.ascontiguousarray(state["total_transitions_episode"], dtype=np.int32)
            reached = state.get("reached_terminal")
            reached = None if reached is None else np.ascontiguousarray(reached, np.uint8)
            rc = self._lib.mdpp_set_state_grid(self._h, capi.nptr(cells), capi.nptr(steps), capi.nptr(reached))
            capi.check(self._lib, self._h, rc, "mdpp_set_state_grid")
            return
        sd = np.ascontiguousarray(state["state_derivatives"], dtype=np.float32)
        cur = np.ascontiguousarray(state["curr_state"], dtype=np.float32)
        steps = np.ascontiguousarray(state["total_transitions_episode"], dtype=np.int32)
        ring = state.get("reward_buffer")
        ring = None if ring is None else np.ascontiguousarray(ring, np.float64)
        is32 = state.get("reward_buffer_is32")
        is32 = None if is32 is None else np.ascontiguousarray(is32, np.uint8)
        reached = state.get("reached_terminal")
        reached = None if reached is None else np.ascontiguousarray(reached, np.uint8)
        rc = self._lib.mdpp_set_state_continuous(self._h, capi.nptr(sd), capi.nptr(cur), capi.nptr(steps),
                                                 capi.nptr(ring), capi.nptr(is32), capi.nptr(reached))
        capi.check(self._lib, self._h, rc, "mdpp_set_state_continuous")
        if self._line_L:
            # two layouts: the [N, sequence_length, n_relevant] window get_augmented_state() returns here, or the REFERENCE's
            # (rl_toy_env.py:660, :2147-2156): per env a list of sequence_length + delay + 1 full state vectors, oldest first
            # -- [N, L + delay + 1, D]; the reward reads its last L rows and the relevant columns (:1865-1872), which is what
            # is kept (the rows before them only feed the delay line, restored through `reward_buffer`)
            aug = np.asarray(state["augmented_state"], dtype=np.float32)
            D, L, d = self._cfg.D, self._line_L, self._cfg.delay
            if aug.shape == (self.num_envs, L + d + 1, D):
                rel = list(self.mdps[0].relevant_indices)
                aug = aug[:, -L:, :][:, :, rel]
            aug = np.ascontiguousarray(aug, dtype=np.float32)
            if aug.shape != (self.num_envs, L, self._cfg.n_rel):
                raise ValueError("move_along_a_line: augmented_state must be the [num_envs, sequence_length, n_relevant] history "
                                 "get_augmented_state() returns, or the reference's [num_envs, sequence_length + delay + 1, "
                                 "state_space_dim] list of states")
            rc = self._lib.mdpp_set_line_history(self._h, capi.nptr(aug))
            capi.check(self._lib, self._h, rc, "mdpp_set_line_history")

    def get_episode_stats(self):
        """The reference's per-episode statistics (attributes of every env object, logged at each reset() and cleared,
        rl_toy_env.py:2231-2247, :2360-2369), per env instance, for handles made with ``episode_stats=True``: a dict
        with the running episode's ``total_abs_noise_in_reward_episode``, ``total_reward_episode``,
        ``total_noisy_transitions_episode`` (discrete, grid), ``total_abs_noise_in_transition_episode`` ([N, D],
        continuous), ``total_transitions_episode``, and under ``"last_episode"`` the same for the episode each env's
        latest reset() ended (what the reference logs).  Host numpy arrays (synchronises)."""
        if not self.episode_stats:
            raise capi.MdppError("get_episode_stats: construct the env with episode_stats=True")
        N = self.num_envs
        D = self.mdps[0].D if self.kind == "continuous" else 0
        nk = 3 + D
        cur = np.zeros((nk, N), np.float64)
        last = np.zeros((nk + 1, N), np.float64)
        rc = self._lib.mdpp_get_episode_stats(self._h, capi.nptr(cur), capi.nptr(last))
        capi.check(self._lib, self._h, rc, "mdpp_get_episode_stats")

        def rows(a, transitions):
            d = {"total_abs_noise_in_reward_episode": a[0].copy(), "total_reward_episode": a[1].copy(),
                 "total_transitions_episode": transitions}
            if self.kind == "continuous":
                # (total_reward_episode of a continuous env is the reference's np.float32 running sum wherever its reward
                #  is np.float32 -- held here as the float64 of exactly that value)
                d["total_abs_noise_in_transition_episode"] = np.ascontiguousarray(a[3:3 + D].T)
            else:
                d["total_noisy_transitions_episode"] = a[2].astype(np.int64)
            return d
        out = rows(cur, np.asarray(self._get_augmented_state()["total_transitions_episode"], dtype=np.int64))
        out["last_episode"] = rows(last, last[nk].astype(np.int64))
        return out

    def get_mdp_tables(self):
        """The discrete tables the kernels read, as host numpy arrays: P uint8 [T, S, A] (uint16 beyond 255 states), the
        reward table -- rbits uint8 [T, ceil(S^L / 8)] with unit rewards, else rtable float64 [T, S^L] (S * A with a
        reward matrix) -- is_term uint8 [T, S] and init_cdf float64 [T, S]; T = num_envs for per-env MDPs, else 1."""
        if self.kind != "discrete":
            raise capi.MdppError("get_mdp_tables: discrete envs only")
        c = self._cfg
        T, S, A = c.num_tables, c.S, c.A
        nkeys = S * A if c.reward_kind == capi.REWARD_STATE_ACTION else S ** c.L
        P = np.zeros((T, S, A), np.uint8 if S <= 255 else np.uint16)
        is_term = np.zeros((T, S), np.uint8)
        init_cdf = np.zeros((T, S), np.float64)
        out = {"P": P, "is_term": is_term, "init_cdf": init_cdf}
        if c.unit_rewards:
            out["rbits"] = rbits = np.zeros((T, (nkeys + 7) // 8), np.uint8)
            rtable = None
        else:
            out["rtable"] = rtable = np.zeros((T, nkeys), np.float64)
            rbits = None
        rc = self._lib.mdpp_get_discrete_tables(self._h, capi.nptr(P), capi.nptr(rtable), capi.nptr(rbits),
                                                capi.nptr(is_term), capi.nptr(init_cdf))
        capi.check(self._lib, self._h, rc, "mdpp_get_discrete_tables")
        return out

    def get_seed_dicts(self):
        """uint64 [N, 8]: per env the seed dict of its MDP -- "env", then mdp._SEED_KEYS in order (rl_toy_env.py:285-333)."""
        if self._gen is not None:
            return self._seed_dicts.copy()
        out = np.zeros((self.num_envs, 8), np.uint64)
        for i in range(self.num_envs):
            m = self.mdps[i if self._per_env else 0]
            out[i] = [m.seed_dict.get("env") or 0] + [m.seed_dict.get(k) or 0 for k in mdp_mod._SEED_KEYS]
        return out

    def get_rng_streams(self, stream=capi.STREAM_ENV):
        words = np.zeros((self.num_envs, 6), np.uint64)
        rc = self._lib.mdpp_get_streams(self._h, stream, capi.nptr(words))
        capi.check(self._lib, self._h, rc, "mdpp_get_streams")
        return words

    def status(self):
        """Per-env sticky fault bits (bad action, ...), cleared by the call."""
        flags = np.zeros(self.num_envs, np.uint32)
        rc = self._lib.mdpp_status(self._h, capi.nptr(flags))
        capi.check(self._lib, self._h, rc, "mdpp_status")
        return flags

    # kernel timing on the caller's stream (HIP events inside the library)
    def timer_begin(self):
        capi.check(self._lib, self._h, self._lib.mdpp_timer_begin(self._h, self._stream()), "mdpp_timer_begin")

    def timer_end(self):
        ms = C.c_float()
        capi.check(self._lib, self._h, self._lib.mdpp_timer_end(self._h, self._stream(), C.byref(ms)), "mdpp_timer_end")
        return ms.value

    def close(self):
        if self._h is not None:
            torch.cuda.synchronize(self.device)
            self._lib.mdpp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class StepGraph:
    """What RLToyVectorEnv.step_graph() returns: a captured HIP graph of K mdpp_step launches.  replay() runs
    the K steps on the current stream and advances the handle's step counter by K, as K step() calls would."""

    def __init__(self, env, graph, K, tick0, actions, obs, reward, term, trunc, by_offset=False):
        self._env, self._g, self.K, self._tick0, self._by_offset = env, graph, K, tick0, by_offset
        self.actions, self.obs, self.reward = actions, obs, reward
        self.terminated, self.truncated = term.view(torch.bool), trunc.view(torch.bool)

    def replay(self):
        env = self._env
        d = int(env._cfg.delay)
        now = C.c_uint64()
        capi.check(env._lib, env._h, env._lib.mdpp_tick(env._h, 0, C.byref(now)), "mdpp_tick")
        if self._by_offset:
            # the captured launches add this to the counter they were captured with (in stream order before the graph)
            stream = C.c_void_p(torch.cuda.current_stream(env.device).cuda_stream)
            capi.check(env._lib, env._h, env._lib.mdpp_graph_set_tick_offset(env._h, int(now.value) - self._tick0, stream),
                       "mdpp_graph_set_tick_offset")
        else:
            ring_in_memory = d > 0 and (env.kind == "continuous" or (env.kind == "discrete" and not env._cfg.unit_rewards))
            if ring_in_memory and (int(now.value) - self._tick0) % d != 0:
                raise capi.MdppError("StepGraph.replay: %d steps were taken outside the graph since its capture; the delay line "
                                     "(length %d) would be read at the captured ring head" % (int(now.value) - self._tick0, d))
        self._g.replay()
        capi.check(env._lib, env._h, env._lib.mdpp_tick(env._h, self.K, None), "mdpp_tick")
        env._obs_src = self.obs[self.K - 1]


def make_vec(env_id="RLToyVec-v0", num_envs=1, **kwargs):
    """gym.make-style entry: 'RLToyVec-v0' and 'RLToyVecFiniteHorizon-v0' (max_episode_steps=100),
    the batched counterparts of RLToy-v0 / RLToyFiniteHorizon-v0 (mdp_playground/__init__.py:3-12)."""
    if env_id == "RLToyVec-v0":
        return RLToyVectorEnv(num_envs=num_envs, **kwargs)
    if env_id == "RLToyVecFiniteHorizon-v0":
        kwargs.setdefault("max_episode_steps", 100)
        return RLToyVectorEnv(num_envs=num_envs, **kwargs)
    raise ValueError(f"unknown env id {env_id}")
