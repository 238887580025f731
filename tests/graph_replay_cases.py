"""What tests/test_gpu_graph_replay.py runs: fused (mdpp_step_n, K > 1) and closed-loop launches captured into a HIP graph in
the library's capture mode and replayed while the handle's step counter moves (include/mdpp.h, the graph section).  Shared
with tests/test_graph_replay_host.py, which checks on the CPU that the table covers what it claims: every replay offset
residue mod 4 (the Philox blocks serve four ticks), at least two residues mod the delay (the head of a delay line kept in
memory), and both RNG modes for every kernel family that serves both.

A case is a dict:
  family    the kernel family (FAMILIES)
  rng       "numpy" | "philox"
  config    the env's config;  kw: the constructor's keywords;  opts: kernel options (set_kernel_options)
  N, K      envs, steps of the captured call
  call      "rollout" | "policy" | "learn" | "eval" | "learn_summary" | "eval_summary"
  prefix    what the kernel's name starts with;  has: substrings it must contain (the summary= forms have no name query of
            their own: the name is the full-output form's, whose template arguments the summary kernel shares)
  between   eager steps taken after replays 0 .. 3 (replay 4 is the last)
  learner   set_learner's keywords (closed-loop learner cases);  levels: per-env noise levels are set before the warm-up
  mutate    what is replaced between replays, on both handles (None: nothing)

N = 256 is one full workgroup (the role-split kernels want full blocks), N = 320 one full and one ragged.  K sits at the
dispatch threshold of the kernel (32 for lean and the multi-role quiet forms) or is 40; the learner's short-pieces case has
K = 12 (three captured launches per call)."""
import numpy as np

BETWEEN = (1, 2, 3, 5)
REPLAYS = len(BETWEEN) + 1

# family -> it serves both RNG modes (the table then needs a case on each)
FAMILIES = {
    "lean": True, "quiet": True, "general": True, "wide": False, "long": False,
    "cfast": True, "cline": True, "cstep": True, "grid": True, "image": True,
    "policy": True, "learn": True, "learn_pe": True, "eval": True, "summary": True, "nlev": True,
}
# (wide and long: one Philox handle each, the issue's list; their numpy forms are the general kernel's code, covered there)

_D = dict(state_space_type="discrete", action_space_type="discrete")
_S8 = dict(_D, state_space_size=8, action_space_size=8)
_PH = dict(rng="philox", philox_seed=77)

CFG2 = dict(_S8, delay=4, sequence_length=3, seed=0)
CFG2_NOISE = dict(CFG2, transition_noise=0.1, reward_noise=0.2)
S50 = dict(_D, state_space_size=50, action_space_size=50, delay=4, sequence_length=1, reward_density=0.25,
           terminal_state_density=0.25, seed=0)
S24_RDIST = dict(_D, state_space_size=24, action_space_size=24, sequence_length=1, reward_density=0.25,
                 terminal_state_density=0.25, reward_dist=[0.01, 1], seed=0)
_C12 = dict(state_space_type="continuous", state_space_dim=12, relevant_indices=[0, 1, 2, 3], irrelevant_features=True,
            target_point=[0, 0, 0, 0], target_radius=0.05, state_space_max=10, action_space_max=1, inertia=1,
            make_denser=True, reward_function="move_to_a_point")
CFG3 = dict(_C12, transition_dynamics_order=1, time_unit=1, seed=0)
CFG5 = dict(_C12, transition_dynamics_order=2, time_unit=0.1, transition_noise=0.05, reward_noise=0.05, seed=0)
LINE = dict(state_space_type="continuous", state_space_dim=4, transition_dynamics_order=1, inertia=1, time_unit=1, delay=0,
            sequence_length=10, reward_scale=1.5, reward_shift=0.25, action_space_max=1, state_space_max=6,
            reward_function="move_along_a_line", seed=8)
C14 = dict(state_space_type="continuous", state_space_dim=14, transition_dynamics_order=3, inertia=2.0, time_unit=0.5, delay=2,
           action_space_max=1, state_space_max=5, target_point=[0.5] * 14, target_radius=3.0, make_denser=True,
           reward_function="move_to_a_point", transition_noise=0.05, reward_noise=0.1, seed=3)
GRID = dict(state_space_type="grid", reward_function="move_to_a_point", grid_shape=(8, 8), make_denser=True, target_point=[5, 5],
            transition_noise=0.3, reward_noise=0.2, term_state_reward=-0.25, seed=31)
IMG4 = dict(_S8, delay=0, image_representations=True, image_width=84, image_height=84, image_transforms="shift,rotate",
            image_sh_quant=1, image_ro_quant=1, seed=3)

# the closed-loop shapes (tests/test_gpu_policy_rollout.py, tests/test_gpu_learn_rollout.py)
RDIST3 = dict(_S8, delay=3, sequence_length=2, reward_dist=[0.5, 1.0], seed=40)
CFG2_L = dict(CFG2, seed=40)
S8_NOISE = dict(_S8, delay=0, sequence_length=1, transition_noise=0.1, reward_noise=0.5, seed=0)
RDIST3_NOISE = dict(RDIST3, transition_noise=0.1, reward_noise=0.5)
S20 = dict(_D, state_space_size=20, action_space_size=20, delay=0, sequence_length=1, seed=0)
# a handle that is given per-env noise levels is created with both keys (tests/noise_levels_cases.py)
NLEV_CREATED = dict(transition_noise=0.5, reward_noise=3.0)
NLEV_TN = (0.0, 0.01, 0.02, 0.10, 0.25)
NLEV_RN = (0.0, 1.0, 5.0, 10.0, 25.0)
NLEV_TN2 = (0.0, 0.05, 0.15, 0.2, 0.5)          # the same number of distinct levels, other values
NLEV_RN2 = (0.5, 0.0, 2.0, 4.0, 8.0)

LEARNER = dict(alpha=0.3, gamma=0.9, epsilon=0.25, seed=(7 << 32) + 4321)
POLICY_SEED = (5 << 32) + 12345
OFF = 1000                          # env_id_offset of both handles


def level_arrays(n, tn=NLEV_TN, rn=NLEV_RN):
    i = np.arange(n)
    return np.asarray(tn)[i % 5], np.asarray(rn)[(i // 5) % 5]


def pe_arrays(n, seed):
    """per-env alpha and epsilon, float32 [n]"""
    r = np.random.default_rng(seed)
    return r.uniform(0.05, 1.0, n).astype(np.float32), r.uniform(0.0, 0.6, n).astype(np.float32)


def _case(family, rng, config, prefix, *, N=256, K=32, call="rollout", has=(), kw=None, opts=(), learner=None, levels=False,
          mutate=None, between=BETWEEN):
    kw = dict(kw or {})
    if rng == "philox":
        kw = dict(_PH, **kw)
    return dict(family=family, rng=rng, config=config, kw=kw, opts=tuple(opts), N=N, K=K, call=call, prefix=prefix, has=tuple(has),
                between=tuple(between), learner=learner, levels=levels, mutate=mutate)


CASES = {}

# ---- open-loop: mdpp_step_n, K > 1 ---------------------------------------------------------------------------------------
CASES.update({
    # k_discrete_rollout_lean (dispatched at K >= 32): r4 = ptick0 & 3 and the chunk base blocks come from the counter
    "lean_philox": _case("lean", "philox", CFG2, "k_discrete_rollout_lean<", has=("PHILOX=1", "NEXT=0")),
    "lean_philox_ragged_k40": _case("lean", "philox", CFG2, "k_discrete_rollout_lean<", N=320, K=40, has=("PHILOX=1",)),
    "lean_philox_noise": _case("lean", "philox", CFG2_NOISE, "k_discrete_rollout_lean<", has=("PHILOX=1", "PN=1,RN=1")),
    "lean_philox_next": _case("lean", "philox", dict(_S8, delay=2, sequence_length=2, seed=7), "k_discrete_rollout_lean<",
                              has=("PHILOX=1", "NEXT=1"), kw=dict(autoreset="next_step", max_episode_steps=9)),
    "lean_philox_max7": _case("lean", "philox", dict(_S8, delay=0, sequence_length=3, seed=6), "k_discrete_rollout_lean<",
                              has=("PHILOX=1", "HASMAX=1"), kw=dict(max_episode_steps=7)),     # start states are drawn
    "lean_numpy_npnoise": _case("lean", "numpy", CFG2_NOISE, "k_discrete_rollout_lean<", has=("PHILOX=0", "PN=1,RN=1")),
    # k_discrete_rollout_quiet (K >= 16; two roles and the Philox producer waves at K >= 32 on full blocks)
    "quiet_philox_s50": _case("quiet", "philox", S50, "k_discrete_rollout_quiet<", has=("ROLES=2", "PHILOX=1", "NPH=2", "PN=0,RN=0")),
    "quiet_philox_s50_noise": _case("quiet", "philox", dict(S50, transition_noise=0.1), "k_discrete_rollout_quiet<",
                                    has=("ROLES=2", "PHILOX=1", "NPH=2", "PN=1,RN=0")),
    # (with reward noise the record ring is twice as wide and leaves the producer waves no LDS: two roles alone)
    "quiet_philox_s50_both_noises": _case("quiet", "philox", dict(S50, transition_noise=0.1, reward_noise=0.3), "k_discrete_rollout_quiet<",
                                          has=("ROLES=2", "PHILOX=1", "NPH=0", "PN=1,RN=1")),
    "quiet_philox_s50_ragged_k16": _case("quiet", "philox", S50, "k_discrete_rollout_quiet<", N=320, K=16, has=("ROLES=1", "PHILOX=1")),
    "quiet_philox_irr": _case("quiet", "philox", dict(_D, state_space_size=[12, 6], action_space_size=[12, 6], irrelevant_features=True,
                                                       delay=2, sequence_length=2, transition_noise=0.2, seed=41),
                              "k_discrete_rollout_quiet<", has=("IRR=1", "PHILOX=1")),
    "quiet_numpy_nu_delay2": _case("quiet", "numpy", dict(S24_RDIST, delay=2), "k_discrete_rollout_quiet<",
                                   has=("ROLES=3", "PHILOX=0", "UNIT=0", "SF=1")),
    "quiet_numpy_nu_delay3": _case("quiet", "numpy", dict(S24_RDIST, delay=3), "k_discrete_rollout_quiet<",
                                   has=("ROLES=3", "PHILOX=0", "UNIT=0", "SF=1")),
    # k_discrete_step: the general kernel's multi-step path
    "general_philox_nu_delay2": _case("general", "philox", dict(S24_RDIST, delay=2), "k_discrete_step<", has=("PHILOX=1", "UNIT=0")),
    "general_philox_nu_ragged_k5": _case("general", "philox", dict(S24_RDIST, delay=3), "k_discrete_step<", N=320, K=5,
                                         has=("PHILOX=1", "UNIT=0")),
    "general_numpy_no_quiet": _case("general", "numpy", dict(S24_RDIST, delay=3, transition_noise=0.2), "k_discrete_step<",
                                    has=("PHILOX=0", "UNIT=0"), opts=("NO_QUIET",)),
    "wide_philox_s300": _case("wide", "philox", dict(_D, state_space_size=300, action_space_size=300, sequence_length=1, delay=2,
                                                      reward_density=0.25, terminal_state_density=0.1, transition_noise=0.2,
                                                      reward_noise=0.3, seed=11), "k_discrete_step_wide<", K=8, has=("PHILOX=1",)),
    "long_philox_l9": _case("long", "philox", dict(_D, state_space_size=4, action_space_size=4, sequence_length=9,
                                                    repeats_in_sequences=True, delay=2, terminal_state_density=0.25,
                                                    transition_noise=0.2, reward_noise=0.3, seed=11), "k_discrete_step_long<", K=8,
                            has=("PHILOX=1",)),
    # continuous
    "cfast_philox_cfg5": _case("cfast", "philox", CFG5, "k_continuous_rollout_fast<", has=("D=12,ORDER=2,NREL=4", "PHILOX=1")),
    "cfast_numpy_cfg3_delay3": _case("cfast", "numpy", dict(CFG3, delay=3), "k_continuous_rollout_fast<",
                                     has=("D=12,ORDER=1,NREL=4", "GEN=1", "PHILOX=0")),         # the ring in memory
    "cline_philox": _case("cline", "philox", LINE, "k_continuous_line_rollout<", has=("PHILOX=1",), kw=dict(max_episode_steps=37)),
    "cline_numpy_ragged": _case("cline", "numpy", LINE, "k_continuous_line_rollout<", N=320, has=("PHILOX=0",),
                                kw=dict(max_episode_steps=37)),
    "cstep_philox_d14_o3": _case("cstep", "philox", C14, "k_continuous_step<", K=8, has=("PHILOX=1",)),
    "cstep_numpy_d14_o3": _case("cstep", "numpy", C14, "k_continuous_step<", N=320, K=8, has=("PHILOX=0",)),
    # grid
    "grid_philox_noise": _case("grid", "philox", GRID, "k_grid_rollout_fast<", has=("PN=1,RN=1", "PHILOX=1")),
    "grid_numpy_noise_ragged": _case("grid", "numpy", GRID, "k_grid_rollout_fast<", N=320, K=8, has=("PN=1,RN=1", "PHILOX=0")),
    # images: the transforms are keyed by the counter; 72 steps are two batches (64 + 8), so the handle's side-stream
    # pipeline is captured with the call
    "image_philox_cfg4": _case("image", "philox", IMG4, "k_image_obs", K=8),
    "image_numpy_cfg4": _case("image", "numpy", IMG4, "k_image_obs", K=8),
    "image_philox_cfg4_two_batches": _case("image", "philox", IMG4, "k_image_obs", K=72),
})

# ---- closed-loop: the agent's streams are Philox-keyed by the counter on every handle ---------------------------------------
for _rng in ("numpy", "philox"):
    _p = "PHILOX=%d" % (_rng == "philox")
    CASES.update({
        # rollout_policy
        "policy_rdist_delay3_" + _rng: _case("policy", _rng, dict(RDIST3, seed=0), "k_discrete_policy_rollout<", N=320, K=40, call="policy",
                                             has=(_p, "UNIT=0")),
        "policy_next_step_" + _rng: _case("policy", _rng, CFG2, "k_discrete_policy_rollout<", call="policy", has=(_p, "UNIT=1"),
                                          kw=dict(autoreset="next_step")),
        "policy_replaced_" + _rng: _case("policy", _rng, CFG2, "k_discrete_policy_rollout<", N=320, K=37, call="policy", has=(_p,),
                                         mutate="policy"),
        # rollout_learn
        "learn_q_" + _rng: _case("learn", _rng, CFG2_L, "k_discrete_learn_rollout<", N=320, K=40, call="learn", has=(_p, "QLDS=1"),
                                 learner=dict(LEARNER, algo="q_learning")),
        "learn_sarsa_" + _rng: _case("learn", _rng, RDIST3, "k_discrete_learn_rollout<", K=37, call="learn", has=(_p, "UNIT=0", "QLDS=1"),
                                     learner=dict(LEARNER, algo="sarsa")),
        "learn_double_" + _rng: _case("learn", _rng, CFG2_L, "k_discrete_learn_rollout<", call="learn", has=(_p, "DOUBLE=1"),
                                      learner=dict(LEARNER, algo="double_q"), kw=dict(autoreset="next_step")),
        "learn_no_lds_" + _rng: _case("learn", _rng, CFG2_L, "k_discrete_learn_rollout<", call="learn", has=(_p, "QLDS=0"),
                                      learner=dict(LEARNER, algo="sarsa"), opts=("NO_LEARN_LDS",)),
        "learn_short_pieces_" + _rng: _case("learn", _rng, CFG2_L, "k_discrete_learn_rollout<", N=320, K=12, call="learn", has=(_p,),
                                            learner=dict(LEARNER, algo="sarsa"), opts=("LEARN_SHORT_PIECES",)),
        "learn_noise_" + _rng: _case("learn", _rng, RDIST3_NOISE, "k_discrete_learn_rollout<", call="learn", has=(_p, "NOISE=1", "UNIT=0"),
                                     learner=dict(LEARNER, algo="q_learning")),
        # the PE form: per-env alpha / epsilon arrays, read at replay
        "learn_pe_" + _rng: _case("learn_pe", _rng, S8_NOISE, "k_discrete_learn_rollout<", N=320, K=40, call="learn", has=(_p, "PE=1"),
                                  learner=dict(LEARNER, algo="q_learning", per_env=True)),
        "learn_pe_replaced_" + _rng: _case("learn_pe", _rng, CFG2_L, "k_discrete_learn_rollout<", call="learn", has=(_p, "PE=1", "DOUBLE=1"),
                                           learner=dict(LEARNER, algo="double_q", per_env=True), mutate="rates"),
        # rollout_eval, and the summary= forms: the five tensors accumulate across replays
        "eval_" + _rng: _case("eval", _rng, RDIST3, "k_discrete_eval_rollout<", N=320, K=40, call="eval", has=(_p, "UNIT=0"),
                              learner=dict(LEARNER, algo="q_learning", random_q=True)),
        "eval_double_noise_" + _rng: _case("eval", _rng, RDIST3_NOISE, "k_discrete_eval_rollout<", call="eval", has=(_p, "NOISE=1", "UNIT=0", "DOUBLE=1"),
                                           learner=dict(LEARNER, algo="double_q", random_q=True)),
        "learn_summary_" + _rng: _case("summary", _rng, CFG2_L, "k_discrete_learn_rollout<", N=320, K=40, call="learn_summary", has=(_p,),
                                       learner=dict(LEARNER, algo="sarsa")),
        "eval_summary_" + _rng: _case("summary", _rng, RDIST3, "k_discrete_eval_rollout<", call="eval_summary", has=(_p, "UNIT=0"),
                                      learner=dict(LEARNER, algo="q_learning", random_q=True), kw=dict(max_episode_steps=9)),
        # NLEV: per-env noise levels, set before the warm-up
        "nlev_learn_" + _rng: _case("nlev", _rng, dict(CFG2_L, **NLEV_CREATED), "k_discrete_learn_rollout<", N=320, K=40, call="learn",
                                    has=(_p, "PE=1", "NLEV=1"), learner=dict(LEARNER, algo="q_learning"), levels=True),
        "nlev_levels_replaced_" + _rng: _case("nlev", _rng, dict(RDIST3, **NLEV_CREATED), "k_discrete_learn_rollout<", call="learn",
                                              has=(_p, "PE=1", "NLEV=1", "UNIT=0"), learner=dict(LEARNER, algo="sarsa"), levels=True,
                                              mutate="levels"),
        "nlev_eval_summary_" + _rng: _case("nlev", _rng, dict(S20, delay=3, reward_dist=[0.5, 1.0], **NLEV_CREATED), "k_discrete_eval_rollout<",
                                           N=320, K=40, call="eval_summary", has=(_p, "UNIT=0", "QLDS=0", "NLEV=1"),
                                           learner=dict(LEARNER, algo="double_q", random_q=True), levels=True),
    })

# By-value semantics: uniform rates changed on the graph's handle after the capture do not reach the replay
BY_VALUE_CASE = _case("learn", "philox", CFG2_L, "k_discrete_learn_rollout<", N=320, K=40, call="learn", has=("PHILOX=1",),
                      learner=dict(LEARNER, algo="q_learning"))

CLOSED_CALLS = ("policy", "learn", "eval", "learn_summary", "eval_summary")


def offsets(case):
    """the tick offset of every replay: 0, then the running sum of K and the eager steps in between"""
    out, t = [0], 0
    for b in case["between"]:
        t += case["K"] + b
        out.append(t)
    return out


def delay_of(case):
    return int(case["config"].get("delay", 0))


def needs_offset(case):
    """True where a replay that withholds the tick offset must differ from the eager twin: the env's Philox keys, the Philox
    streams of a sampling policy or an exploring learner (greedy evaluation draws nothing), or the head of a delay line kept in
    memory (continuous envs, non-unit discrete rewards).  False: by-value capture would do -- such a case shows that the
    device word does not disturb the launch."""
    ring_in_memory = delay_of(case) > 0 and (case["config"]["state_space_type"] == "continuous" or
                                             (case["config"]["state_space_type"] == "discrete" and "reward_dist" in case["config"]))
    return case["rng"] == "philox" or case["call"] in ("policy", "learn", "learn_summary") or ring_in_memory


# the cases a by-value capture would serve (numpy streams, no delay line in memory), kept on purpose
BY_VALUE_WOULD_DO = ("cline_numpy_ragged", "grid_numpy_noise_ragged", "image_numpy_cfg4", "lean_numpy_npnoise")
