/* mdpp.h — C ABI of libmdpp_hip.so: batched RLToyEnv.step()/reset() on MI355X (gfx950).
 *
 * One handle = one shard of env instances on one GPU.  Every `*_dev` pointer is a
 * DEVICE pointer owned by the caller (the Python layer passes torch tensors'
 * data_ptr()); every `*_host` pointer is host memory.  All work is enqueued on the
 * caller's HIP stream (`stream` is a hipStream_t passed as void*; NULL = default
 * stream) and is asynchronous with respect to the host (image rollouts additionally fork to a side
 * stream owned by the handle and join back into the caller's stream before they return).  The library owns only its
 * per-env state and tables (freed by mdpp_destroy); nothing is allocated inside
 * mdpp_step / mdpp_step_n / mdpp_reset or the closed-loop launches (mdpp_step_n_policy / _learn / _eval and their
 * _summary forms, mdpp_current_obs), so they can be captured into a HIP graph
 * (tests/test_gpu_parity.py::test_rollout_is_graph_capturable, tests/test_gpu_graph_replay.py).  The handle's step counter
 * travels to the kernels by value: a replayed graph is exact for numpy-stream handles with
 * unit rewards; Philox keys and the key ring of non-unit rewards read the counter -- such handles, and every
 * closed-loop launch, replay exactly in capture mode (the section "HIP graphs" below).  A handle is not
 * thread-safe.  Every function returns 0 on success or a negative MDPP_E* code and
 * never throws; mdpp_last_error() gives the message.
 *
 * What each entry point replaces in the reference (/root/reference):
 *   mdpp_create + mdpp_upload_*   RLToyEnv.__init__            mdp_playground/envs/rl_toy_env.py:216-853
 *                                 (the tables themselves are generated on the host by
 *                                  mdp_playground_amd/mdp.py, restating :855-1575, or for
 *                                  per-env discrete MDPs by mdpp_generate_discrete)
 *   mdpp_seed_streams             RLToyEnv.seed / Space.seed   rl_toy_env.py:2379-2406,
 *                                                              spaces/discrete_extended.py:7-9
 *   mdpp_reset                    RLToyEnv.reset               rl_toy_env.py:2217-2377
 *   mdpp_step                     RLToyEnv.step                rl_toy_env.py:1992-2125
 *                                 (transition_function :1577-1725, reward_function :1782-1990,
 *                                  ImageMultiDiscrete.get_image_representation
 *                                  spaces/image_multi_discrete.py:129-288)
 *                                 (grid: transition :1727-1778, reward :1947-1965,
 *                                  GridActionSpace spaces/grid_action_space.py:13-39)
 *   mdpp_step_n                   a Python loop of K step() calls (e.g. example.py:69-86)
 *   mdpp_get_state/set_state      get/set_augmented_state      rl_toy_env.py:2127-2215
 *                                 (plus the RNG streams, ring and counters the reference omits)
 */
#ifndef MDPP_H
#define MDPP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDPP_ABI_VERSION 8

enum { MDPP_OK = 0, MDPP_EINVAL = -1, MDPP_EHIP = -2, MDPP_ENOMEM = -3, MDPP_ESTATE = -4,
       MDPP_EUNSUPPORTED = -5 };

enum { MDPP_KIND_DISCRETE = 0, MDPP_KIND_CONTINUOUS = 1, MDPP_KIND_GRID = 2 };
enum { MDPP_RNG_NUMPY_PCG64 = 0,   /* per-env numpy Generator(PCG64) streams: reference-exact */
       MDPP_RNG_PHILOX = 1 };      /* counter-based Philox4x32-10 keyed by (seed, global env id, tick, stream id): no reference for
                                      this mode, its draws are defined in mdp_playground_amd/csrc/mdpp_rng.hpp and restated in
                                      oracle/np_random.c.  Stream ids: 0-4 the MDPP_STREAM_* below (whole blocks per tick:
                                      continuous / grid noise, image transforms; 4 also the irrelevant sub-space's transition
                                      noise), 3 an explicit reset(), 5 grid noisy action, 6-8 the post-processor, 9 / 10 the
                                      start state of an in-rollout reset (relevant / irrelevant), 11 an explicit reset()'s image,
                                      12 discrete transition noise, 13 discrete reward noise -- ids 4 (discrete), 9, 10, 12, 13
                                      take ONE word (one float32 normal) per tick from a block that serves four ticks */
enum { MDPP_AUTORESET_DISABLED = 0,    /* the reference's own behaviour: keeps stepping after done */
       MDPP_AUTORESET_SAME_STEP = 1,   /* gymnasium 0.29 SyncVectorEnv: the step that ends an episode returns the next episode's first obs */
       MDPP_AUTORESET_NEXT_STEP = 2 }; /* gymnasium >= 1.0 vector envs: the step() AFTER the one that ended an episode ignores that env's
                                          action, resets it and returns (first obs, reward 0, no flags) */
enum { MDPP_OBS_I64 = 0, MDPP_OBS_I32 = 1, MDPP_OBS_F32 = 2, MDPP_OBS_IMAGE_U8 = 3 };
/* RNG streams, named after the generator object they mirror in the reference */
enum { MDPP_STREAM_ENV = 0,        /* RLToyEnv._np_random: reset draw, reward noise, continuous P-noise */
       MDPP_STREAM_SPACE = 1,      /* discrete: observation_spaces[0] (P-noise); continuous, grid: feature_space (reset) */
       MDPP_STREAM_IMAGE = 2,      /* observation_space (ImageMultiDiscrete transforms) */
       MDPP_STREAM_SPACE_IRR = 3,  /* discrete, irrelevant_features: observation_spaces[1] (its P-noise) */
       MDPP_STREAM_ACTION = 4,     /* grid: action_space (GridActionSpace.sample of a noisy action) */
       MDPP_NUM_STREAMS = 5 };
/* per-env status bits (mdpp_status) */
enum { MDPP_STATUS_BAD_ACTION = 1u,     /* discrete: action out of range (reference: IndexError);
                                           continuous: action rejected by Box.contains -> "stay" (:1671) */
       MDPP_STATUS_RESET_GAVE_UP = 2u,  /* continuous reset(): 4096 draws all fell into terminal hypercubes */
       MDPP_STATUS_INTERNAL = 0x80000000u }; /* a bounded in-kernel wait expired (never expected) */

/* Kernel-selection switches (mdpp_set_options): each bit takes one specialised rollout kernel (or
 * one of its multi-wave forms) out of the dispatch, so that the same handle runs on the more general
 * kernel of the same arithmetic.  Results never depend on them (tests compare both sides); they exist
 * for those tests, for profiling and for ablations.  Per handle; nothing is read from the environment. */
enum { MDPP_OPT_NO_PIPE = 1u << 0,         /* discrete: no three-role k_discrete_rollout_pipe */
       MDPP_OPT_NO_HELPER = 1u << 1,       /* no helper (producer) waves in k_*_rollout_fast */
       MDPP_OPT_NO_PARK = 1u << 2,         /* continuous helper waves draw in lockstep (no parked lanes) */
       MDPP_OPT_NO_CFAST = 1u << 3,        /* continuous: k_continuous_step instead of k_continuous_rollout_fast */
       MDPP_OPT_NO_QUIET = 1u << 4,        /* discrete: k_discrete_step instead of k_discrete_rollout_quiet */
       MDPP_OPT_NO_QUIET_NOISE = 1u << 5,  /* ... only for handles with P- or reward noise */
       MDPP_OPT_NO_DUO = 1u << 6,          /* k_discrete_rollout_quiet: one role only */
       MDPP_OPT_NO_TRIO = 1u << 7,         /* k_discrete_rollout_quiet: at most two roles */
       MDPP_OPT_NO_GFAST = 1u << 8,        /* grid: k_grid_step instead of k_grid_rollout_fast */
       MDPP_OPT_NO_GFAST_NOISE = 1u << 9,  /* ... only for handles with noise */
       MDPP_OPT_NO_IMGFAST = 1u << 10,     /* polygon images: k_image_obs instead of k_image_obs_fast */
       MDPP_OPT_NO_IMG_OVERLAP = 1u << 11, /* image rollouts: no side-stream pipeline of the batches */
       MDPP_OPT_NO_PHILOX_FAST = 1u << 12, /* Philox handles: general kernels only */
       MDPP_OPT_NO_LEAN = 1u << 13,        /* discrete: no k_discrete_rollout_lean (S <= 8 re-encoding of _pipe) */
       MDPP_OPT_NO_IMG_NEARTAB = 1u << 14, /* polygon images: k_image_obs_fast walks the bounding box instead of the near-dword table */
       MDPP_OPT_NO_STEP1 = 1u << 15,       /* mdpp_step (K = 1): the rollout kernels with K = 1 instead of k_discrete_step1 / k_continuous_step1 */
       MDPP_OPT_NO_QUIET_SF = 1u << 17,    /* k_discrete_rollout_quiet: no compile-time form of the sweep defaults (sequence_length 1, same-step autoreset, ...) */
       MDPP_OPT_NO_SIGMA0 = 1u << 16,      /* noise keys present with sigma 0 (the reference draws rng.normal(0, 0): rl_toy_env.py:398-403, :1982):
                                              form the normals' values anyway instead of advancing the streams alone */
       MDPP_OPT_NO_LEARN_LDS = 1u << 18,   /* k_discrete_learn_rollout: the Q-tables stay in global memory (QLDS=0) */
       MDPP_OPT_LEARN_SHORT_PIECES = 1u << 19, /* mdpp_step_n_policy and mdpp_step_n_learn go out in launches of at most 5 steps
                                              (the hand-over between the pieces of a very long call, at a size a test can run) */
       MDPP_OPT_NO_NLEV_LDS = 1u << 20,    /* per-env noise levels (mdpp_set_noise_levels): the per-level cdfs stay in global memory */
       MDPP_OPT_NO_PM_LDS = 1u << 21,      /* one MDP per env (mdpp_learner_per_env_mdp): the envs' tables stay in global memory (PM=1) */
       MDPP_OPT_NO_PM_NLEV_LDS = 1u << 22,   /* per-env noise levels on one MDP per env (mdpp_noise_levels_per_env_mdp): the per-level cdfs stay
                                              in global memory in the PM kernels (MDPP_OPT_NO_NLEV_LDS keeps its meaning for a shared MDP) */
       MDPP_OPT_NO_LINEAR_LDS = 1u << 23,    /* k_continuous_linear_rollout / _summary: the linear policies' parameters stay in global memory (PLDS=0) */
       MDPP_OPT_NO_GRID_QLDS = 1u << 24 };   /* k_grid_learn_rollout: the grid learners' Q-tables stay in global memory (QLDS=0) */

/* transition-noise levels one handle serves at a time (mdpp_set_noise_levels) */
#define MDPP_MAX_NOISE_LEVELS 16
#define MDPP_MAX_SCHEDULE_ENTRIES (1 << 22) /* R M of one table of mdpp_set_learner_schedule */

/* the tabular learner's algorithm (mdpp_set_learner); 2 is double Q-learning: two tables per env */
enum { MDPP_LEARN_Q_LEARNING = 0, MDPP_LEARN_SARSA = 1, MDPP_LEARN_DOUBLE_Q = 2 };
enum { MDPP_TRACE_ACCUMULATING = 1, MDPP_TRACE_REPLACING = 2 };    /* mdpp_set_learner_traces */

/* what a discrete env's reward table is keyed by */
enum { MDPP_REWARD_SEQUENCES = 0,     /* the last L states (rewardable_sequences, rl_toy_env.py:1837-1841) */
       MDPP_REWARD_STATE_ACTION = 1 }; /* (s, a) of the transition: use_custom_mdp with a reward MATRIX
                                          (:1259-1267, :1817-1818); no NaN gate, needs unit_rewards = 0 */

/* reward_function of a continuous env */
enum { MDPP_CREWARD_MOVE_TO_A_POINT = 0,    /* rl_toy_env.py:1912-1945 */
       MDPP_CREWARD_MOVE_ALONG_A_LINE = 1 }; /* :1864-1910: minus the mean distance of the last L states from
                                                the line fitted through them (first right-singular vector);
                                                n_rel <= 8 (state_space_dim <= 12 beyond 4), L <= 64, no image observations */

typedef struct mdpp_env mdpp_env;

#define MDPP_MAX_DIM 32
#define MDPP_MAX_ORDER 4
#define MDPP_MAX_BOXES 8

typedef struct {
    int32_t abi_version;        /* MDPP_ABI_VERSION */
    int32_t kind;               /* MDPP_KIND_* */
    int32_t num_envs;           /* env instances in this shard */
    int64_t env_id_offset;      /* global id of local env 0 (multi-GPU sharding; Philox keys use the global id) */
    int32_t rng_mode;           /* MDPP_RNG_* */
    int32_t autoreset;          /* MDPP_AUTORESET_* */
    int32_t max_episode_steps;  /* 0 = never truncate (RLToyFiniteHorizon-v0: 100) */
    int32_t obs_dtype;          /* MDPP_OBS_* */
    uint64_t philox_seed;       /* MDPP_RNG_PHILOX only */

    /* reward post-processing shared by both kinds, rl_toy_env.py:1968-1990, :2105-2109 */
    int32_t delay;              /* reward_buffer length */
    int32_t every_n;            /* reward_every_n_steps */
    int32_t has_reward_noise;   /* "reward_noise" in config (a normal is drawn even for std 0) */
    double reward_noise;        /* std */
    double reward_scale, reward_shift, term_state_reward;

    /* ---- discrete ---- */
    int32_t S, A, L;            /* state_space_size (<= 65 535), action_space_size, sequence_length (<= 15; S^L < 4e9) -- S > 255 and L > 7: the general
                                   kernel alone, not together, without image observations */
    int32_t num_tables;         /* 1 = one MDP shared by all envs; num_envs = one MDP per env */
    int32_t unit_rewards;       /* 1: every rewardable sequence pays exactly 1.0 (bitmask table) */
    int32_t reward_kind;        /* MDPP_REWARD_*: what the reward table is keyed by */
    int32_t has_transition_noise;
    double transition_noise;
    /* irrelevant_features=True (rl_toy_env.py:2028-2035, :2063-2092): a second, reward-irrelevant
     * sub-space with its own transition table and P-noise generator; actions and observations
     * become pairs [N][2] = (relevant, irrelevant) */
    int32_t irrelevant;
    int32_t S_irr, A_irr;

    /* ---- continuous ---- */
    int32_t D, n_rel, order;    /* state_space_dim, len(relevant_indices), transition_dynamics_order */
    int32_t reward_function;    /* MDPP_CREWARD_*; move_along_a_line takes sequence_length from L above */
    int32_t rel_idx[MDPP_MAX_DIM];
    int32_t make_denser;
    int32_t has_p_noise;        /* "transition_noise" in config (D normals drawn even for std 0) */
    double p_noise;             /* std */
    double inertia, time_unit, state_space_max, action_space_max;
    double target_radius, action_loss_weight;
    float target[MDPP_MAX_DIM];
    int32_t n_boxes;            /* terminal hypercubes, rl_toy_env.py:908-952: [n_boxes][n_rel] packed, n_boxes * n_rel <= 256 (ABI 8; 8 before) */
    float box_lo[MDPP_MAX_BOXES * MDPP_MAX_DIM];
    float box_hi[MDPP_MAX_BOXES * MDPP_MAX_DIM];

    /* ---- grid (move_to_a_point), rl_toy_env.py:1727-1778, :1947-1965; uses make_denser,
     * has_transition_noise / transition_noise (probability of a re-drawn action) from above ---- */
    int32_t grid_dims;          /* 2, or 4 with irrelevant_features (the grid repeated, :604-608) */
    int32_t grid_shape[4];
    int32_t grid_target[2];

    /* ---- image observations: discrete envs (ImageMultiDiscrete: polygons, random transforms), or
     * continuous envs (ImageContinuous, spaces/image_continuous.py:116-277: RGB pictures, uses image,
     * img_w, img_h and img_r0 = radius of the agent / target discs only) ---- */
    int32_t image;              /* 1: obs is uint8[W][H][1] per env (discrete) or uint8[n_sub W][H][3] (continuous, grid) */
    int32_t img_w, img_h;
    int32_t img_has_scale, img_has_shift, img_has_rotate, img_has_flip;
    int32_t img_sh_quant, img_ro_quant;
    int32_t img_r0;             /* circle_radius */
    int32_t img_r_min, img_r_max; /* radii that can occur (scale transform), templates cover [r_min, r_max] */
    double img_log_min_r, img_log_max_r;
    int32_t img_tpl_size;       /* templates are (2*tpl_half+1)^2 bitmaps */

    /* ---- ABI 6 ---- */
    int32_t episode_stats;      /* 1: keep the reference's per-episode noise statistics per env (mdpp_get_episode_stats); such
                                   handles run on the general kernels */
    int32_t target_f64;         /* continuous, move_to_a_point, no "target_point" in the config: the reference's default,
                                   np.zeros(shape=(state_space_dim,)) -- float64, every dimension relevant
                                   (rl_toy_env.py:652-654): distances, the target latch and a dense reward are float64 */
} mdpp_config;

/* Lifetime */
int mdpp_abi_version(void);
int mdpp_create(const mdpp_config *cfg, int device, mdpp_env **out);
void mdpp_destroy(mdpp_env *h);
const char *mdpp_last_error(const mdpp_env *h);   /* h may be NULL: last create() error */

/* Discrete tables (host pointers; T = cfg.num_tables):
 *   P        uint8 [T][S][A]      transition matrix                       rl_toy_env.py:1050-1151
 *            (cfg.S > 255, up to 65 535 -- round 6: uint16 [T][S][A] behind the same pointer; such handles run the general
 *            kernel alone, without image observations: mdpp_discrete_wide.hip)
 *   rtable   double[T][S^L] (MDPP_REWARD_SEQUENCES) or double[T][S][A] (MDPP_REWARD_STATE_ACTION:
 *            use_custom_mdp with a reward matrix, R(s, a) of the transition s, a -> s', :1259-1267)
 *            or, when cfg.unit_rewards, NULL with
 *   rbits    uint8 [T][ceil(S^L/8)] bit k set <=> sequence with key k is rewardable (:1508)
 *   is_term  uint8 [T][S]                                                 :868-889
 *   init_cdf double[T][S]  cumsum(rho_0)/cumsum(rho_0)[-1]                :1003-1018, :2255
 *   noise_cdf double[S][S] row n = normalised cdf of the P-noise categorical whose mode is n
 *            (:1605-1612); NULL when cfg.has_transition_noise == 0 */
int mdpp_upload_discrete_tables(mdpp_env *h, const uint8_t *P_host, const double *rtable_host,
                                const uint8_t *rbits_host, const uint8_t *is_term_host,
                                const double *init_cdf_host, const double *noise_cdf_host);

/* Per-env discrete MDPs generated on the device (mdpp_generate.hip): table i is what mdp.build_mdp({**config,
 * "seed": seeds_host[i]}) builds, bit for bit -- P, and the rewardable sequences into rbits or rtable -- drawn from numpy's
 * PCG64(SeedSequence) streams in the host's order.  For a handle with cfg.num_tables == cfg.num_envs, S <= 255, no
 * irrelevant sub-space and MDPP_REWARD_SEQUENCES; which configs qualify is decided by mdp.device_coverage (the sequence
 * draw must take Generator.choice's Floyd branch).  Numpy-stream handles also get every env's streams: ENV fresh from
 * the seed, SPACE as P's generation left it (its buffered half-word is not kept, as with mdpp_seed_streams), and with
 * cfg.image IMAGE fresh from seed_dict["image_representations"].  The kernels are then selected exactly as after
 * mdpp_upload_discrete_tables.  Synchronous.  What the config alone decides travels in mdpp_gen_params; is_term,
 * init_cdf and noise_cdf are the host tables of mdpp_upload_discrete_tables for ONE env (every env shares them). */
typedef struct {
    int32_t diameter, n_term, maximally_connected, repeats;   /* repeats = repeats_in_sequences */
    uint64_t total;             /* sequence numbers picked from: (A - n_term)^L with repeats, else prod(radices) per set */
    uint32_t n_sel;             /* picks per choice() call: int(reward_density * total), at least 1 */
    int32_t n_radices;          /* without repeats: L radices (A - n_term) - pos // diameter; with repeats 0 */
    uint32_t radices[16];
    const double *rews;         /* host: the unshuffled np.linspace(reward_dist[0], reward_dist[1], n_rews), n_rews > 1,
                                   or NULL: every value is 1.0 */
    uint32_t n_rews;
    int32_t image;              /* cfg.image (image_representations) */
    uint64_t *seed_dicts;       /* host out: uint64 [N][8] = the env seed, then the 7 entries of _SEED_KEYS; NULL: none */
} mdpp_gen_params;
int mdpp_generate_discrete(mdpp_env *h, const uint64_t *seeds_host, const mdpp_gen_params *params,
                           const uint8_t *is_term_host, const double *init_cdf_host, const double *noise_cdf_host);
/* The discrete tables as the kernels read them, in mdpp_upload_discrete_tables' layout (any pointer may be NULL;
 * asking for the reward table the handle does not keep is an error).  Synchronises the device. */
int mdpp_get_discrete_tables(mdpp_env *h, uint8_t *P_host, double *rtable_host, uint8_t *rbits_host,
                             uint8_t *is_term_host, double *init_cdf_host);

/* Irrelevant sub-space tables (host; shared by all envs or one set per env like the others):
 *   P_irr uint8 [T][S_irr][A_irr]   transition_function_irrelevant            rl_toy_env.py:1153-1228
 *   init_cdf_irr double[T][S_irr]   cumsum(irrelevant_init_state_dist) normalised  :1025-1037, :2260
 *   noise_cdf_irr double[S_irr][S_irr]  as noise_cdf, for the irrelevant P-noise  :2068-2076; NULL without noise */
int mdpp_upload_discrete_irrelevant(mdpp_env *h, const uint8_t *P_irr_host, const double *init_cdf_irr_host,
                                    const double *noise_cdf_irr_host);

/* Image templates (host): uint8 [S][n_radii][n_cls][tpl][tpl], polygon rasters centred in the
 * template; cls_x/cls_y int16 [S][n_radii][W or H] map a centre coordinate to its template class.
 * A centre whose polygon is CUT by the picture's edge (a quantised shift (v // q) * q rounds towards -inf and can leave the
 * draw's own range, image_multi_discrete.py:172-181) must be a class of its own whose template is cut the same way: the
 * specialised renderers apply Pillow's "source outside the picture reads 0" rule through the template alone
 * (mdp_playground_amd/image_obs.py _edge_clip; golden i_shq5_rot). */
int mdpp_upload_image_templates(mdpp_env *h, const uint8_t *tpl_host, int32_t n_radii, int32_t n_cls_x,
                                int32_t n_cls_y, const int16_t *cls_x_host, const int16_t *cls_y_host);

/* Continuous image observations: disc uint8 [(2 R + 1)][(2 R + 1)], non-zero = covered, R = cfg.img_r0:
 * the raster of Pillow's ellipse with the integer bounding box centre +- R (image_continuous.py:190-207). */
int mdpp_upload_image_disc(mdpp_env *h, const uint8_t *disc_host);
/* Grid envs with image observations additionally: lines uint8 [n_sub W][H], non-zero = white grid line
 * (Pillow's draw.line from the reference's end points, image_continuous.py:145-165); the terminal
 * cells drawn as rectangles ride in cfg.box_lo[2 b + d] (cell coordinates), cfg.n_boxes of them. */
int mdpp_upload_image_lines(mdpp_env *h, const uint8_t *lines_host);

/* RNG streams.  words_host: uint64 [num_envs][6] = PCG64 {state_lo, state_hi, inc_lo, inc_hi,
 * has_uint32, uinteger} exactly as numpy's bit_generator.state reports them. */
int mdpp_seed_streams(mdpp_env *h, int stream, const uint64_t *words_host);
int mdpp_get_streams(mdpp_env *h, int stream, uint64_t *words_host);
/* The same for fresh generators, computed on the device: stream i = PCG64(SeedSequence(seeds_host[i])), seeds below 2^64
 * (what mdp.new_generator(seed) starts from; no buffered half-word). */
int mdpp_seed_streams_seedseq(mdpp_env *h, int stream, const uint64_t *seeds_host);

/* reset(): mask_dev == NULL resets every env, else only envs with mask_dev[i] != 0.
 * obs_dev receives the new first observation of the reset envs (others untouched). */
int mdpp_reset(mdpp_env *h, const uint8_t *mask_dev, void *obs_dev, void *stream);

/* step(): actions int32[N] (discrete; int32[N][2] with cfg.irrelevant), float32[N][D]
 * (continuous) or int32[N][grid_dims] (grid); obs per cfg.obs_dtype ([N], [N][2] with
 * cfg.irrelevant, [N][D], [N][grid_dims] or [N][W][H]);
 * reward float32[N]; terminated/truncated uint8[N].
 * final_obs_dev (nullable): with same-step autoreset, the last observation of episodes that ended. */
int mdpp_step(mdpp_env *h, const void *actions_dev, void *obs_dev, float *reward_dev,
              uint8_t *terminated_dev, uint8_t *truncated_dev, void *final_obs_dev, void *stream);

/* K fused steps in one launch, per-env state held in registers between steps.
 * actions [K][N](…), outputs [K][N](…), time-major. */
int mdpp_step_n(mdpp_env *h, int K, const void *actions_dev, void *obs_dev, float *reward_dev,
                uint8_t *terminated_dev, uint8_t *truncated_dev, void *stream);

/* Closed-loop fused rollouts: a handle may carry ONE tabular policy, and mdpp_step_n_policy samples a ~ pi(. | s) in the
 * launch that steps the envs -- K steps of an agent acting on what it observes in one launch, nothing between steps.
 * The policy is a table of thresholds thr uint32 [S][A] with non-decreasing rows, thr[s][j] = ceil(cdf_s[j] 2^31) (so
 * thr[s][A-1] = 2^31), and a 64-bit seed.  Env i (global id g = cfg.env_id_offset + i) at step counter t (mdpp_tick; a
 * graph's tick offset applies) draws
 *   w = word (t & 3) of block 0 of the Philox4x32-10 stream (policy_seed, g, t >> 2, stream id 14), m = w >> 1,
 *   a = min(#{ j < A : thr[s][j] <= m }, A - 1) = searchsorted(cdf_s, m 2^-31, 'right'),
 * s the state the env is in (the last observation returned for it), and the step is mdpp_step_n's with that action;
 * actions_out_dev int32 [K][N] receives the actions (on the reset call of a next-step-autoreset env the action is drawn
 * and written, and ignored like a caller's).  The policy reads none of the env's streams: the launch leaves the handle
 * where mdpp_step_n fed with actions_out leaves it, whichever RNG mode, and the two kinds of launch mix freely.
 * Served: discrete handles with one shared MDP (num_tables = 1), S <= 255, L <= 7, no irrelevant sub-space, no image
 * observations, no episode_stats, no transition- or reward-noise key, tables + thresholds within 64 KiB of LDS; any
 * reward form, delay, every_n, autoreset mode and RNG mode.  Anything else: MDPP_EUNSUPPORTED with the reason in
 * mdpp_last_error, from mdpp_set_policy already; there is no other path.
 * mdpp_set_policy copies thr_dev (device) into a buffer of the handle ON `stream`: ordered behind the work queued there
 * and ahead of later launches, so a policy is replaced between rollouts without a host round trip.
 * mdpp_step_n_policy without a policy: MDPP_ESTATE.  mdpp_policy_kernel_name: as mdpp_kernel_name, for that launch. */
int mdpp_set_policy(mdpp_env *h, const uint32_t *thr_dev, uint64_t policy_seed, void *stream);
int mdpp_clear_policy(mdpp_env *h);
int mdpp_step_n_policy(mdpp_env *h, int K, int32_t *actions_out_dev, void *obs_dev, float *reward_dev,
                       uint8_t *terminated_dev, uint8_t *truncated_dev, void *stream);
const char *mdpp_policy_kernel_name(mdpp_env *h, int K);

/* In-kernel tabular TD learners: a discrete handle may carry ONE learner -- algo (MDPP_LEARN_*), float32 alpha in (0, 1], gamma
 * and epsilon in [0, 1], a 64-bit seed and one table Q float32 [S][A] PER ENV -- and mdpp_step_n_learn runs K steps of "select
 * epsilon-greedily from the env's own Q, step, update that Q" in one launch.  Env i (global id g = cfg.env_id_offset + i) at step
 * counter t (mdpp_tick; a graph's tick offset applies) in state s:
 *   sel(s, t): wE = word (t & 3) of block 0 of the Philox4x32-10 stream (seed, g, t >> 2, stream id 15); with
 *     E = ceil((double)epsilon 2^31), (wE >> 1) < E explores: a = (uint64(wA) A) >> 32, wA the same word of stream id 16;
 *     otherwise a = the lowest j maximising Q[s][j];
 *   the step is mdpp_step_n's with that action (transition and reward noise included): float32 reward r as written,
 *     terminated, truncated, the true next state s' (before any autoreset);
 *   target (float32, one rounding per operation): terminated: y = r; q_learning: y = r + gamma max_j Q[s'][j];
 *     sarsa: y = r + gamma Q[s'][a'], a' = sel(s', t + 1) on Q before this step's update;
 *   update: q = Q[s][a], d = y - q, u = alpha d, Q[s][a] = q + u;
 *   sarsa: when the env's next step of the same call starts from s' (no termination, no reset in between) it takes a' and does
 *     not select again; a call's first step always selects afresh -- the one departure from textbook SARSA: there is no
 *     per-env learner state besides Q;
 *   the reset call of a next-step-autoreset env: an action is selected from the state in the record, written and ignored;
 *     no update.
 * The learner reads none of the env's streams: the launch leaves the handle where mdpp_step_n fed with actions_out leaves it.
 * Non-finite Q: unspecified.
 * Served: discrete handles with one shared MDP, S <= 255, L <= 7, no irrelevant sub-space, no image observations, no
 * episode_stats, the MDP's tables within 64 KiB of LDS; any reward form, delay, every_n, max_episode_steps, autoreset mode,
 * RNG mode, with or without the transition- and reward-noise keys.  Anything else: MDPP_EUNSUPPORTED with the reason in
 * mdpp_last_error, from mdpp_set_learner already.
 * mdpp_set_learner (re)starts the learner: Q = q_init_dev ([N][S][A], device; copied on `stream`) or zeros.
 * mdpp_set_learner_rates changes alpha and epsilon only (no device work); the new values hold from the next launch on, for
 * every env alike -- rates that follow each env's own episode count are mdpp_set_learner_schedule's (Schedules, below).
 * mdpp_get_q / mdpp_set_q: device pointers, float32 [N][S][A], ordered on `stream`.  Without a learner: MDPP_ESTATE, as
 * mdpp_step_n_learn.  mdpp_learn_kernel_name: as mdpp_kernel_name, for that launch (QLDS=1: the tables are staged in LDS). */
int mdpp_set_learner(mdpp_env *h, int algo, float alpha, float gamma, float epsilon, uint64_t seed, const float *q_init_dev,
                     void *stream);
int mdpp_clear_learner(mdpp_env *h);
int mdpp_set_learner_rates(mdpp_env *h, float alpha, float epsilon);
int mdpp_step_n_learn(mdpp_env *h, int K, int32_t *actions_out_dev, void *obs_dev, float *reward_dev,
                      uint8_t *terminated_dev, uint8_t *truncated_dev, void *stream);
int mdpp_get_q(mdpp_env *h, float *q_out_dev, void *stream);
int mdpp_set_q(mdpp_env *h, const float *q_in_dev, void *stream);
const char *mdpp_learn_kernel_name(mdpp_env *h, int K);

/* Per-env learner hyper-parameters: alpha, gamma and epsilon are each either launch-uniform (mdpp_set_learner,
 * mdpp_set_learner_rates) or one float32 per env.  mdpp_set_learner_params takes HOST pointers to float32 [N]; NULL leaves
 * that parameter as it is (uniform or per-env).  Every element is range-checked like the scalar (alpha in (0, 1], gamma and
 * epsilon in [0, 1], NaN refused: MDPP_EINVAL, nothing changed); E[i] = ceil((double)epsilon[i] 2^31) is formed on the host;
 * the arrays are copied into buffers of the handle, ordered on `stream`.  Env i of the handle (its LOCAL index: only the
 * Philox streams use the global id) then learns with alpha[i], gamma[i], E[i]; everything else above holds word for word.
 * Without a learner: MDPP_ESTATE.  mdpp_set_learner makes all three uniform again, mdpp_set_learner_rates alpha and epsilon,
 * mdpp_set_learner_gamma (a new uniform gamma in [0, 1]; no device work) gamma.
 * While any parameter is per-env the launch is the kernel's PE form (the name gains ",PE=1"): the lane loads its three
 * values once per launch; the uniform parameters travel as arrays of equal entries.
 *
 * Double Q-learning (algo = MDPP_LEARN_DOUBLE_Q): TWO tables per env, QA and QB, float32 [S][A] each.
 *   sel(s, t): explore-or-not and the exploring action as above (stream ids 15, 16); greedy: the lowest j maximising
 *     QA[s][j] + QB[s][j] (one float32 addition per j, scanned from j = 0 with a strict >);
 *   wU = the tick's word of stream id 17 (same key and counter layout, the learner's seed): wU >> 31 == 0 updates A, else B.
 *     With X the updated table and Y the other: terminated: y = r; otherwise a* = the lowest argmax_j X[s'][j],
 *     y = r + gamma Y[s'][a*];  q = X[s][a], d = y - q, u = alpha d, X[s][a] = q + u (float32, one rounding per operation);
 *   nothing is carried from step to step; on the reset call of a next-step-autoreset env an action is selected, written
 *     and ignored, no update is made and that tick's wU is unused.
 * q_init_dev, mdpp_get_q and mdpp_set_q are float32 [N][2][S][A] for this algorithm (A first); [N][S][A] for the other two.
 * Served handles and refusals: as above.  The kernel's name gains ",DOUBLE=1"; QLDS=1 when a workgroup's 256 x 2 tables fit
 * in LDS beside the MDP's. */
int mdpp_set_learner_params(mdpp_env *h, const float *alpha, const float *gamma, const float *epsilon, void *stream);
int mdpp_set_learner_gamma(mdpp_env *h, float gamma);

/* Schedules: per-EPISODE epsilon and / or alpha.  A handle with a learner may carry one schedule: an epsilon table (float32 in
 * [0, 1]), an alpha table (float32 in (0, 1]) or both, each [R][M] with 1 <= M and R M <= MDPP_MAX_SCHEDULE_ENTRIES; a row index
 * row[i] in [0, R) per env (the handle's LOCAL index i, like the per-env parameters); and a counter ep[i], int32, in a buffer
 * of the handle -- zero when the schedule is set.  The epsilon table becomes thresholds on the host by the rule above:
 * T[r][e] = ceil((double)epsilon[r][e] 2^31).
 * In a learning launch (mdpp_step_n_learn, mdpp_step_n_learn_summary) env i starts with e = min(ep[i], M - 1),
 * E = T[row[i]][e] if epsilon is scheduled (else its own E, uniform or per-env), alpha = A[row[i]][e] if alpha is scheduled
 * (else its own).  Every selection made in a step -- the action, and sarsa's a' = sel(s', t + 1) inside its target -- uses the E
 * in force at the step's start, the update the alpha in force then.  AFTER the update of a step that is not the reset call
 * of a next-step-autoreset env: terminated or truncated moves ep[i] by one and E and alpha are looked up again -- exactly the
 * rule by which the summary's `episodes` moves.  The counter is stored when the launch ends.  So: with autoreset disabled
 * truncated stays set past max_episode_steps and the counter moves at every step, as `episodes` does; a sarsa action carried
 * over an episode's end was chosen under the old E; a reset call selects with the current E, writes the action, ignores it
 * and counts nothing; past M - 1 the last entry holds.  Behaviour of ep[i] beyond 2^31 - 1 is unspecified.
 * Everything else above holds word for word (stream ids 15 - 17, the twin property, pieces, QLDS).  mdpp_step_n_eval and its
 * summary form read neither table and do not move the counter.
 * mdpp_set_learner_schedule takes HOST pointers: epsilon and alpha [R][M] or NULL (one at least), row [N] or NULL when R == 1.
 * It validates (MDPP_EINVAL: nothing changed), forms the thresholds, copies on `stream` and zeroes the counters.  Without a
 * learner: MDPP_ESTATE.  On a handle with per-env noise levels in force or with mdpp_learner_per_env_mdp on:
 * MDPP_EUNSUPPORTED, "... an epsilon/alpha schedule with per-env noise levels / one MDP per env: not built", nothing changed;
 * while a schedule is in force mdpp_set_noise_levels and turning mdpp_learner_per_env_mdp on are refused with the same
 * reason, and what is in force stays.  mdpp_clear_learner_schedule drops it (the scheduled parameter is again what
 * mdpp_set_learner / _rates / _params made it); so do mdpp_set_learner and mdpp_clear_learner.  While epsilon is scheduled,
 * mdpp_set_learner_params with an epsilon and mdpp_set_learner_rates (which always carries one) are refused: MDPP_ESTATE,
 * the reason names mdpp_clear_learner_schedule; likewise alpha while alpha is scheduled.
 * mdpp_get_learner_episodes / mdpp_set_learner_episodes: the counters, int32 [N] DEVICE pointers, ordered on `stream`;
 * dev_in NULL zeroes them (the schedule starts again).  Without a schedule: MDPP_ESTATE.
 * The launch is the kernel's SCHED form, always with PE=1 (the name gains ",SCHED=1", last): the lane looks its values up at
 * the launch's start and at each of its episode ends, one dword load per scheduled table.
 * Under a graph: which tables are scheduled and M are carried by value; the tables, the rows and the counters are read from
 * the handle's buffers at replay, so a captured launch continues the schedule where the last launch left it, like Q.
 * Schedules together with per-env noise levels and / or one MDP per env: mdpp_learner_schedule_sweep(h, on) sets a flag of the
 * handle, off at creation.  With it off every call above returns exactly what it returns without the flag, the three "not
 * built" refusals included.  With it on those three refusals do not fire: mdpp_set_learner_schedule is accepted with levels
 * in force and / or mdpp_learner_per_env_mdp on, and while such a schedule is in force mdpp_set_noise_levels and turning
 * mdpp_learner_per_env_mdp on are accepted too (mdpp_noise_levels_per_env_mdp keeps its own rule).  The launch is then the
 * learner of that handle -- its step, stream ids 15 - 17, the level bytes, an env of transition_noise 0 making no
 * transition draw, every env's own tables, the LDS placements of the sections below -- with E and alpha taken from
 * (row[i], ep[i]) exactly as above: looked up at the launch's start, the counter moved and both looked up again after the
 * update of every step that ends an episode and is not a reset call, the clamp at M - 1, sarsa's a' chosen under the old E,
 * the counter stored when the launch ends.  The kernel's name gains ",SCHED=1" after everything else
 * ("...,PE=1[,DOUBLE=1][,NLEV=1][,PM=1|2],SCHED=1>"); the schedule has no LDS placement and changes none.  mdpp_step_n_eval and
 * its summary form read no table and move no counter.  Turning the flag off while a schedule is in force together with
 * levels or one MDP per env drops the schedule as mdpp_clear_learner_schedule does; otherwise turning it off changes nothing.
 * mdpp_set_learner and mdpp_clear_learner drop the schedule and leave the flag; turning mdpp_learner_per_env_mdp off drops the
 * learner and its schedule.  On a handle that is not discrete the call is accepted and changes nothing. */
int mdpp_set_learner_schedule(mdpp_env *h, const float *epsilon, const float *alpha, int R, int M, const int32_t *row, void *stream);
int mdpp_clear_learner_schedule(mdpp_env *h);
int mdpp_get_learner_episodes(mdpp_env *h, int32_t *dev_out, void *stream);
int mdpp_set_learner_episodes(mdpp_env *h, const int32_t *dev_in, void *stream);
int mdpp_learner_schedule_sweep(mdpp_env *h, int on);

/* Eligibility traces: SARSA(lambda) and Watkins's Q(lambda).  A handle with a q_learning or sarsa learner may carry traces: a
 * kind (MDPP_TRACE_ACCUMULATING or MDPP_TRACE_REPLACING), float32 lambda in [0, 1] -- uniform or one per env -- and one table Z
 * float32 [S][A] PER ENV, zeros when traces are set.  Everything in "In-kernel tabular TD learners" holds word for word -- sel,
 * stream ids 15 and 16, the step, the target y, sarsa's carry, the reset call -- except the update.
 * For a step that is not a reset call, with q = Q[s][a] read before anything is written, all arithmetic float32 with one
 * rounding per operation and no FMA: d = y - q and u = alpha d are formed first; c = gamma lambda is formed once, when the
 * lane's parameters are loaded.  Then, in order:
 *   1. cut (q_learning only): if this step's action came from the explore branch of sel ((wE >> 1) < E, whatever action that
 *      drew), every entry of Z becomes +0;
 *   2. mark: accumulating Z[s][a] = Z[s][a] + 1.0f; replacing Z[s][a] = 1.0f;
 *   3. sweep: for every entry e = 0 ... S A - 1 in ascending order, unconditionally: z = Z[e]; Q[e] = Q[e] + u z (the product
 *      is rounded, then the sum); Z[e] = c z;
 *   4. episode end: where the summary's `episodes` moves (terminated or truncated), Z becomes +0 for that env, after the sweep.
 * The reset call of a next-step-autoreset env selects an action, writes it and ignores it; it touches neither Q nor Z.
 * Z lives in a buffer of the handle, entry-major [S A][N] like Q: it crosses launches, the pieces of one call and graph
 * replays.  mdpp_step_n_eval and its summary form neither read nor write Z.  mdpp_set_learner and mdpp_clear_learner drop the
 * traces, as they drop a schedule; mdpp_set_q leaves Z alone.  Non-finite Q or Z: unspecified.  Denormal traces are kept, not
 * flushed.  With lambda = 0 and a Q that holds no -0 the launch equals the traceless learner's bit for bit (q + u 1 = q + u,
 * Q[e] + u 0 = Q[e]).
 * mdpp_set_learner_traces(h, kind, lambda, stream): allocates and zeroes Z (on `stream`), uniform lambda.  Without a learner:
 * MDPP_ESTATE; an unknown kind, a lambda outside [0, 1] or NaN: MDPP_EINVAL, nothing changed.
 * mdpp_set_learner_lambda takes a HOST pointer to float32 [N]: one lambda per env (the handle's LOCAL index), range-checked
 * like the other per-env parameters (NaN refused: MDPP_EINVAL, nothing changed), copied on `stream`; it forces the PE form as
 * mdpp_set_learner_params does (alpha, gamma and epsilon travel as arrays).  Without traces: MDPP_ESTATE.
 * mdpp_set_learner_traces makes lambda uniform again.  mdpp_clear_learner_traces drops the traces (the buffers stay).
 * mdpp_get_traces / mdpp_set_traces: device pointers, float32 [N][S][A], ordered on `stream`; without traces: MDPP_ESTATE.
 * mdpp_learner_traces: the kind in force, or 0.
 * Served: what mdpp_set_learner serves for q_learning / sarsa on one shared MDP -- uniform and per-env parameters, the
 * full-output, _summary and _log launches, a per-episode schedule on a shared-MDP handle.  Refused with MDPP_EUNSUPPORTED,
 * "... eligibility traces with <what>: not built", what is in force staying as it is: double_q; per-env noise levels; one
 * MDP per env; the schedule of mdpp_learner_schedule_sweep.  In both orders: mdpp_set_learner_traces on such a handle, and
 * mdpp_set_noise_levels, turning mdpp_learner_per_env_mdp on (a handle with one MDP per env) or mdpp_learner_schedule_sweep on
 * while traces are set.
 * The launch is k_discrete_trace_rollout / k_discrete_trace_summary (mdpp_learn_kernel_name names it, with PHILOX, NOISE, UNIT,
 * QLDS and, when present, ",PE=1" and ",SCHED=1"; the kind is a run-time field).  QLDS=1: Q and Z are both staged in LDS, entry e
 * of lane l at dword (256 e + l) of its table, and both written back when the launch ends; QLDS=0 when a workgroup's 256 x 2
 * tables do not fit beside the MDP's, or under MDPP_OPT_NO_LEARN_LDS: the same indexing on the two buffers.
 * Traces on one MDP per env: a lambda x seed sweep in one launch.  mdpp_learner_traces_per_env_mdp(h, on) sets a flag of the
 * handle, off at creation.  With it off every call returns exactly what it returns without the flag, the refusals above and
 * their messages included.  With it on AND mdpp_learner_per_env_mdp on, on a handle with cfg.num_tables == cfg.num_envs:
 * mdpp_set_learner_traces is accepted, and so are traces together with the schedule of mdpp_learner_schedule_sweep, in either
 * order (mdpp_learner_schedule_sweep / mdpp_set_learner_schedule while traces are set, mdpp_set_learner_traces while the flag
 * of the schedule is on).  Nothing else changes: env i learns bit for bit (outputs, Q, Z, state record, streams, status,
 * step counter) like env i of a handle with one shared MDP that has env i's table set, the same global env id
 * (env_id_offset + i) and the same traces -- the rule above word for word, cut, mark, sweep and episode end, around the step
 * of "One MDP per env"; the schedule's rules are those of mdpp_set_learner_schedule.  Still refused, with or without the flag
 * and in both orders: double_q; per-env noise levels (mdpp_noise_levels_per_env_mdp included); the schedule of
 * mdpp_learner_schedule_sweep on a handle with one shared MDP.
 * The launch is the PE form with PM != 0: "k_discrete_trace_rollout<PHILOX=.,NOISE=.,UNIT=.,QLDS=.,PE=1,PM=1|2[,SCHED=1]>"
 * (or _summary).  Placement per launch, never a refusal, by the rule of "One MDP per env" with Q and Z counted together
 * (256 x 2 S A floats per workgroup, at most 160 KiB): {Q + Z, slots}, {Q + Z}, {slots}, {} -- QLDS=1,PM=2; QLDS=1,PM=1;
 * QLDS=0,PM=2; QLDS=0,PM=1 -- the first one the device grants; Q and Z lie behind the slots and the shared noise cdf.
 * What clears the flag and the traces: the flag stays until it is turned off; turning it off, or turning
 * mdpp_learner_per_env_mdp off, on a handle with one MDP per env drops the traces (as mdpp_clear_learner_traces: the buffers
 * stay); mdpp_set_learner and mdpp_clear_learner drop the traces as ever and leave the flag; mdpp_clear_learner_traces leaves
 * the flag.  On a handle with one shared MDP, or one that is not discrete, the call is accepted and changes nothing.
 * Under a graph a captured launch reads every env's table set, Q and Z from the handle's buffers at replay. */
int mdpp_learner_traces_per_env_mdp(mdpp_env *h, int on);
int mdpp_set_learner_traces(mdpp_env *h, int kind, float lambda, void *stream);
int mdpp_set_learner_lambda(mdpp_env *h, const float *lambda, void *stream);
int mdpp_clear_learner_traces(mdpp_env *h);
int mdpp_get_traces(mdpp_env *h, float *z_out_dev, void *stream);
int mdpp_set_traces(mdpp_env *h, const float *z_in_dev, void *stream);
int mdpp_learner_traces(mdpp_env *h);

/* One MDP per env for the learner and evaluation launches.  mdpp_learner_per_env_mdp(h, on) sets a flag of the handle, off at
 * creation.  With the flag on, a handle with cfg.num_tables == cfg.num_envs (each env its own P, terminal states, rewardable
 * sequences and start distribution) is served by mdpp_set_learner, mdpp_step_n_learn, mdpp_step_n_eval, both _summary calls,
 * mdpp_get_q / mdpp_set_q, mdpp_set_learner_params / _rates / _gamma and the kernel-name dry runs: the "one shared MDP" rule
 * above is dropped and so is "within 64 KiB of LDS", which is about a shared MDP staged per workgroup; every other rule holds.
 * Env i steps bit for bit as env i of an identical handle given the same actions through mdpp_step_n, and agent i is the
 * learner above on table set i: sel, target, update, SARSA's carry, the reset call, summaries and evaluation hold word for
 * word; the Philox streams are keyed by cfg.env_id_offset + i as ever.
 * The launch is the kernel's PM form, always with PE=1 (uniform parameters travel as arrays of equal entries; mdpp_set_learner
 * allocates them on such a handle).  Where the tables live is a placement the host makes per launch, never a refusal: the
 * kernel's name ends ",PM=2>" when each lane's table set is staged into LDS (dword w of lane l at byte (256 w + l) 4: bank =
 * lane) and ",PM=1>" when lane i reads set i in global memory; QLDS says the same of the Q-tables.  Tried in this order, as
 * far as the device grants the LDS: Q and the MDPs, Q alone, the MDPs alone, neither (the MDPs are candidates while a
 * workgroup's 256 table sets take at most 64 KiB, the Q-tables at most 160 KiB).  MDPP_OPT_NO_PM_LDS forces PM=1,
 * MDPP_OPT_NO_LEARN_LDS QLDS=0.  The transition-noise cdf and the ziggurat tables stay shared.
 * On a handle with one shared MDP, or one that is not discrete, the call is accepted and changes nothing.  Turning the flag
 * off (on a handle it was on for) clears the learner.  Whatever the flag: mdpp_set_policy and mdpp_step_n_policy refuse one
 * MDP per env ("need one shared MDP"), and mdpp_set_noise_levels on a flagged handle with one MDP per env returns
 * MDPP_EUNSUPPORTED ("per-env noise levels on one MDP per env: not built") unless mdpp_noise_levels_per_env_mdp (below) has
 * opted in.  Without the flag such a handle is refused by every learner entry point as before, message included.
 * Under a graph capture the form (PM and QLDS) is fixed at capture like PE; the tables are read from the handle's buffers at
 * replay. */
int mdpp_learner_per_env_mdp(mdpp_env *h, int on);

/* Greedy evaluation of the learner's tables: mdpp_step_n_eval runs K steps in which env i in state s takes
 *   one table:  a = the lowest j maximising Q[s][j] (scanned from j = 0 with a strict >),
 *   double Q:   a = the lowest j maximising QA[s][j] + QB[s][j] (one float32 addition per j) -- the greedy branch of sel above,
 * and the step is mdpp_step_n's with that action (transition and reward noise included).  There is no exploration, no
 * target, no update and no carry: the tables are left bit for bit as they were, no word of stream ids 15, 16, 17 is used,
 * alpha, gamma and epsilon (uniform or per-env) are not read.  On the reset call of a next-step-autoreset env the action is
 * selected from the state in the record, written and ignored.  The launch leaves the handle where mdpp_step_n fed with
 * actions_out leaves it.  The handle needs a learner (any algorithm; MDPP_ESTATE without one); served handles and refusals
 * are mdpp_step_n_learn's.  To evaluate on a separate env, create a second handle and give it the tables (mdpp_get_q, then
 * q_init_dev or mdpp_set_q).  mdpp_eval_kernel_name: as mdpp_kernel_name, for that launch (QLDS=1: the tables are staged in
 * LDS, and not written back; DOUBLE=1: two tables per env).
 *
 * Episode summaries: mdpp_step_n_learn_summary / mdpp_step_n_eval_summary run the K steps of mdpp_step_n_learn / mdpp_step_n_eval
 * with the same effect on the handle (state, streams, step counter, tables) and write NO [K][N] array.  Instead they keep
 * five arrays of the caller, [N] each on the device -- ret float64, len int32 (the running episode's return and length),
 * episodes int32, return_sum float64, length_sum int32 (finished episodes: their count, the sums of their returns and
 * lengths).  Per env, in step order, for every step that is not the reset call of a next-step-autoreset env:
 *   ret += (double)r (r the float32 reward the full-output launch writes; one float64 addition);  len += 1;
 *   terminated or truncated:  episodes += 1;  return_sum += ret;  length_sum += len;  ret = 0;  len = 0.
 * A reset call changes nothing.  The launch loads the five values before its first step and stores them after its last:
 * the caller zeroes them (all five at an episode boundary it makes itself, mdpp_reset; the three sums when it has read
 * them).  Nothing of them is kept in the handle.  Without [K][N] arrays a call is one launch whatever K.
 *   The episode log: mdpp_step_n_learn_log is mdpp_step_n_learn_summary with three more arrays of the
 * caller and a capacity M >= 1 -- log_count int32 [N], the number of episodes this log has seen finish for env i (it goes on
 * counting past M); log_ret float64 [M][N] and log_len int32 [M][N], episode-major: entry [m][i] is the return and the length
 * of the m-th episode of env i that finished under this log.  Where the rule above finds terminated or truncated, BEFORE ret
 * and len are zeroed:
 *   if (count < M) { log_ret[count][i] = ret;  log_len[count][i] = len; }   (the values just added to return_sum / length_sum)
 *   count += 1;
 * ret is the float64 value added to return_sum.  Nothing else changes: the five summary values, env, streams, step counter,
 * tables, schedule counters and the kernel name the library reports are those of the same launch without a log (the launch
 * itself runs the form's k_discrete_learn_summary_log kernel, so that a launch WITHOUT a log runs the code it always ran).
 * There is no log for mdpp_step_n_eval_summary: a greedy evaluation ends episodes at nearly every step, and its log launch
 * did not beat the full-output launch; run the evaluation with full output where its episodes are wanted.  The lane loads log_count[i]
 * where it loads its five values and stores it where it stores them (no atomics); entries the launch does not write keep what
 * they held; a reset call writes nothing; the log never reads `episodes`, so zeroing the three sums does not disturb it.
 * Two consequences, both exact: a log and a summary zeroed together, the sums never zeroed in between, have
 * log_count == episodes and length_sum[i] == the sum of log_len[0 .. min(count, M) - 1][i] wherever count <= M; and the
 * left-to-right float64 sum of log_ret[0 .. count[i] - 1][i] equals return_sum[i] bit for bit for every env with
 * count[i] <= M.  Episode-major so that lanes of a wave finishing their m-th episode at one step store adjacent entries, and
 * "the mean over envs of episode m" is a contiguous row.  Served handles, forms and refusals are mdpp_step_n_learn_summary's, with the
 * same text; a null log pointer, M < 1 or M * num_envs > 2^31 - 1 is MDPP_EINVAL with a message, before any device work.
 * Nothing of a log is kept in the handle; after mdpp_reset the caller zeroes the five summary arrays (which hold the running
 * episode), the log's finished episodes stay valid.
 * mdpp_current_obs writes the observation each env shows now (what the last step or reset returned for it), taken from the
 * state record, to obs_dev [N] in the handle's observation type, ordered on `stream`: what a caller needs after a launch
 * that wrote no observations.  Served: the handles of mdpp_step_n_learn; and a continuous handle that has a linear policy
 * (mdpp_set_linear_policy): the state in every env's record as float32 [N][D]. */
int mdpp_step_n_eval(mdpp_env *h, int K, int32_t *actions_out_dev, void *obs_dev, float *reward_dev,
                     uint8_t *terminated_dev, uint8_t *truncated_dev, void *stream);
const char *mdpp_eval_kernel_name(mdpp_env *h, int K);
int mdpp_step_n_learn_summary(mdpp_env *h, int K, double *ret_dev, int32_t *len_dev, int32_t *episodes_dev,
                              double *return_sum_dev, int32_t *length_sum_dev, void *stream);
int mdpp_step_n_eval_summary(mdpp_env *h, int K, double *ret_dev, int32_t *len_dev, int32_t *episodes_dev,
                             double *return_sum_dev, int32_t *length_sum_dev, void *stream);
int mdpp_step_n_learn_log(mdpp_env *h, int K, double *ret_dev, int32_t *len_dev, int32_t *episodes_dev,
                          double *return_sum_dev, int32_t *length_sum_dev,
                          int32_t *log_count_dev, double *log_ret_dev, int32_t *log_len_dev, int M, void *stream);
int mdpp_current_obs(mdpp_env *h, void *obs_dev, void *stream);

/* Grid learners: one tabular TD agent per GRIDWORLD.  A grid handle with grid_dims == 2 may carry ONE learner -- algo
 * (MDPP_LEARN_Q_LEARNING or MDPP_LEARN_SARSA), n_actions (4 or 5), a 64-bit seed, float32 alpha[N] in (0, 1], gamma[N] and
 * epsilon[N] in [0, 1], and one table Q float32 [S][A] PER ENV -- and mdpp_step_n_grid_learn runs K steps of "select
 * epsilon-greedily from the env's own Q, step, update that Q" in one launch.  The parameters always travel as [N] arrays (a
 * uniform value is an array of equal entries: there is no separate uniform kernel form); env i of the handle (its LOCAL
 * index) learns with alpha[i], gamma[i], E[i] = ceil((double)epsilon[i] 2^31), formed on the host.
 *   State index: with (g0, g1) = grid_shape and the env in cell (c0, c1):  s = c0 (g1 + 1) + c1,  S = (g0 + 1)(g1 + 1).  The
 *     "+ 1": reset() draws floor(uniform(0, g + 1)) per coordinate, so the index g, one past the grid, occurs as an episode's
 *     first cell; the first move clips it away.
 *   Action index to vector: j < 4: d = j >> 1, component d is +1 if (j & 1) == 0 else -1, the other component 0; j == 4 (only
 *     with n_actions == 5): the all-zero noop.  In order: (+1,0), (-1,0), (0,+1), (0,-1)[, (0,0)].
 *   sel(s, t), the target, the update and sarsa's carried action are those of "In-kernel tabular TD learners" above, word for
 *     word: stream ids 15 and 16 keyed by (learner seed, global env id, t >> 2), word t & 3; (wE >> 1) < E[i] explores with
 *     a = (uint64(wA) A) >> 32; otherwise the lowest j maximising Q[s][j]; float32 arithmetic, one rounding per operation, no
 *     fused multiply-add.  r is the float32 reward as the launch writes it; terminated is the step's own terminated output,
 *     the latched target flag (with autoreset disabled it stays set and y = r from then on); s' is the cell after the move,
 *     before any autoreset; a truncation that resets drops sarsa's carry; a call's first step always selects afresh; on the
 *     reset call of a next-step-autoreset env an action is selected from the cell in the record, written and ignored, and
 *     nothing is updated.  Transition noise re-draws the move inside the env, from the env's own action stream: the learner
 *     still updates Q[s][a] for the a it chose.
 *   The learner reads none of the env's streams.  actions_out_dev is int32 [K][N][2], the action VECTORS taken: mdpp_step_n on
 *     an identically built handle, fed those vectors, writes the same observations, rewards, terminated and truncated and
 *     leaves the same state, streams, status words and step counter, bit for bit, in both RNG modes.
 *   Greedy evaluation (mdpp_step_n_grid_eval): K steps of the lowest argmax of Q[s]; nothing is drawn, nothing is updated,
 *     no parameter is read; the tables are left bit for bit as they were.
 *   The _summary forms run the same steps, write no [K][N] array and keep the caller's five [N] arrays by the rule of
 *     "Episode summaries" above.
 * Served: grid handles with grid_dims == 2; make_denser on or off; reward_every_n_steps, reward scale, shift and terminal
 * reward; max_episode_steps; the three autoreset modes; int64 or int32 observations; both RNG modes; the transition- and
 * reward-noise keys absent, at 0 or above 0.  Refused with MDPP_EUNSUPPORTED and the reason in mdpp_last_error, from
 * mdpp_set_grid_learner already: discrete and continuous handles ("grid learners serve grid envs only"),
 * irrelevant_features (grid_dims == 4), image observations, episode_stats, and tables of num_envs S A 4 bytes >= 2^32 (the
 * kernels address Q with 32-bit byte offsets).  Without a learner the launches and the Q accessors return MDPP_ESTATE
 * ("no learner set").
 * mdpp_set_grid_learner (re)starts the learner: alpha, gamma, epsilon are HOST pointers to float32 [N] (range-checked, NaN
 * refused: MDPP_EINVAL, nothing changed), Q = q_init_dev (float32 [N][S][A], DEVICE, copied on `stream`) or zeros when NULL.
 * mdpp_set_grid_learner_params: host [N] pointers, NULL keeps the current values; range-checked like
 * mdpp_set_learner_params, an error changes nothing.  mdpp_get_grid_q / mdpp_set_grid_q: device pointers, float32 [N][S][A],
 * ordered on `stream`.  mdpp_clear_grid_learner forgets the learner (the buffers stay for launches already queued).
 * Kernel: k_grid_learn_rollout<PHILOX,NOISE,QLDS,EVAL,SUMMARY>, one lane per env.  Q lives in the handle entry-major: entry
 * e = s A + j of env i at q[e N + i].  QLDS=1: each lane stages its table once per launch at q_lds[e 256 + tid] (bank = lane)
 * and, unless EVAL, writes it back after the last step -- taken when the device grants 256 S A 4 bytes of dynamic LDS beside
 * the kernel's static LDS (a 5 x 5 grid with 4 actions: 144 KiB); QLDS=0, or MDPP_OPT_NO_GRID_QLDS: the same indexing on the
 * buffer.  mdpp_grid_learn_kernel_name: as mdpp_kernel_name, for the launch of mdpp_step_n_grid_learn (eval == 0) or
 * mdpp_step_n_grid_eval, full output (summary == 0) or the _summary form; nothing is launched; empty without a learner. */
int mdpp_set_grid_learner(mdpp_env *h, int algo, int n_actions, uint64_t seed, const float *alpha, const float *gamma,
                          const float *epsilon, const float *q_init_dev, void *stream);
int mdpp_clear_grid_learner(mdpp_env *h);
int mdpp_set_grid_learner_params(mdpp_env *h, const float *alpha, const float *gamma, const float *epsilon, void *stream);
int mdpp_step_n_grid_learn(mdpp_env *h, int K, int32_t *actions_out_dev, void *obs_dev, float *reward_dev,
                           uint8_t *terminated_dev, uint8_t *truncated_dev, void *stream);
int mdpp_step_n_grid_eval(mdpp_env *h, int K, int32_t *actions_out_dev, void *obs_dev, float *reward_dev,
                          uint8_t *terminated_dev, uint8_t *truncated_dev, void *stream);
int mdpp_step_n_grid_learn_summary(mdpp_env *h, int K, double *ret_dev, int32_t *len_dev, int32_t *episodes_dev,
                                   double *return_sum_dev, int32_t *length_sum_dev, void *stream);
int mdpp_step_n_grid_eval_summary(mdpp_env *h, int K, double *ret_dev, int32_t *len_dev, int32_t *episodes_dev,
                                  double *return_sum_dev, int32_t *length_sum_dev, void *stream);
int mdpp_get_grid_q(mdpp_env *h, float *q_out_dev, void *stream);
int mdpp_set_grid_q(mdpp_env *h, const float *q_in_dev, void *stream);
const char *mdpp_grid_learn_kernel_name(mdpp_env *h, int K, int eval, int summary);

/* Grid learner schedules and the episode log.  The reference has no such agent: this text is the definition.
 * Schedule: a grid handle with a learner may carry one schedule -- an epsilon table (float32 in [0, 1]), an alpha table
 * (float32 in (0, 1]) or both, each [R][M] with 1 <= M and R M <= MDPP_MAX_SCHEDULE_ENTRIES; a row index row[i] in [0, R) per
 * env (the handle's LOCAL index i); and a counter ep[i], int32, in a buffer of the handle -- zero when the schedule is set.
 * The epsilon table becomes thresholds on the host: T[r][e] = ceil((double)epsilon[r][e] 2^31).
 * The kernel rules are those of "Schedules" above, word for word.  In mdpp_step_n_grid_learn, its _summary and its _log form
 * env i starts with e = min(ep[i], M - 1), E = T[row[i]][e] if epsilon is scheduled (else E[i]), alpha = A[row[i]][e] if alpha
 * is scheduled (else alpha[i]).  Every selection made in a step -- the action, and sarsa's a' = sel(s', t + 1) inside its
 * target -- uses the E in force at the step's start, the update the alpha in force then.  AFTER the update of a step that is
 * not the reset call of a next-step-autoreset env: terminated or truncated moves ep[i] by one and E and alpha are looked up
 * again -- exactly the rule by which the summary's `episodes` moves in this kernel.  So: with autoreset disabled the counter
 * moves at every step once a flag latches; a sarsa action carried over an episode's end was chosen under the old E; a reset
 * call selects with the current E, writes the action, ignores it and counts nothing; past M - 1 the last entry holds.  The
 * counter is stored when the launch ends.  gamma is never scheduled.  mdpp_step_n_grid_eval and its _summary form read no
 * table and move no counter.  Stream ids, the twin property and the placement of Q (QLDS) are unchanged: the schedule has no
 * LDS placement.  Behaviour of ep[i] beyond 2^31 - 1 is unspecified.
 * mdpp_set_grid_learner_schedule takes HOST pointers: epsilon and alpha [R][M] or NULL (one at least), row [N], NULL iff
 * R == 1.  It validates first (MDPP_EINVAL with a message: nothing changed), then forms the thresholds, copies on `stream`
 * and zeroes the counters.  ("Nothing changed" is promised for validation failures only: an MDPP_EHIP from an allocation or a
 * copy, after validation, may leave the handle without any schedule -- larger tables replace the old buffers first.)
 * mdpp_clear_grid_learner_schedule drops the schedule (the scheduled parameter is again what
 * mdpp_set_grid_learner / _params made it); so do mdpp_set_grid_learner and mdpp_clear_grid_learner.
 * mdpp_get_grid_learner_episodes / mdpp_set_grid_learner_episodes: the counters, int32 [N] DEVICE pointers, ordered on
 * `stream`; dev_in NULL zeroes them.  Without a learner the schedule calls and the counter accessors return MDPP_ESTATE
 * ("no learner set"); the counter accessors also without a schedule ("no schedule set").  On a handle that is not a grid:
 * MDPP_EUNSUPPORTED, "grid learners serve grid envs only".  While epsilon is scheduled mdpp_set_grid_learner_params with
 * an epsilon is MDPP_ESTATE, the reason names mdpp_clear_grid_learner_schedule, and nothing is changed (a gamma given in
 * the same call included); likewise alpha while alpha is scheduled.  gamma alone is always accepted.
 * Log: mdpp_step_n_grid_learn_log is mdpp_step_n_grid_learn_summary with three more arrays of the caller and a capacity
 * M >= 1 -- log_count int32 [N], log_ret float64 [M][N], log_len int32 [M][N], episode-major.  The rule is that of "The
 * episode log" above, word for word: where the summary rule finds terminated or truncated, BEFORE ret and len are zeroed,
 *   if (count < M) { log_ret[count][i] = ret;  log_len[count][i] = len; }      count += 1;
 * count goes on past M; the lane loads log_count[i] where it loads its five values and stores it where it stores them (no
 * atomics); entries the launch does not write keep what they held; a reset call writes nothing.  A null log pointer, M < 1
 * or M * num_envs > 2^31 - 1 is MDPP_EINVAL with a message, before any device work.  With a log, the env, the tables, the
 * five values and the schedule counters are those of the summary launch without one.  There is no log for the evaluation
 * launches (DESIGN.md 3.24 measured that decision on discrete handles).
 * Kernels: k_grid_learn_sched_rollout<PHILOX,NOISE,QLDS,SUMMARY> (a schedule in force, no log) and
 * k_grid_learn_log_rollout<PHILOX,NOISE,QLDS,SCHED> (a log, with or without a schedule): the step loop of
 * k_grid_learn_rollout with the lookup (one dword load per scheduled table at the launch's start and at each of the lane's
 * episode ends) and the log's two stores; a launch without schedule and log runs k_grid_learn_rollout, the code it always
 * ran.  QLDS is decided per kernel, on that kernel's own function.  mdpp_grid_learn_kernel_name keeps its signature and
 * its names: while a schedule is in force the learning forms' names gain ",SCHED=1" after "SUMMARY=."; evaluation names do
 * not change; a log launch reports the name of the same launch without a log. */
int mdpp_set_grid_learner_schedule(mdpp_env *h, const float *epsilon, const float *alpha, int R, int M, const int32_t *row, void *stream);
int mdpp_clear_grid_learner_schedule(mdpp_env *h);
int mdpp_get_grid_learner_episodes(mdpp_env *h, int32_t *dev_out, void *stream);
int mdpp_set_grid_learner_episodes(mdpp_env *h, const int32_t *dev_in, void *stream);   /* NULL: zeros */
int mdpp_step_n_grid_learn_log(mdpp_env *h, int K, double *ret_dev, int32_t *len_dev, int32_t *episodes_dev, double *return_sum_dev,
                               int32_t *length_sum_dev, int32_t *log_count_dev, double *log_ret_dev, int32_t *log_len_dev, int M, void *stream);

/* Grid noise levels.  The reference has no such handle: this text is the definition.
 * Any grid handle that mdpp_set_grid_learner serves (grid_dims == 2, no image observations, no episode_stats; a learner need
 * not be set) may carry per-env levels of its two noise keys: env i of the handle (its LOCAL index) steps with
 * transition_noise[i] and reward_noise[i] in place of the two creation values, in the learner and evaluation launches --
 * mdpp_step_n_grid_learn, mdpp_step_n_grid_eval, their _summary forms, mdpp_step_n_grid_learn_log, with or without a
 * schedule.  Levels are configuration of the handle: mdpp_set_grid_learner, mdpp_clear_grid_learner, the schedule calls,
 * mdpp_set_grid_q and the state accessors (mdpp_get_state_* / mdpp_set_state_*, the streams, the reset-pending flags)
 * neither carry nor disturb them.
 *   reward_noise[i]: float64, finite, >= 0; the handle must have been created with the reward_noise key, at any value
 *     including 0.  The env's noise term is  0.0 + reward_noise[i] * z,  z drawn exactly as without levels -- at
 *     reward_noise[i] == 0 too.
 *   transition_noise[i]: float64 in [0, 1] (-0.0 becomes 0.0), any number of distinct values (there is no per-level table);
 *     the handle must have been created with transition_noise > 0, which is what gives it an action stream.
 *     transition_noise[i] > 0: the env draws u from its env stream and re-draws the move where u < transition_noise[i],
 *     exactly as without levels.  transition_noise[i] == 0: NO u is drawn, lane by lane (the reference's
 *     `if self.transition_noise:`).  On numpy streams that env's env stream then moves only by its reward-noise normals and
 *     its action stream does not move, while its neighbours' do; on Philox streams the reward-noise normal then takes the
 *     first words of the tick's env stream.
 *   The equivalence: env i of such a handle equals, bit for bit, env i of a handle created uniformly with transition_noise[i]
 *     and reward_noise[i] and everything else equal, the global env id included -- for transition_noise[i] == 0 a handle
 *     created with transition_noise = 0, which has no such key.  "Equals": the outputs, the action vectors, Q, the state
 *     record, the words of the env, feature-space and action-space streams, the status word and the step counter.  Nothing
 *     else of "Grid learners" and "Grid learner schedules and the episode log" changes; evaluation still draws no learner
 *     word, and the env's noise is the lane's own.
 * While levels are set mdpp_step and mdpp_step_n return MDPP_ESTATE ("grid noise levels: learner and evaluation launches
 * only; clear_grid_noise_levels() first"); mdpp_reset is unaffected.  mdpp_set_noise_levels and its kin refuse a grid handle
 * as ever.
 * mdpp_set_grid_noise_levels takes HOST float64 [N] pointers; NULL: that key stays as it is (both NULL: MDPP_OK, nothing
 * changes).  Everything is validated before the handle is touched: MDPP_EUNSUPPORTED for a handle the grid learner does not
 * serve (mdpp_set_grid_learner's reasons), MDPP_ESTATE for a key the handle was not created with, MDPP_EINVAL for a value
 * out of range or not finite; the reason is in mdpp_last_error and nothing is applied.  The levels live in two float64 [N]
 * device buffers of the handle, allocated once and always both filled -- a key without levels holds its creation value --
 * and overwritten in place by later calls, ordered on `stream`.  mdpp_get_grid_noise_levels: the values in force (HOST
 * pointers, either may be NULL); while nothing is set the creation values, 0 for an absent key.
 * mdpp_clear_grid_noise_levels: back to the creation values and to the kernels launched before (the buffers stay for
 * launches already queued).
 * Kernels: k_grid_learn_nlev_rollout<PHILOX,QLDS,EVAL,SUMMARY>, k_grid_learn_nlev_sched_rollout<PHILOX,QLDS,SUMMARY> and
 * k_grid_learn_nlev_log_rollout<PHILOX,QLDS,SCHED> -- the step loop of k_grid_learn_rollout with NOISE = 1, in which the lane
 * loads its two float64 once per launch and keeps them in registers.  A launch without levels runs the kernels, and the
 * code, it ran before.  mdpp_grid_learn_kernel_name keeps its signature: while levels are set it reports
 * k_grid_learn_rollout<PHILOX=.,NOISE=1,QLDS=.,EVAL=.,SUMMARY=.,NLEV=1>, with ",SCHED=1" after "NLEV=1" under a schedule; a
 * log launch reports the name of the same launch without a log. */
int mdpp_set_grid_noise_levels(mdpp_env *h, const double *transition_noise, const double *reward_noise, void *stream);
int mdpp_get_grid_noise_levels(mdpp_env *h, double *transition_noise_out, double *reward_noise_out);
int mdpp_clear_grid_noise_levels(mdpp_env *h);

/* Linear policies: closed-loop CONTINUOUS rollouts.  The handle holds float32 parameters theta, one set shared by every env
 * ([D][D + 1]) or one per env ([N][D][D + 1]; per_env != 0): theta[.., r, c] for c < D is W[r][c], theta[.., r, D] is b[r]
 * (D = state_space_dim = action_space_dim).  At every step of a launch env i forms its action from o = the state in its
 * record -- the last observation returned for it; after a same-step reset the new episode's first state; on the reset call
 * of a next-step-autoreset env the ended episode's last state --:
 *   for r = 0 .. D-1:  acc = b[r];  for c = 0 .. D-1 in that order: acc = acc + W[r][c] * o[c]
 *                      a[r] = acc < -amax ? -amax : (acc > amax ? amax : acc),   amax = (float)action_space_max
 * every product and every sum rounded to float32, no fused multiply-add; a NaN acc stays NaN.  The step is mdpp_step_n's with
 * that action: a NaN component fails the admission test, the env stays and gets MDPP_STATUS_BAD_ACTION.  On the reset call of
 * a next-step-autoreset env the action is formed, written and ignored.  The policy reads no stream: mdpp_step_n on an
 * identically built handle, fed the actions mdpp_step_n_linear wrote, writes the same observations, rewards and flags and
 * leaves the same state, streams, status words and step counter, bit for bit.
 * Served: continuous handles with reward_function move_to_a_point, state_space_dim <= 12 and transition_dynamics_order <= 2,
 * no image observations and no episode_stats; every other field of the config as mdpp_step_n serves it.  Anything else is
 * MDPP_EUNSUPPORTED with the reason, from mdpp_set_linear_policy on.  Without a policy the launches return MDPP_ESTATE
 * ("no linear policy set").
 * mdpp_set_linear_policy copies theta_dev (DEVICE pointer, the caller's layout above) into the handle's entry-major buffer on
 * `stream`; mdpp_get_linear_policy writes it back in the layout it was given in.  mdpp_clear_linear_policy forgets it.
 * mdpp_step_n_linear: K steps in ONE launch; actions_out_dev float32 [K][N][D] receives the actions taken, the other four as
 * mdpp_step_n.  mdpp_step_n_linear_summary: the same K steps with no [K][N] output, keeping the caller's five [N] arrays by
 * the rule of "Episode summaries" above (reward: the float32 the full-output launch writes).
 * Kernels: k_continuous_linear_rollout / k_continuous_linear_summary<D,ORDER,PHILOX,NOISE,PLDS> (D, ORDER: the padded shape).
 * PLDS=1: every lane stages its D (D + 1) parameters once per launch in dynamic LDS (256 D (D + 1) 4 bytes per workgroup) and
 * reads them there at every step -- taken when the device grants that beside the kernel's static LDS; PLDS=0: they are read
 * from the buffer at every step (MDPP_OPT_NO_LINEAR_LDS forces it).  mdpp_linear_kernel_name: as mdpp_kernel_name, for the
 * launch of mdpp_step_n_linear (summary == 0) or mdpp_step_n_linear_summary; nothing is launched. */
int mdpp_set_linear_policy(mdpp_env *h, const float *theta_dev, int per_env, void *stream);
int mdpp_get_linear_policy(mdpp_env *h, float *theta_dev, void *stream);
int mdpp_clear_linear_policy(mdpp_env *h);
int mdpp_step_n_linear(mdpp_env *h, int K, float *actions_out_dev, float *obs_dev, float *reward_dev,
                       uint8_t *terminated_dev, uint8_t *truncated_dev, void *stream);
int mdpp_step_n_linear_summary(mdpp_env *h, int K, double *ret_dev, int32_t *len_dev, int32_t *episodes_dev,
                               double *return_sum_dev, int32_t *length_sum_dev, void *stream);
const char *mdpp_linear_kernel_name(mdpp_env *h, int K, int summary);

/* Linear policies with memory.  A linear policy has a HISTORY, 1 (the policy above, unchanged in every bit and kernel name) or 2.
 * With history = 2 theta is float32 [D][2 D + 1] (shared) or [N][D][2 D + 1] (per env): theta[.., r, c] = W[r][c] for c < D,
 * theta[.., r, D + c] = V[r][c] for c < D, theta[.., r, 2 D] = b[r]; entry number e = r (2 D + 1) + c, E = D (2 D + 1).
 * At every step env i reads o exactly as "Linear policies" defines it, and p:
 *   p = o  when the env's count of steps taken in its current episode -- word meta.x of its record,
 *          total_transitions_episode -- is 0 at the moment the action is formed;
 *   p = the env's MEMORY otherwise: the o it read the last time it formed an action.
 * After the action is formed the memory becomes o, on the reset call of a next-step-autoreset env too (where the action is
 * formed, written and ignored as above).  Per row
 *   acc = b[r];  for c = 0 .. D-1: acc = acc + W[r][c] * o[c];  then for c = 0 .. D-1: acc = acc + V[r][c] * p[c]
 * every product and every sum rounded to float32, no fused multiply-add; then the clamp and the NaN rule of "Linear policies".
 * The memory is a float32 [D][N] buffer of the handle.  It persists across launches.  Setting a history = 2 policy sets every
 * env's memory to its current state, and so does mdpp_set_state_continuous; mdpp_reset and a masked reset need nothing (the
 * step count is 0).  The policy reads no stream: the twin property of "Linear policies" holds as it stands.
 * mdpp_set_linear_policy_history: history = 1 is mdpp_set_linear_policy; history = 2 as above; anything else MDPP_EINVAL.  The
 * first history = 2 policy of a handle allocates the larger parameter buffer (it waits for the launches queued on the old one).
 * mdpp_linear_policy_history: the history of the policy in force (0: none).  mdpp_linear_memory: set == 0 writes the memory to
 * buf_dev as float32 [N][D], set != 0 replaces it from there, on `stream`; MDPP_ESTATE unless a history = 2 policy is in force.
 * Every launch, summary, search, ES and kernel-name entry point serves the handle as it stands: E and the act are those of the
 * history in force, and the [E][.] arrays of mdpp_linear_search and mdpp_linear_es are simply longer -- they are the CALLER's and
 * the library cannot see their size: after a change of history they must hold E rows for the history now in force (the normal of entry e is
 * the e-th draw of the same streams 18 and 19).  Kernels: the HIST = 2 forms of the six kernels, named with ",HIST=2" after
 * everything else (k_continuous_linear_rollout<D=4,ORDER=2,PHILOX=1,NOISE=0,PLDS=1,HIST=2>); PLDS is decided as before, on
 * 256 E 4 bytes.  The memory is not staged: the V pass reads it from the buffer and the act overwrites it, 8 D bytes per env step. */
int mdpp_set_linear_policy_history(mdpp_env *h, const float *theta_dev, int per_env, int history, void *stream);
int mdpp_linear_policy_history(mdpp_env *h);
int mdpp_linear_memory(mdpp_env *h, float *buf_dev, int set, void *stream);

/* Linear policy search: one (1+1)-ES per env on the linear policy, inside the launch.  Served: the handles of
 * mdpp_set_linear_policy that hold PER-ENV parameters [N][D][D + 1].  E = D (D + 1) entries, e = r (D + 1) + c (c == D: b[r]).
 * The CANDIDATE of env i -- the policy it acts with -- is the handle's own linear-policy buffer (mdpp_get_linear_policy reads
 * it); everything else is caller-owned DEVICE memory, one struct passed by pointer and copied by value at the call:
 *   best     float32 [E][N], entry-major (entry e of env i at best[e N + i]): the incumbent
 *   sigma    float32 [N]: step size per env, >= 0 and finite on entry
 *   score    float64 [N]: the incumbent's score, -inf at the start
 *   acc      float64 [N]: sum of the returns of the candidate's finished episodes in this trial
 *   ret      float64 [N]: running return of the candidate's current episode
 *   eps      int32 [N]: episodes finished in this trial
 *   trial    int32 [N]: index of the current trial, 0 at the start
 *   accepted int32 [N]: accepted trials
 *   by value: seed (u64), episodes_per_trial T >= 1, sigma_up, sigma_down, sigma_max (float32)
 * At every step that is not a reset call (the steps the summary rule counts), after the step's float32 reward rw is final:
 *   ret += (double)rw
 *   if terminated or truncated:
 *       acc += ret; ret = 0; eps += 1
 *       if eps == T:                                   -- the trial ends
 *           improved = (acc >= score)                  -- false for a NaN acc
 *           if trial > 0: sigma = improved ? min(sigma * sigma_up, sigma_max) : sigma * sigma_down      (float32)
 *           if improved: score = acc; best[e] = cand[e] for all e; accepted += 1
 *           trial += 1; acc = 0; eps = 0
 *           z[0 .. E-1] = the first E normals of Philox stream (seed, env_id_offset + i, tick = trial, stream id 18)
 *           cand[e] = best[e] + sigma * z[e]           -- float32 product, rounded, then float32 sum, rounded: no FMA
 * Trial 0 evaluates the start policy unperturbed; the caller initialises best from the handle's parameters, so a rejected
 * trial 0 (NaN return) leaves a defined incumbent.  The normals are Philox::normal() in sequence: float32 Box-Muller pairs of
 * words (0,1) then (2,3) of blocks 0, 1, ....  The search draws from this stream only, on numpy-stream and Philox handles
 * alike; the env's own streams are never read, so the twin property of "Linear policies" holds: mdpp_step_n on an identically
 * built handle, fed the actions the search launch wrote, gives the same outputs, state, streams, status words and step counter.
 * The new candidate acts from the next action on -- the formed, written and ignored action of a next-step-autoreset reset
 * call included.  With autoreset disabled the rule is driven by the flags of every step, as the summary rule is.  mdpp_reset
 * does not touch the arrays (a caller that abandons the running episode zeroes ret).
 * mdpp_step_n_linear_search: K steps in ONE launch, outputs as mdpp_step_n_linear.  mdpp_step_n_linear_search_summary: the same
 * K steps and the same search with no [K][N] output, keeping the caller's five summary arrays as mdpp_step_n_linear_summary.
 * Refusals: everything mdpp_step_n_linear refuses, with its text; no linear policy set: MDPP_ESTATE; a shared policy:
 * MDPP_EUNSUPPORTED ("the search needs one parameter set per env"); episodes_per_trial < 1, a null array, a non-finite or
 * negative sigma_up / sigma_down, a NaN or negative sigma_max (+inf: no clamp): MDPP_EINVAL.
 * Kernels: k_continuous_search_rollout / k_continuous_search_summary<D,ORDER,PHILOX,NOISE,PLDS>; the placement rule is the
 * linear kernels' (PLDS=1: the candidate staged in dynamic LDS, rewritten there at a trial end and written back to the buffer
 * after the last step for the lanes whose trial moved; PLDS=0: read and rewritten in the buffer; MDPP_OPT_NO_LINEAR_LDS forces
 * it).  The incumbent is touched at trial ends only.  mdpp_linear_search_kernel_name: as mdpp_linear_kernel_name. */
typedef struct mdpp_linear_search {
    float *best, *sigma;
    double *score, *acc, *ret;
    int32_t *eps, *trial, *accepted;
    uint64_t seed;
    int32_t episodes_per_trial;
    float sigma_up, sigma_down, sigma_max;
} mdpp_linear_search;
int mdpp_step_n_linear_search(mdpp_env *h, int K, const mdpp_linear_search *search, float *actions_out_dev, float *obs_dev,
                              float *reward_dev, uint8_t *terminated_dev, uint8_t *truncated_dev, void *stream);
int mdpp_step_n_linear_search_summary(mdpp_env *h, int K, const mdpp_linear_search *search, double *ret_dev, int32_t *len_dev,
                                      int32_t *episodes_dev, double *return_sum_dev, int32_t *length_sum_dev, void *stream);
const char *mdpp_linear_search_kernel_name(mdpp_env *h, int K, int summary);

/* Linear policy ES: one antithetic evolution strategy per 64 linear policies, inside the launch.  Served: the handles
 * mdpp_step_n_linear_search serves (per-env parameters, move_to_a_point, D <= 12, order <= 2) with N % 64 == 0; anything else
 * is MDPP_EUNSUPPORTED ("the ES needs whole groups of 64 envs"): a population is one full wave.
 * Group g is the local envs 64g .. 64g+63, G = N / 64.  Member m = i - 64g, pair p = m >> 1, sign s_m = +1 for even m and -1
 * for odd m.  E = D (D + 1), entry e = r (D + 1) + c, as in the search.
 * The CANDIDATE of env i is the handle's own linear-policy buffer, as in the search.  Everything else is caller-owned DEVICE
 * memory in one struct, passed by pointer and copied by value; nothing lives in the handle:
 *   mean     float32 [E][G], entry-major (entry e of group g at mean[e G + g]): the population means
 *   sigma    float32 [G]: perturbation scale per group, finite and > 0
 *   gain     float32 [G]: step per unit of rank-weighted sum (the binding: lr / (sigma * 4032) in float32; the kernel never divides)
 *   gen      int32 [G]: generation index
 *   acc      float64 [N]: summed return of the candidate's counted episodes
 *   ret      float64 [N]: running return of the current counted episode
 *   fitness  float64 [N]: each member's acc at the last generation end
 *   eps      int32 [N]: -1: waiting for an episode boundary; 0 .. T-1: counting; T: done, spare episodes ignored
 *   log_mean float64 [M][G], may be null with M = 0: mean member score of generation j in row j
 *   by value: seed (u64), episodes_per_member T >= 1, log_rows M
 * Per env, at every step that is not a reset call, after the step's float32 reward rw is final:
 *   if 0 <= eps < T:
 *       ret += (double)rw
 *   if the episode ended (terminated or truncated):
 *       if 0 <= eps < T:
 *           acc += ret; ret = 0; eps += 1
 *       elif eps == -1:
 *           eps = 0
 * Per group, after every step (once all 64 members have completed it, reset calls included) and before any member forms its
 * next action -- after the last step of a launch too --: if every member has eps == T, the generation ends:
 *   1. fitness[i] = acc.  The sort key is k_m = isnan(acc) ? -inf : acc.  Ties get the average rank, so that equal scores
 *      cancel within a pair:
 *        rank2_m = 2 #{j : k_j < k_m} + #{j != m : k_j == k_m}
 *        r_m = rank2_m - 63, an integer in [-63, 63].
 *   2. If gen < M: log_mean[gen][g] = (sum_m acc_m) * (1/64), the sum taken in float64 by the butterfly of point 3.  A NaN
 *      propagates.
 *   3. For each entry e in order:
 *        z0[e] = normal e of Philox stream (seed, env_id_offset + 64g + 2p, tick = gen, stream id 19) -- the even member's
 *                id, so both members of a pair read the same stream;  z1[e] = the same stream at tick gen + 1.
 *                The normals are Philox::normal() in sequence, as in the search.
 *        v_m = (float)r_m * (s_m > 0 ? z0 : -z0)            -- a float32 product
 *        S = the butterfly sum: for k = 0 .. 5: v = v + shfl_xor(v, 1 << k), in float32.  Float addition is commutative, so
 *            every lane ends with the same bits.
 *        mu = mean[e][g] + gain[g] * S                      -- the product rounded, then the sum rounded: no FMA
 *        t = sigma[g] * z1[e]
 *        cand_m[e] = s_m > 0 ? mu + t : mu - t
 *        member 0 stores mean[e][g] = mu
 *   4. gen += 1; acc = 0; ret = 0.  eps = 0 for a member whose step just completed was not a reset call and ended an
 *      episode; eps = -1 otherwise: a candidate is judged on whole episodes only.
 * The new candidates act from the next action on, the ignored action of a reset call included.
 * mdpp_linear_es_init writes the candidates of the current gen into the handle's buffer -- mean +- sigma z, z at tick = gen
 * (t = sigma z; s_m > 0 ? mean + t : mean - t) -- and sets acc = ret = 0 and eps = 0; one small kernel on `stream`.  Call it
 * after mdpp_reset; it is also how a search continues from saved arrays.
 * The ES reads no stream of the env: the twin property of "Linear policies" holds.  A member whose env stays in
 * MDPP_STATUS_BAD_ACTION (a NaN candidate) never ends an episode, so its group's generation stands still; the other groups go
 * on.  With autoreset disabled the rule follows every step's flags, as in the search.  mdpp_reset touches nothing.
 * mdpp_step_n_linear_es / mdpp_step_n_linear_es_summary: K steps in ONE launch, outputs as mdpp_step_n_linear /
 * mdpp_step_n_linear_summary.  Refusals: everything the search refuses, with its text; a shared policy or N % 64 != 0:
 * MDPP_EUNSUPPORTED; a null array (log_mean with M = 0 excepted), T < 1, M < 0: MDPP_EINVAL.  sigma and gain are the binding's
 * to validate.
 * Kernels: k_continuous_es_rollout / k_continuous_es_summary<D,ORDER,PHILOX,NOISE,PLDS>, the placement rule the search's
 * (MDPP_OPT_NO_LINEAR_LDS forces PLDS=0).  The cross-lane work is ballots and shuffles: no LDS, no barrier.
 * mdpp_linear_es_kernel_name: as mdpp_linear_kernel_name. */
typedef struct mdpp_linear_es {
    float *mean, *sigma, *gain;
    int32_t *gen;
    double *acc, *ret, *fitness;
    int32_t *eps;
    double *log_mean;
    uint64_t seed;
    int32_t episodes_per_member, log_rows;
} mdpp_linear_es;
int mdpp_linear_es_init(mdpp_env *h, const mdpp_linear_es *es, void *stream);
int mdpp_step_n_linear_es(mdpp_env *h, int K, const mdpp_linear_es *es, float *actions_out_dev, float *obs_dev,
                          float *reward_dev, uint8_t *terminated_dev, uint8_t *truncated_dev, void *stream);
int mdpp_step_n_linear_es_summary(mdpp_env *h, int K, const mdpp_linear_es *es, double *ret_dev, int32_t *len_dev,
                                  int32_t *episodes_dev, double *return_sum_dev, int32_t *length_sum_dev, void *stream);
const char *mdpp_linear_es_kernel_name(mdpp_env *h, int K, int summary);

/* Per-env noise levels for the learner and evaluation launches.  A handle mdpp_set_learner serves may give each env its own
 * reward-noise sigma and its own transition-noise probability; mdpp_step_n_learn, mdpp_step_n_eval and their _summary forms
 * then run ONE launch over all levels (the kernel's name gains ",NLEV=1"; the learner always in its PE form).
 * mdpp_set_noise_levels takes HOST pointers to float64 [N] (the handle's LOCAL env index); NULL leaves that key as it is.
 *   reward_noise[i]: finite, >= 0.  Env i's reward-noise term is 0.0 + reward_noise[i] z with z drawn exactly as without
 *     levels (at sigma 0 too).  Needs a handle created with has_reward_noise.
 *   transition_noise[i]: in [0, 1].  The distinct values, ascending, are the levels -- at most MDPP_MAX_NOISE_LEVELS; each env
 *     gets a level byte.  Per level p > 0: T = ceil(p 2^32) and M = ceil(2^64 (S - 1) / T) for Philox streams; for numpy streams
 *     the S categoricals' cdfs of rl_toy_env.py:1605-1612, and one uniform of the env's space stream per step.  p == 0:
 *     T = M = 0, NO draw: the space stream of that env does not move.  Needs a handle created with has_transition_noise.
 *   Env i then behaves bit for bit (outputs, tables, state record, env and space streams, step counter) like env i of a
 *   handle created with transition_noise[i] and reward_noise[i] and everything else equal.
 * Errors: MDPP_ESTATE for a handle mdpp_set_learner refuses or one created without the key, MDPP_EINVAL for a value out of
 * range, NaN, or more than MDPP_MAX_NOISE_LEVELS distinct transition levels (nothing changed; the reason: mdpp_last_error).
 * The arrays are copied into buffers of the handle, ordered on `stream` (the call also allocates the learner's per-env
 * parameter arrays when absent: a launch with levels takes the PE form, and no launch allocates).  While levels are set mdpp_step and mdpp_step_n
 * return MDPP_ESTATE ("per-env noise levels: learner and evaluation launches only; clear_noise_levels() first"); mdpp_reset is
 * unaffected.  mdpp_get_noise_levels writes the values in force (the creation values while nothing was set) to HOST float64
 * [N] arrays (NULL: not asked for).  mdpp_clear_noise_levels returns to the creation values and the launches the handle made
 * before.  Levels are configuration, not state: the state getters / setters neither carry nor disturb them. */
int mdpp_set_noise_levels(mdpp_env *h, const double *transition_noise, const double *reward_noise, void *stream);
int mdpp_get_noise_levels(mdpp_env *h, double *transition_noise_out, double *reward_noise_out);
int mdpp_clear_noise_levels(mdpp_env *h);

/* Per-env noise levels on one MDP per env: a noise x seed sweep in one launch.  mdpp_noise_levels_per_env_mdp(h, on) sets a
 * second flag of the handle, off at creation.  With it off, mdpp_set_noise_levels on a handle with cfg.num_tables != 1 returns
 * exactly what it returned before the flag existed (MDPP_ESTATE "need one shared MDP" without mdpp_learner_per_env_mdp,
 * MDPP_EUNSUPPORTED "... not built" with it).  With it on AND mdpp_learner_per_env_mdp on, mdpp_set_noise_levels proceeds: every
 * rule of the section above holds word for word (the values, the level bytes, sigma, (T, M), the limit of
 * MDPP_MAX_NOISE_LEVELS, the errors), and env i behaves bit for bit (outputs, Q-tables, state record, env and space streams,
 * status, step counter) like env i of a handle with the same table sets, created uniformly with transition_noise[i] and
 * reward_noise[i], that runs the per-env-MDP learner.  The per-level cdfs depend on S and p only: they stay one
 * [levels][S][S] table shared by the envs' MDPs.
 * The launch is the kernel's NLEV form with PM != 0; its name ends ",NLEV=1,PM=1>" or ",NLEV=1,PM=2>".  Placement per launch,
 * never a refusal: the Q-tables (at most 160 KiB, not under MDPP_OPT_NO_LEARN_LDS), the envs' MDP slots (at most 64 KiB, not
 * under MDPP_OPT_NO_PM_LDS) and the per-level cdfs (at most 32 KiB, numpy streams with the transition key only, not under
 * MDPP_OPT_NO_PM_NLEV_LDS) go to LDS in the first of these subsets the device grants: {Q, slots, cdfs}, {Q, slots}, {Q, cdfs},
 * {Q}, {slots, cdfs}, {slots}, {cdfs}, {}.  The handle's own shared cdf is not staged; the per-level cdfs lie in its place
 * (behind the slots for PM=2, at the start of dynamic LDS for PM=1), the Q-tables behind them.
 * On a handle with one shared MDP, or one that is not discrete, the call is accepted and changes nothing.  Turning this flag
 * off, or mdpp_learner_per_env_mdp off, on a handle with one MDP per env also clears the levels (mdpp_clear_noise_levels) and
 * this flag.  mdpp_step, mdpp_step_n and mdpp_set_policy refuse as in the two sections above. */
int mdpp_noise_levels_per_env_mdp(mdpp_env *h, int on);

/* Per-env internal state <-> host (synchronous; checkpoint / set_augmented_state).
 * Discrete: hist int32[N][L+1] (-1 = NaN slot), steps int32[N], ring double[N][delay].
 * Continuous: derivs float[N][order+1][D], cur float[N][D], steps int32[N],
 *             ring double[N][delay] + ring_is32 uint8[N][delay], reached uint8[N]. */
int mdpp_get_state_discrete(mdpp_env *h, int32_t *hist_host, int32_t *steps_host, double *ring_host);
int mdpp_set_state_discrete(mdpp_env *h, const int32_t *hist_host, const int32_t *steps_host,
                            const double *ring_host);
/* cfg.irrelevant: the irrelevant part of curr_state, int32[N] (curr_state[1], :2089) */
int mdpp_get_state_irrelevant(mdpp_env *h, int32_t *irr_host);
int mdpp_set_state_irrelevant(mdpp_env *h, const int32_t *irr_host);
/* Grid: cells int32[N][grid_dims], steps int32[N], reached uint8[N] (the latched target flag, :1776) */
int mdpp_get_state_grid(mdpp_env *h, int32_t *cells_host, int32_t *steps_host, uint8_t *reached_host);
int mdpp_set_state_grid(mdpp_env *h, const int32_t *cells_host, const int32_t *steps_host,
                        const uint8_t *reached_host);
int mdpp_get_state_continuous(mdpp_env *h, float *derivs_host, float *cur_host, int32_t *steps_host,
                              double *ring_host, uint8_t *ring_is32_host, uint8_t *reached_host);
int mdpp_set_state_continuous(mdpp_env *h, const float *derivs_host, const float *cur_host,
                              const int32_t *steps_host, const double *ring_host,
                              const uint8_t *ring_is32_host, const uint8_t *reached_host);
/* reward_function = move_along_a_line (rl_toy_env.py:1864-1910): the window of the line fit -- the relevant coordinates
 * of the last sequence_length states of every env, which the reference keeps in `augmented_state` and returns from
 * get_augmented_state() (:2147-2156) --, oldest first, float32 [N][L][n_rel] on the host; slots older than the running
 * episode are NaN like the reference's NaN-filled list.  mdpp_set_state_continuous on such a handle restores the step
 * counters but not this window: stepping is refused (MDPP_EUNSUPPORTED) until mdpp_set_line_history has been called
 * AFTER it (the slot of a state depends on the step counter).  ABI 7. */
int mdpp_get_line_history(mdpp_env *h, float *hist_host);
int mdpp_set_line_history(mdpp_env *h, const float *hist_host);

/* HIP graphs.  Single steps first (RLToyVectorEnv.step_graph).  mdpp_step hands the handle's step counter to its
 * launch by value (ring head = counter mod delay for delay lines kept in memory; Philox keys), so a captured
 * launch replays with the counter it was captured with.
 * mdpp_graph_replay_exact: 1 when a graph of K captured mdpp_step launches replays exactly for this handle
 * (numpy streams, and either no delay line in memory or K a multiple of the delay), 2 when it does through the
 * device-side offset below, < 0 on error (0, "does not": image observations keyed by the counter until round 4; no handle now).
 * mdpp_tick: adds `advance` (may be negative) to the step counter and returns the new value in *tick_out (may be
 * NULL): the capture advances the counter although nothing ran (take it back with -K), a replay runs K steps the
 * counter has not seen (add K). */
int mdpp_graph_replay_exact(mdpp_env *h, int K);
/* ABI 7 -- graphs that replay exactly for EVERY handle (Philox streams, any delay line; round 5: image observations too -- the
 * kernels that draw a step's image transforms read the same device word):
 * mdpp_graph_replay_exact returns 2 where a by-value capture would not be exact but this protocol is:
 *   mdpp_graph_capture(h, 1);  capture the K mdpp_step launches;  mdpp_graph_capture(h, 0);  mdpp_tick(h, -K, NULL);
 *   per replay:  mdpp_graph_set_tick_offset(h, counter_now - counter_at_capture, stream);  launch the graph on `stream`;
 *                mdpp_tick(h, K, NULL).
 * Launches made in capture mode add the device word that mdpp_graph_set_tick_offset writes to the step counter they
 * were captured with (ring head of a delay line in memory, Philox keys), first thing in the kernel. */
/* Fused and closed-loop launches in a graph (tests/test_gpu_graph_replay.py pins what follows, bit for bit against an eager
 * twin).  The protocol above holds for ANY launch of K steps in all -- mdpp_step_n, mdpp_step_n_policy, mdpp_step_n_learn,
 * mdpp_step_n_eval, the _summary forms, and calls that go out as several launches (image batches on the handle's side stream,
 * the pieces of a very long call): capture in capture mode, mdpp_tick(h, -K, NULL), and per replay the offset, the graph,
 * mdpp_tick(h, K, NULL).  Every step, rollout and closed-loop kernel reads the counter through the device word: the Philox
 * keys, the alignment of the launch inside a four-tick Philox block, the blocks it spans, the head of a delay line in memory.
 * Any number of eager launches of any kind may run between two replays; the offset need not be a multiple of 4 or of the delay.
 *   A CLOSED-LOOP launch replays exactly ONLY in capture mode, whatever the handle's RNG mode: the agent's streams (ids 14 - 17)
 *   are Philox streams keyed by the counter on every handle, so a by-value capture would repeat the same exploration words at
 *   every replay.  (Greedy evaluation draws none of them; it still needs capture mode for a Philox handle or a delay line in memory.)
 *   mdpp_graph_replay_exact speaks of mdpp_step launches only.
 *   BEFORE a capture make one eager launch of the same form on the same handle (same entry point, K, kernel options, agent,
 *   per-env parameters or noise levels in force): what a form's first launch sets up -- a kernel's dynamic-LDS attribute, the
 *   fill of the per-env parameter arrays with the uniform values, an image handle's pipeline -- then happens outside the
 *   capture.  No entry point named above allocates, synchronises or copies from the host; the setters (mdpp_set_policy,
 *   mdpp_set_learner*, mdpp_set_noise_levels, ...) may do all three and are not for a capture.
 *   What a captured launch carries BY VALUE (a replay uses what was in force at capture; change it and capture again): K and
 *   the caller's buffers, the kernel and its form (kernel options, the learner's algorithm, uniform or per-env parameters,
 *   levels or none, one MDP per env and where its tables are placed -- PM, QLDS and NLEV are fixed at capture), the policy's
 *   and the learner's seeds, the UNIFORM
 *   alpha, gamma and epsilon (mdpp_set_learner_rates / mdpp_set_learner_gamma after the capture do not reach a replay; an
 *   eager launch uses them), the NUMBER of noise levels and where their cdfs are staged.
 *   What it READS from the handle's buffers at replay (replace it between replays, on the replay's stream): the actions
 *   tensor of mdpp_step_n, the policy's thresholds (mdpp_set_policy with the same seed), the Q-tables (mdpp_set_q), the per-env
 *   alpha / gamma / epsilon arrays (mdpp_set_learner_params: the way to change rates under a graph), the per-env noise
 *   levels' values (mdpp_set_noise_levels with the same number of distinct transition levels), the caller's five summary
 *   arrays (they accumulate across replays), the env's state record, streams and tables.  Per-env noise levels on one MDP
 *   per env (mdpp_noise_levels_per_env_mdp) are no exception: the level bytes, sigma, the per-level cdfs and (T, M) and every
 *   env's table set are read from the handle's buffers at replay.  A schedule (mdpp_set_learner_schedule): which tables are
 *   scheduled and M go by value; the tables, the rows and the episode counters are read -- and the counters written -- at
 *   replay (mdpp_set_learner_schedule with the same tables given and the same M, or mdpp_set_learner_episodes, between replays).
 *   Eligibility traces (mdpp_set_learner_traces): the kind and the uniform lambda go by value; Z is READ AND WRITTEN in the
 *   handle's buffer at replay, like Q, so the traces cross replays as they cross launches (mdpp_set_traces between replays,
 *   on the replay's stream); per-env lambdas are read from their array at replay.  On one MDP per env
 *   (mdpp_learner_traces_per_env_mdp) every env's table set is read from the handle's buffers at replay as well.
 *   An episode log (mdpp_step_n_learn_log): the three log pointers and M go by value; log_count is read and written at replay and
 *   log_ret / log_len are written, so a log accumulates across replays like the five summary arrays.
 *   A linear policy (mdpp_step_n_linear / mdpp_step_n_linear_summary): shared or per-env parameters and their placement (PLDS)
 *   go by value; the parameter buffer is READ at replay (mdpp_set_linear_policy with the same per_env between replays, on the
 *   replay's stream).  The policy reads no stream, so only a Philox handle or a delay line in memory needs capture mode.
 *   A linear policy with memory (history = 2): the history goes by value too (the same history between replays); the memory
 *   buffer is READ AND WRITTEN at replay, in the search and ES launches alike, so p crosses replays as it crosses launches.
 *   The FIRST history = 2 policy of a handle frees the parameter buffer and allocates the larger one: every graph captured
 *   from a linear, search or ES launch of that handle before it holds the old address and must be captured again.
 *   A linear policy search (mdpp_step_n_linear_search / _summary): the struct travels BY VALUE -- the eight pointers, seed,
 *   episodes_per_trial and the three sigma factors are those of the capture --; the eight arrays and the handle's parameter
 *   buffer (the candidate) are READ AND WRITTEN at replay, so a search goes on across replays.  Its stream (id 18) is keyed by
 *   the trial index, not by the step counter: it needs capture mode no more than the linear policy does.
 *   A linear policy ES (mdpp_step_n_linear_es / _summary): likewise -- the nine pointers, seed, episodes_per_member and
 *   log_rows are those of the capture; the arrays and the candidates are read and written at replay; stream id 19 is keyed
 *   by the generation index.
 *   A grid learner (mdpp_step_n_grid_learn / mdpp_step_n_grid_eval and their _summary forms): algo, n_actions, the seed and
 *   the placement of the tables (QLDS, fixed at capture with the kernel options) go by value; Q is READ AND WRITTEN in the
 *   handle's buffer at replay (mdpp_set_grid_q between replays, on the replay's stream), the alpha / gamma / epsilon arrays
 *   are read from the handle's buffers at replay (mdpp_set_grid_learner_params: the way to change rates under a graph), and
 *   the step counter comes through the device offset, as for the discrete learner: the learning launch replays exactly
 *   only in capture mode, whatever the handle's RNG mode.
 *   A grid learner's schedule (mdpp_set_grid_learner_schedule): which tables are scheduled and M go by value; the tables, the
 *   rows and the episode counters are read -- and the counters written -- at replay.  Its episode log
 *   (mdpp_step_n_grid_learn_log): the three log pointers and the capacity go by value; log_count is read and written at
 *   replay and log_ret / log_len are written, so counters and log go on from replay to replay.
 *   Grid noise levels (mdpp_set_grid_noise_levels): "levels are set" goes by value -- a launch captured with levels replays
 *   the NLEV kernel whatever mdpp_clear_grid_noise_levels does later --; the two float64 [N] arrays are READ from the
 *   handle's buffers at replay, like Q and the parameter arrays (mdpp_set_grid_noise_levels between replays, on the
 *   replay's stream: the buffers are overwritten in place, never replaced).
 *   A handle must not be destroyed, and no other HIP call that synchronises may be made from the capturing thread, while a
 *   capture is open (a garbage-collected binding object's finaliser counts). */
int mdpp_graph_capture(mdpp_env *h, int on);
int mdpp_graph_set_tick_offset(mdpp_env *h, int64_t offset, void *stream);
int mdpp_tick(mdpp_env *h, int64_t advance, uint64_t *tick_out);

/* MDPP_AUTORESET_NEXT_STEP: the per-env flag "the episode ended on the previous call, the next call is the reset"
 * (gymnasium >= 1.0 vector envs; the reference itself never autoresets).  mdpp_get_state_* leave it out and
 * mdpp_set_state_* clear it; a checkpoint taken between the two calls carries it through these (uint8[N], host).
 * Call mdpp_set_reset_pending AFTER mdpp_set_state_*. */
int mdpp_get_reset_pending(mdpp_env *h, uint8_t *pending_host);
int mdpp_set_reset_pending(mdpp_env *h, const uint8_t *pending_host);

/* cfg.episode_stats: what the reference accumulates per env object and logs at every reset() (rl_toy_env.py:2231-2247,
 * cleared :2360-2369).  Rows of `current_host` (double [nk][N], the running episode): 0 total_abs_noise_in_reward_episode
 * (:1984), 1 total_reward_episode (:1985: the reward after the delay line and the every-n mask, before noise, scale and shift;
 * accumulated in float32 where the reference's reward is np.float32), 2 total_noisy_transitions_episode (discrete :1620, grid
 * :1746; 0 for continuous envs), 3 .. 3 + D - 1 total_abs_noise_in_transition_episode per dimension (continuous :1686);
 * nk = 3, or 3 + D for continuous envs.  `last_host` (double [nk + 1][N]): the same rows of the episode the latest reset()
 * of each env ended -- in-rollout autoresets and mdpp_reset alike -- and in row nk its total_transitions_episode.  Either
 * pointer may be NULL.  Synchronises the device. */
int mdpp_get_episode_stats(mdpp_env *h, double *current_host, double *last_host);

/* Kernel selection (see MDPP_OPT_*): disable_mask replaces the handle's current mask (0 = default dispatch). */
int mdpp_set_options(mdpp_env *h, uint32_t disable_mask);
/* Name (with template arguments) of the kernel mdpp_step_n(h, K, ...) would launch for this handle
 * right now -- K = 1: mdpp_step -- decided by the same code that launches it, nothing is launched.
 * Image handles: the renderer (the dominant kernel).  The string lives in the handle until the next call. */
const char *mdpp_kernel_name(mdpp_env *h, int K);

/* Philox-mode streams made visible (diagnostics, offline reproduction of the noise): out_dev[e][j]
 * (double, device) = the j-th standard normal of stream (seed, env_id0 + e, tick, stream id) -- a float32
 * Box-Muller pair per 64-bit draw, see mdp_playground_amd/csrc/mdpp_rng.hpp.  Runs on the current device.
 * (The reward noise of a DISCRETE env at tick t is normal t & 3 of stream (seed, env, t >> 2, 13): call with tick = t >> 2,
 *  stream = 13, n_per_env = 4.) */
int mdpp_philox_normals(uint64_t seed, int64_t env_id0, uint64_t tick, uint32_t stream, int32_t n_envs,
                        int32_t n_per_env, double *out_dev, void *hip_stream);

/* Per-env sticky status bits (MDPP_STATUS_*), cleared by the call. flags_host: uint32[N]. */
int mdpp_status(mdpp_env *h, uint32_t *flags_host);

/* Kernel timing with HIP events on the caller's stream (bench.py roofline leg):
 * begin/end bracket any number of launches; returns elapsed milliseconds. */
int mdpp_timer_begin(mdpp_env *h, void *stream);
int mdpp_timer_end(mdpp_env *h, void *stream, float *ms_out);

/* ---- peer-copy gather of the observation shards (ABI 7; SURVEY.md 8e "Collective") ----------------------------------
 * The path's one collective -- every rank gets the concatenated current-observation tensor -- as device-to-device copies
 * on the copy engines instead of a collective KERNEL: the rollout kernels hold every compute unit, so an RCCL all-gather
 * can only run between two launches, a copy engine runs beside them.  No counterpart in the reference (one process, one
 * env); `dist.PeerGatherer` is the binding, `ObsGatherer` (RCCL all_gather_into_tensor) stays the default and `value`.
 *   mdpp_peer_create   a buffer [slots][world][shard_bytes] on `device` (+ one 64-bit flag per slot and rank)
 *   mdpp_peer_handle   its hipIpcMemHandle_t (MDPP_PEER_HANDLE_BYTES bytes); exchange them over any channel
 *   mdpp_peer_open     maps the other ranks' buffers: `handles` = world x MDPP_PEER_HANDLE_BYTES bytes in rank order
 *   mdpp_peer_push     behind what `stream` has enqueued: shard_dev (shard_bytes on this device) -> row `rank` of slot
 *                      `slot` of EVERY rank's buffer, then `seq` into this rank's flag there (side stream of the handle)
 *   mdpp_peer_fence    `stream` waits (an event) until THIS rank's copies of the slot's latest push have left: the shard
 *                      buffer may be overwritten after that
 *   mdpp_peer_wait     `stream` waits until every rank's flag of `slot` is >= seq (a one-wave kernel polling device
 *                      memory, bounded: a timeout sets a status bit per missing rank -- mdpp_peer_status -- never hangs)
 *   mdpp_peer_buffer   device pointer of slot `slot`: [world][shard_bytes], rank-major = global env-id order */
#define MDPP_PEER_HANDLE_BYTES 64
typedef struct mdpp_peer mdpp_peer;
int mdpp_peer_create(int device, int world, int rank, size_t shard_bytes, int slots, mdpp_peer **out);
int mdpp_peer_handle(mdpp_peer *p, void *handle_out);
int mdpp_peer_open(mdpp_peer *p, const void *handles);
int mdpp_peer_push(mdpp_peer *p, int slot, const void *shard_dev, uint64_t seq, void *stream);
int mdpp_peer_fence(mdpp_peer *p, int slot, void *stream);
int mdpp_peer_wait(mdpp_peer *p, int slot, uint64_t seq, void *stream);
void *mdpp_peer_buffer(mdpp_peer *p, int slot);
int mdpp_peer_status(mdpp_peer *p, uint32_t *status_out, int *finegrained_out);
const char *mdpp_peer_last_error(mdpp_peer *p);
int mdpp_peer_destroy(mdpp_peer *p);

/* What the memory system of the current device gives plain streaming kernels (no handle; nothing of the reference):
 * `reps` launches of a 16-bytes-per-lane kernel over `nbytes` on `stream` (one 16 KiB tile per workgroup, tiles in address
 * order), HIP events around them -> *ms_out (all reps).  mode 0: copy src -> dst (2 x nbytes moved per launch; the float4
 * copy MI355X_MICROARCH.md measures at 6.29 TB/s), 1: fill dst (src unused), 2: read src (dst: a device pointer to 4 scratch
 * bytes); ABI 8: 3 = copy, 4 = fill with non-temporal stores.  bench.py prices `roofline.frac` beside the fastest form of
 * each (`peak_measured`). */
int mdpp_probe_hbm(int mode, void *dst_dev, const void *src_dev, size_t nbytes, int reps, void *stream, float *ms_out);
/* ABI 8.  The floor of the one-launch-per-step API on this device: n launches of an EMPTY kernel (`workgroups` x 64 threads)
 * back to back on `stream` -> the host's time per launch call and the device's time per launch (HIP events), microseconds.
 * bench.py reports mdpp_step beside it (`single_step.launch_floor`): below about 3.5 us per launch eager stepping is bound
 * by the host's launch call, not by the kernel. */
int mdpp_probe_launch(int n, int workgroups, void *stream, float *host_us_out, float *device_us_out);

/* ---- GymEnvWrapper-style post-processor ---------------------------------------
 * What the reference's mdp_playground/envs/gym_env_wrapper.py does around ANY inner env, for a batch of N
 * independent instances whose (obs, reward, done) the caller supplies as device tensors -- from
 * libmdpp_hip's own envs or from any other batched simulator.  Instance i is one GymEnvWrapper object:
 * one generator (the wrapper's _np_random, seeded by mdpp_post_seed_streams or a Philox stream), one reward
 * FIFO.  Replaces, per entry point:
 *   mdpp_post_actions   discrete action noise                                   gym_env_wrapper.py:354-366
 *   mdpp_post_step(_n)  continuous observation noise :367-373, :400-402; image canvas + shift :404-405,
 *                       :523-618; reward delay / flush on done / terminal reward / noise / scale / shift :407-432
 *   mdpp_post_reset     reset(): buffer refilled with zeros, image of the first observation :441-486
 * Rewards are float64 in and out (the reference computes them as Python floats).  Upstream's `done` branch
 * raises TypeError (list * float, :410); what is implemented is its evident numpy meaning, see INTEGRATION.md. */
typedef struct mdpp_post mdpp_post;
typedef struct {
    int32_t abi_version;        /* MDPP_ABI_VERSION */
    int32_t num_envs;
    int64_t env_id_offset;      /* global id of local instance 0 (Philox keys) */
    int32_t rng_mode;           /* MDPP_RNG_* */
    uint64_t philox_seed;
    int32_t continuous;         /* config["state_space_type"] == "continuous" */
    int32_t n_actions;          /* discrete: env.action_space.n */
    int32_t obs_dim, obs_f64;   /* continuous: length of an observation and its dtype (0 float32, 1 float64) */
    int32_t delay;              /* 0..128 */
    int32_t has_transition_noise; double transition_noise;   /* discrete: P(action replaced), continuous: std of the obs noise */
    int32_t has_reward_noise; double reward_noise;
    double reward_scale, reward_shift, term_state_reward;
    int32_t autoreset;          /* 1: the caller's env resets itself at done -> the buffer is refilled with zeros after a done step */
    /* image_transforms (discrete envs with uint8 [H][W][C] observations): canvas uint8 [W + 2 pad][H + 2 pad][C] */
    int32_t image, img_h, img_w, img_c, img_pad, img_has_shift, img_sh_quant;
} mdpp_post_config;
int mdpp_post_create(const mdpp_post_config *cfg, int device, mdpp_post **out);
void mdpp_post_destroy(mdpp_post *h);
const char *mdpp_post_last_error(const mdpp_post *h);
int mdpp_post_seed_streams(mdpp_post *h, const uint64_t *words_host);   /* uint64 [N][6], as mdpp_seed_streams */
int mdpp_post_get_streams(mdpp_post *h, uint64_t *words_host);
int mdpp_post_get_reward_buffer(mdpp_post *h, double *ring_host);       /* double [N][delay], [0] pays out next */
/* mask_dev NULL = every instance.  Image handles: obs_in uint8 [N][H][W][C] -> obs_out uint8 [N][W+2p][H+2p][C]
 * (instances outside the mask untouched); others: both NULL. */
int mdpp_post_reset(mdpp_post *h, const uint8_t *mask_dev, const void *obs_in_dev, void *obs_out_dev, void *stream);
/* the actions the inner envs receive: int32 [N] -> int32 [N] (may alias) */
int mdpp_post_actions(mdpp_post *h, const int32_t *actions_in_dev, int32_t *actions_out_dev, void *stream);
/* obs_in / obs_out: continuous float32|float64 [K][N][obs_dim]; image uint8 [K][N][H][W][C] -> [K][N][W+2p][H+2p][C];
 * otherwise NULL (observations pass through).  reward double [K][N], done uint8 [K][N] (terminated). */
int mdpp_post_step(mdpp_post *h, const void *obs_in_dev, const double *reward_in_dev, const uint8_t *done_dev,
                   void *obs_out_dev, double *reward_out_dev, void *stream);
int mdpp_post_step_n(mdpp_post *h, int K, const void *obs_in_dev, const double *reward_in_dev, const uint8_t *done_dev,
                     void *obs_out_dev, double *reward_out_dev, void *stream);
/* What mdpp_post_step_n(h, K, ...) would launch, as mdpp_kernel_name (nothing is launched; the string lives in the handle):
 * "k_post_step<PHILOX=.,RING=.,DC=.>" (RING 2: the reward FIFO in registers, its delay the constant DC; 1: in LDS; 0: in
 * HBM, or no delay), and for image handles " + " and the picture kernel, which mdpp_post_reset launches too:
 * "k_post_image_lds<LDS=bytes,PER_CU=workgroups>" (dynamic LDS per workgroup, workgroups per CU of its grid) or
 * "k_post_image" (the general form). */
const char *mdpp_post_kernel_name(mdpp_post *h, int K);

/* Episode statistics of a block of per-step outputs (what RLlib reports per training iteration and the reference's
 * callbacks write to the stats CSV, config_processor.py:275-407; mdp_playground_amd/stats_csv.py EpisodeStats): for
 * every instance the running return (double [N]) and length (int64 [N]) are carried through the K rows of
 * reward [K][N] (float32, or float64 when reward_is_f64) with end flags ended | ended2 (uint8 [K][N]; ended2 may be
 * NULL), and over the episodes that end inside the block *sum_ret, *sum_len, *count (device scalars) grow by the sum of
 * their returns, the sum of their lengths and their number.  Deterministic (no atomics).  scratch_dev: at least
 * 24 * ceil(N / 256) bytes.  Runs on the current device. */
int mdpp_episode_stats(int32_t K, int32_t N, const void *reward_dev, int32_t reward_is_f64, const uint8_t *ended_dev,
                       const uint8_t *ended2_dev, double *ret_dev, int64_t *len_dev, double *sum_ret_dev,
                       int64_t *sum_len_dev, int64_t *count_dev, void *scratch_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MDPP_H */
