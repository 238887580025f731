// Internal definitions shared by the translation units of libmdpp_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <type_traits>
#include <vector>

#include "../../include/mdpp.h"

namespace mdpp {

// Cache policy of the rollout kernels' OUTPUT stores (aux of the raw-buffer store builtins; 2 = nt).  Every
// output row is written once and never read by the kernel; left at the default policy the write-back
// traffic of these rows throttled the whole memory pipeline of the CU (cfg2 fused rollout: 147 -> 106 us
// per launch with nt, profiles/archive/r02_ablation_lean_kernel.txt).  NOT for the picture kernels: their 16-byte
// stores of whole pictures ran 0.51 -> 0.44 (polygon pictures) and 0.54 -> 0.18 (continuous pictures) with nt.
#ifndef MDPP_ST_NT
#define MDPP_ST_NT 2
#endif
constexpr int kBlock = 256;         // 4 wavefronts of 64 lanes; one lane per env instance
constexpr uint32_t kNoKey = 0xFFFFFFFFu;
constexpr uint32_t kRingPyZero = 0x7FC0DE1Au; // float32 ring slot holding Python's float 0.0
// Philox stream ids beyond the MDPP_STREAM_* indices (keys are (seed, env id, tick, stream id)):
constexpr uint32_t kPhiloxResetStream = 3;    // an explicit reset(), keyed by the reset tick
constexpr uint32_t kPhiloxIrrStream = 4;      // P-noise of the irrelevant sub-space
constexpr uint32_t kPhiloxActionStream = 5;   // grid: the re-drawn noisy action
// (6-8: the post-processor's streams, mdpp_post.hip)
constexpr uint32_t kPhiloxStartStream = 9;    // discrete: start state of an in-rollout reset, one word per tick (mdpp_rng.hpp)
constexpr uint32_t kPhiloxStartIrrStream = 10; // ... of the irrelevant sub-space
constexpr uint32_t kPhiloxPNoiseStream = 12;  // discrete: transition noise, one word per tick (mdpp_rng.hpp)
constexpr uint32_t kPhiloxRNoiseStream = 13;  // discrete: reward noise, one float32 normal per tick (four per block)
constexpr uint32_t kPhiloxPolicyStream = 14;  // discrete: the tabular policy's action, one word per tick, keyed by the POLICY's seed (mdpp_discrete_policy.hip)
constexpr uint32_t kPhiloxLearnExploreStream = 15; // discrete: the tabular learner's explore-or-not word, one per tick, keyed by the LEARNER's seed (mdpp_discrete_learn.hip)
constexpr uint32_t kPhiloxLearnActionStream = 16;  // ... and the word of its exploring action
constexpr uint32_t kPhiloxLearnUpdateStream = 17;  // ... double Q-learning: the word whose top bit says which table learns (0: A, 1: B)
constexpr uint32_t kPhiloxLinearSearchStream = 18; // continuous: the linear policy search's normals, keyed by the SEARCH's seed and the TRIAL index (mdpp_continuous_search.hip)
constexpr uint32_t kPhiloxLinearEsStream = 19;     // continuous: the linear policy ES's normals, keyed by the ES's seed, the PAIR's even env id and the GENERATION index (mdpp_continuous_es.hip)

// ---- per-episode noise statistics (cfg.episode_stats; general kernels only) ------------------------------------
// What the reference accumulates per env object and logs at every reset() (rl_toy_env.py:2231-2247; cleared
// :2360-2369): row 0 total_abs_noise_in_reward_episode (:1984), row 1 total_reward_episode (:1985: the reward after the
// delay line and the every-n mask, before noise / scale / shift), row 2 total_noisy_transitions_episode (discrete :1620,
// grid :1746), rows 3.. total_abs_noise_in_transition_episode per dimension (continuous :1686).  cur [nk][N] is the running
// episode, last [nk + 1][N] the episode a reset() ended (row nk: its total_transitions_episode).  cur == nullptr: off.
struct EpisodeStatsDev {
    double *cur, *last;
    int32_t nk;
};
__device__ __forceinline__ void est_add(const EpisodeStatsDev &e, long N, long i, int k, double v) {
    e.cur[(size_t)k * N + i] += v;
}
__device__ __forceinline__ void est_roll(const EpisodeStatsDev &e, long N, long i, uint32_t steps) {   // reset(): log, then clear
    for (int k = 0; k < e.nk; k++) {
        e.last[(size_t)k * N + i] = e.cur[(size_t)k * N + i];
        e.cur[(size_t)k * N + i] = 0.0;
    }
    e.last[(size_t)e.nk * N + i] = (double)steps;
}

// ---- discrete: kernel arguments (passed by value; wave-uniform => SGPRs) -------------------
struct DiscreteArgs {
    int32_t N;
    int32_t S, A, L, delay, every_n;
    int32_t shared_tables;      // 1: tables staged in LDS once per block; 0: one table set per env
    int32_t unit_rewards;       // reward table is a bitmask of keys, every reward = 1.0
    int32_t rew_sa;             // reward table keyed by (state, action) of the transition (custom reward matrix)
    int32_t has_p_noise, has_r_noise;
    int32_t autoreset, max_steps, obs_i32;
    int32_t philox;
    uint32_t pn_T;              // Philox streams: transition-noise threshold ceil(p 2^32) (mdpp_rng.hpp philox_pnoise_*)
    uint64_t pn_M, pn_M1;       // ... and ceil(2^64 (S - 1) / T) for the relevant / the irrelevant sub-space
    uint32_t nkeys;             // S^L
    uint32_t tick;              // head of the delay ring at this launch: env steps taken so far mod delay
    uint64_t ptick;             // env steps taken by this handle before this launch (Philox counter)
    const uint64_t *dtick;      // launches captured into a HIP graph: device word added to ptick at run time (tick_from_device)
    uint32_t opts;              // MDPP_OPT_* (host side: kernel selection only)
    uint64_t philox_seed;
    int64_t env_id_offset;
    double r_noise, scale, shift, term_add; // term_add = term_state_reward * reward_scale
    // tables (device)
    const uint8_t *P;           // [T][S][A]
    const double *rtable;       // [T][nkeys]      (unit_rewards == 0)
    const uint8_t *rbits;       // [T][rbits_stride] (unit_rewards == 1)
    const uint8_t *is_term;     // [T][S]
    const double *init_cdf;     // [T][S]
    const double *noise_cdf;    // [S][S]
    uint32_t rbits_stride;
    // LDS carve (byte offsets, 16-aligned), shared_tables only
    uint32_t lds_P, lds_term, lds_rew, lds_init, lds_noise, lds_bytes;
    uint32_t rew_in_lds, noise_in_lds;
    // per-env state (device)
    uint4 *state;               // {hist bytes 0-3, hist bytes 4-7, steps, ring bits}
    uint64_t *hist_hi;          // S > 255 (mdpp_discrete_wide.hip): states are 16-bit fields, the four oldest of the L + 1 live here; L > 7 (mdpp_discrete_long.hip): the eight oldest bytes
    uint32_t *ring_keys;        // [delay][N] keys awaiting payout (unit_rewards == 0)
    ulonglong2 *env_s, *env_inc, *sp_s, *sp_inc; // PCG64 streams
    uint32_t *status;
    EpisodeStatsDev est;
    // ---- irrelevant sub-space (cfg.irrelevant; general kernel only) ----
    int32_t irr, S1, A1;
    const uint8_t *P1;          // [T][S1][A1]
    const double *init_cdf1;    // [T][S1]
    const double *noise_cdf1;   // [S1][S1]
    uint32_t *irr_state;        // [N] irrelevant part of curr_state
    ulonglong2 *sp1_s, *sp1_inc; // observation_spaces[1] PCG64 streams
    // ---- precomputed on the host for the fused fast path (mdpp_discrete_fast.hip) ----
    uint32_t fast_ok;           // shape qualifies: shared LDS tables, unit rewards, no noise, L <= 3, S <= 16
    uint32_t shape_ok;          // fast_ok without its "numpy streams" condition (Philox handles: k_discrete_rollout_lean)
    uint32_t shape_ok_irr;      // the same shape with an irrelevant sub-space of at most 8 states (k_discrete_rollout_lean<IRR>)
    uint32_t shape_ok_noise;    // the lean shape (at most 8 states) with transition and / or reward noise on Philox streams (k_discrete_rollout_lean<..., NZ>)
    uint32_t lean_next_ok;      // ... with next-step autoreset (at most 8 states, with or without the irrelevant sub-space)
    uint32_t shape_ok_noise_np; // the lean shape with transition and / or reward noise on NUMPY streams (k_discrete_rollout_lean<..., PHILOX=0, NZ>)
    // transition noise on numpy streams, row-independent form of the S categoricals (:1604-1622): with m = r >> 11 the 53-bit
    // draw, the state re-drawn around table entry n is  min(a, n) + max(b - n, 0),  a = #{j <= S - 2 : pn_TL[j] <= r},
    // b = #{j <= S - 1 : pn_TU[j] <= r}  (thresholds pre-shifted by 11: compared with the 64-bit word itself).  Valid when
    // ceil(cdf_n[j] 2^53) is the same for every row n > j (TL) and for every row n <= j (TU): checked on the host, else
    // shape_ok_noise_np stays 0 and the general / quiet kernels search the row's own thresholds.
    uint64_t pn_TL[8], pn_TU[8];
    uint32_t s_shift;           // log2(S) when S is a power of two, else 0xFFFFFFFF
    uint32_t key_mask;          // S^L - 1 (power-of-two S)
    uint32_t spow;              // S^(L-1)
    uint64_t term_mask;         // bit s set <=> state s terminal (S <= 64)
    uint64_t init_thr[16];      // ceil(init_cdf[j] * 2^53): cdf[j] <= u  <=>  init_thr[j] <= (r >> 11)
    float rsel[4];              // reward for {paid*2 + terminal}, formed in float64 like :1987-1990,:2107
    uint64_t minv_lo, minv_hi;  // inverse of the PCG64 LCG multiplier mod 2^128 (un-drawing)
    // k_discrete_rollout_lean's LDS tables as one device blob (layout: kLeanTab* below), built once per upload by
    // k_lean_build_tables; nullptr: the handle is not one the lean launcher takes
    const uint4 *lean_blob;
};

// The lean rollout kernel's MDP tables, in 16-byte units of the blob (mdpp_discrete_lean.hip): the reward-bit table, the action
// columns, the rho_0 thresholds, the same two of the irrelevant sub-space, the reward values by (steps to the pay step, bit,
// terminated).  An instantiation without an irrelevant sub-space leaves units [kLeanTabCol1, kLeanTabRsel) out of its LDS copy.
constexpr uint32_t kLeanTabV = 0, kLeanTabCol = 512, kLeanTabT = 520, kLeanTabCol1 = 524, kLeanTabT1 = 532, kLeanTabRsel = 536,
                   kLeanTabUnits = 600;

// ---- discrete, one launch = one step (mdpp_discrete_step1.hip): everything the kernel reads, nothing else -- built once at
// mdpp_upload_discrete_tables (the caller's buffers are filled in per launch)
#ifndef MDPP_S1_REPLICAS
#define MDPP_S1_REPLICAS 1
#endif
// 1 KiB rounds of the wide one-step kernel's table blob that ONE wave stages into its LDS (k_discrete_step1w<NZ>: with a
// noise key / without): the upload refuses the one-step path for a longer blob, the launcher checks again
constexpr uint32_t kS1wRounds = 8, kS1wRoundsNoise = 12;
// copies of the one-step kernels' table blob (power of two), one per group of workgroups.  1: sixteen copies measured the
// same (S = 50: 4.07 against 4.04 us per step) -- 1 024 waves reading the same 4 KiB is not what made that launch slow, the
// compiler serialising the blob's loads was (mdpp_discrete_step1.hip)
constexpr int kS1Replicas = MDPP_S1_REPLICAS;
struct Step1Args {
    int32_t N;
    uint32_t A, S, L, every_n, max_steps, delay, autoreset;
    uint32_t term32;            // bit s: state s terminal (S <= 16)
    uint32_t nan_mask;          // 0xFF << 8 L: history byte L is the NaN test (:1822)
    uint32_t topup_rounds, topup_fill;   // start-state queue: at most this many rounds of one draw per lane after a step, up to this many entries
    float rsel[4];              // reward for {paid*2 + terminal} (DiscreteArgs::rsel)
    double inv_every_n;
    uint64_t ptick;             // Philox streams: env steps taken by this handle before this launch ...
    const uint64_t *dtick;      // ... plus this device word when the launch is replayed from a graph (tick_now)
    uint64_t philox_seed;
    int64_t env_id_offset;
    const uint4 *blob;          // 1 KiB: P columns as nibbles, rho_0 thresholds, reward bits (layout: mdpp_discrete_step1.hip)
    // k_discrete_step1w (any S <= 255 whose tables fit 8 KiB): byte offsets into the blob, its size in 1 KiB rounds
    uint32_t wide, blob_rounds, off_term, off_thr, off_thr31, off_rew, S8, off_bk;
    // ... with rewards that are not all 1.0 (reward_dist): a float64 table by sequence key at off_rew, the delay line of KEYS in HBM
    uint32_t unit, ring_head;   // ring_head: env steps taken so far mod delay (a graph replay: from ptick + *dtick)
    uint32_t *ring_keys;        // [delay][N]
    double scale, shift, term_add;
    // ... with transition and / or reward noise (k_discrete_step1w<..., NZ = true>): thresholds of the S noise categoricals
    // [S][S8] (numpy streams) at off_tn, numpy's ziggurat tables ki / wi / fi (3 x 2 KiB) at off_zig; the state space's stream
    uint32_t has_p_noise, has_r_noise, off_tn, off_zig, pn_T;
    uint64_t pn_M;
    double r_noise;
    ulonglong2 *sp_s;
    const ulonglong2 *sp_inc;
    const int32_t *actions;
    void *obs;
    float *reward;
    uint8_t *term, *trunc;
    void *final_obs;
    uint4 *state;
    ulonglong2 *env_s;
    const ulonglong2 *env_inc;
    uint32_t *status;
};

struct ContinuousArgs {
    int32_t N, D, n_rel, order, delay, every_n;
    int32_t make_denser, has_p_noise, has_r_noise, bounded;
    int32_t autoreset, max_steps, philox, n_boxes, rel_prefix;
    uint32_t tick;              // head of the delay ring at this launch: env steps taken so far mod delay
    uint64_t ptick;             // env steps taken by this handle before this launch (Philox counter)
    const uint64_t *dtick;      // launches captured into a HIP graph: device word added to ptick at run time (tick_from_device)
    uint32_t opts;              // MDPP_OPT_* (host side: kernel selection only)
    uint64_t philox_seed;
    int64_t env_id_offset;
    float inertia32, amax32, smax32, radius32, alw32, scale32, shift32, term_add32;
    float tpow32[MDPP_MAX_ORDER + 1];
    double fact[MDPP_MAX_ORDER + 1];
    double p_noise, r_noise, scale, shift, term_add, reset_lo, reset_range;
    int32_t rel[MDPP_MAX_DIM];
    float target[MDPP_MAX_DIM];
    float box_lo[MDPP_MAX_BOXES * MDPP_MAX_DIM];
    float box_hi[MDPP_MAX_BOXES * MDPP_MAX_DIM];
    // per-env state (device), struct-of-arrays: consecutive lanes -> consecutive addresses
    float *sd;                  // [order+1][D][N] state_derivatives
    float *cur;                 // [D][N] last returned (noisy, clipped) state
    uint2 *meta;                // {steps, flags: bit0 reached_terminal}
    uint32_t *ring;             // [delay][N] float32 bit patterns (kRingPyZero = Python 0.0)
    // reward_function move_along_a_line (0 = move_to_a_point): sequence_length, the last line_L states'
    // relevant coordinates [slot = s % line_L][line_NL][N] (s = transitions made when the state was
    // reached), and a float64 delay line (these rewards are Python floats)
    int32_t line_L;
    int32_t line_NL;            // row width of line_hist: 4 (at most 4 relevant dimensions) or 8
    int32_t line_lds;           // this launch mirrors the L points of every lane in dynamic LDS (set by launch_step_t)
    float *line_hist;
    double *line_ws;            // more than 8 relevant dimensions: the fit's matrices in HBM, [(2 n n + 3 n)][N] (c_line_reward_big); else null
    double *ring64;             // [delay][N]
    // the reference's DEFAULT target_point, float64 zeros over every dimension (:652-654): float64 distances, target
    // latch and dense reward; rew64 = the reward is float64 throughout (line reward, or default target + make_denser)
    int32_t target64, rew64;
    double radius;
    ulonglong2 *env_s, *env_inc, *sp_s, *sp_inc;
    uint32_t *status;
    EpisodeStatsDev est;
    // ---- precomputed on the host for the fused fast path (mdpp_continuous_fast.hip) ----
    int32_t park;               // helper waves park lanes that leave the ziggurat's fast path (mdpp_continuous_fast.hip)
    int32_t image_quirk;        // image observations: every step clips and zeroes the derivatives (see k_continuous_step C4)
    uint32_t fast_ok;           // PCG64, no hypercubes, relevant dims = a prefix, bounded, delay 0, every_n 1
    uint32_t inertia_pow2;      // inertia is a power of two: a / inertia == a * inv_inertia32 exactly
    float inv_inertia32;
    uint32_t fact_pow2_mask;    // bit k: k! is a power of two (k = 1, 2)
    double inv_fact[MDPP_MAX_ORDER + 1];
};

// A launch captured into a HIP graph replays with the argument values it was captured with -- the step counter among
// them (Philox keys; the head of a delay line kept in memory).  In capture mode (mdpp_graph_capture) the launches carry a
// pointer to a device word instead: the difference between the counter NOW and the counter at capture, written by
// mdpp_graph_set_tick_offset before a replay; every step / rollout kernel reads its counter through tick_now() /
// ring_head_now() (a wave-uniform scalar load).  (NOT by patching the argument struct inside the kernel: a write to a
// by-value kernel argument makes the compiler copy the whole struct to private memory -- the cfg2 rollout went from 129 to
// 195 us per launch with exactly that.)
template <class A>
__device__ __forceinline__ uint64_t tick_now(const A &a) { return a.ptick + (a.dtick ? *a.dtick : 0ULL); }
template <class A>
__device__ __forceinline__ uint32_t ring_head_now(const A &a, uint64_t ptick) {
    return a.dtick ? (a.delay > 0 ? (uint32_t)(ptick % (uint64_t)a.delay) : 0u) : a.tick;
}

// A kernel that asks for more than the default 32 KiB of dynamic LDS: raise its limit, and say whether the launch can go
// ahead (static + dynamic LDS within what a workgroup may have; the attribute call succeeded).  false = the caller takes
// its path without the LDS mirror.
inline bool dynamic_lds_ok(const void *kernel, size_t dyn_bytes) {
    if (dyn_bytes <= 32 * 1024) return true;
    hipFuncAttributes fa;
    if (hipFuncGetAttributes(&fa, kernel) != hipSuccess) { (void)hipGetLastError(); return false; }
    int dev = 0, max_lds = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (fa.sharedSizeBytes + dyn_bytes > (size_t)max_lds) return false;
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn_bytes) != hipSuccess) { (void)hipGetLastError(); return false; }
    return true;
}

// ---- grid (mdpp_grid.hip) ----
struct GridArgs {
    int32_t N, G;               // envs; state dimensions (2 or 4)
    int32_t shape[4], target[2];
    int32_t make_denser, has_p_noise, has_r_noise, every_n;
    int32_t autoreset, max_steps, obs_i32, philox;
    uint64_t ptick;             // env steps taken by this handle before this launch (Philox counter)
    const uint64_t *dtick;      // launches captured into a HIP graph: device word added to ptick at run time (tick_from_device)
    uint32_t opts;              // MDPP_OPT_* (host side: kernel selection only)
    uint64_t philox_seed;
    int64_t env_id_offset;
    double p_noise, r_noise, scale, shift, term_add;
    uint4 *state;               // {cells (one byte per dimension), steps, flags: bit0 reached target, -}
    ulonglong2 *env_s, *env_inc, *sp_s, *sp_inc, *act_s, *act_inc;
    uint2 *act_half;            // numpy's buffered 32-bit half of the action stream
    uint64_t minv_lo, minv_hi;  // inverse of the PCG64 LCG multiplier mod 2^128 (un-drawing queued reset cells)
    uint32_t *status;
    EpisodeStatsDev est;
};

} // namespace mdpp

// The handle.  Plain struct; all members are host-side bookkeeping + device allocations.
struct mdpp_env {
    mdpp_config cfg;
    int device;
    std::string err;
    uint64_t tick;              // env steps taken so far (ring head = tick mod delay; Philox counter)
    uint64_t reset_tick;        // reset() calls so far (Philox counter)
    uint32_t opts;              // MDPP_OPT_* kernel-selection switches (mdpp_set_options)
    char kname[192];            // mdpp_kernel_name()
    // device allocations
    void *d_P, *d_rtable, *d_rbits, *d_is_term, *d_init_cdf, *d_noise_cdf;
    void *d_state, *d_ring, *d_status;
    void *d_hist_hi;            // discrete, S > 255
    void *d_line_hist, *d_line_ws, *d_ring64;                             // continuous, move_along_a_line
    void *d_est_cur, *d_est_last;                             // cfg.episode_stats: EpisodeStatsDev rows
    int32_t est_nk;
    void *d_P1, *d_init_cdf1, *d_noise_cdf1, *d_irr_state;   // irrelevant sub-space
    bool irr_ready;
    bool graph_capture;         // mdpp_graph_capture(h, 1): launches take the step counter's offset from d_tick_off
    void *d_tick_off;           // uint64: counter now - counter at capture (mdpp_graph_set_tick_offset)
    bool line_hist_stale;       // move_along_a_line: set_state_continuous restored the step counters, the fit's window not yet
    void *d_sd, *d_cur, *d_meta;
    void *d_rng_s[MDPP_NUM_STREAMS], *d_rng_inc[MDPP_NUM_STREAMS], *d_rng_half;
    void *d_img_tpl, *d_img_tplp, *d_img_clsx, *d_img_clsy, *d_img_rot, *d_img_state_out, *d_img_state_final;
    void *d_img_near;           // fast renderer: table of the near dwords of a polygon (mdpp_image.hip render_fast_eval), or null
    void *d_img_rec;            // ImgRec [2][img_chunk][N] per-image records (mdpp_image.hip), 64 B each
    void *d_img_ctr;            // uint32 [2][2]: the fast renderer's work counters (scratch set x render launch)
    int32_t img_chunk;          // env steps per state-kernel + draw + render batch
    uint32_t imgc_disc_rows[32]; // continuous image observations: the disc raster, one bitmask per row
    void *d_imgc_boxes;          // ... and the terminal hypercubes / cells it draws: [n_boxes]{lo0, lo1, hi0, hi1} float32 (grid: {c0, c1, 0, 0})
    bool img_ready, img_fast_ok, img_lines_ready;   // img_fast_ok: k_image_obs<true> applies (mdpp_image.hip)
    int32_t img_n_radii, img_n_cls_x, img_n_cls_y;
    int32_t img_colb;            // fast renderer: 64 (k_image_obs_fast) or 128 (k_image_obs_wide) bytes of an LDS row per wave
    uint32_t nkeys, rbits_stride;
    bool tables_ready, streams_ready[MDPP_NUM_STREAMS];
    hipEvent_t ev0, ev1;
    // image rollouts: the next batch's state / draw / record kernels run on a side stream under the
    // rendering of the current batch (two scratch sets, events both ways; mdpp_capi.hip)
    hipStream_t side_stream;
    hipEvent_t ev_entry, ev_side[2], ev_render[2];
    mdpp::DiscreteArgs dargs;
    mdpp::Step1Args s1args;     // k_discrete_step1's argument block (blob == nullptr: the shape does not qualify)
    void *d_s1_blob;
    void *d_lean_blob;          // DiscreteArgs::lean_blob (kLeanTabUnits * 16 bytes)
    // the tabular policy of closed-loop rollouts (mdpp_set_policy): thresholds uint32 [S][A] on the device, the seed of its stream
    void *d_policy_thr;
    uint64_t policy_seed;
    bool policy_ready;
    // the tabular TD learner of mdpp_step_n_learn (mdpp_set_learner): one Q-table per env, entry-major float32 [S A][N]; the
    // sarsa action carried between the pieces of one call, int32 [N]
    void *d_learn_q, *d_learn_carry;
    uint64_t learn_seed;
    uint32_t learn_E;           // ceil(epsilon 2^31)
    float learn_alpha, learn_gamma;
    int32_t learn_algo;
    bool learn_ready;
    // double Q-learning keeps two tables, A then B: [2 S A][N] (learn_q_tables: how many the buffer was allocated for).
    // Per-env alpha / gamma / E (mdpp_set_learner_params): float32 / float32 / uint32 [N] on the device; learn_pe: which
    // parameters are per-env (bit 0 alpha, 1 gamma, 2 epsilon) -- any bit set: the launch takes the PE form and reads all
    // three arrays; learn_pe_stale: the arrays of these parameters do not hold the uniform value yet (filled on the stream
    // of the next launch)
    int32_t learn_q_tables;
    void *d_learn_alpha, *d_learn_gamma, *d_learn_E;
    uint32_t learn_pe, learn_pe_stale;
    // mdpp_learner_per_env_mdp: the learner and evaluation launches serve this handle's one MDP per env (their PM forms; only
    // ever set on a discrete handle with num_tables == num_envs != 1)
    bool learn_pm;
    // Per-env noise levels (mdpp_set_noise_levels; mdpp_discrete_closed.hpp NoiseLevelArgs): nl_on: the learner and evaluation
    // launches take their NLEV form and every other step launch is refused.  Device: the level byte and the sigma of every
    // env, the per-level cdfs [levels][S][S] and (T, M) pairs; host: the values in force, for mdpp_get_noise_levels.
    // nl_fill_*: the uniform alpha / gamma / E the learner's per-env arrays were last filled with for an NLEV launch.
    // nl_pm: mdpp_noise_levels_per_env_mdp -- levels are accepted on a handle with one MDP per env whose learn_pm is on (the
    // NLEV kernels with PM != 0; only ever set on a discrete handle with num_tables != 1)
    bool nl_on, nl_pm;
    int32_t nl_levels;
    void *d_nl_level, *d_nl_sigma, *d_nl_cdf, *d_nl_T, *d_nl_M;
    std::vector<double> nl_tn, nl_rn;
    bool nl_fill_valid;
    float nl_fill_alpha, nl_fill_gamma;
    uint32_t nl_fill_E;
    // Per-episode schedules of the learner (mdpp_set_learner_schedule; mdpp_discrete_learn.hpp SCHED): sched_on: the learning
    // launches take their SCHED form.  Device: the thresholds uint32 [R][M] and / or the alphas float32 [R][M] (sched_eps /
    // sched_alpha: which table is in force), every env's row int32 [N] and episode counter int32 [N]; sched_cap: the entries
    // the two table buffers were allocated for.  Like levels, a schedule makes the launch the PE form (nl_fill_*).
    // sched_sweep: mdpp_learner_schedule_sweep -- a schedule is accepted together with per-env noise levels and / or learn_pm
    // (the SCHED kernels with NLEV = 1 and / or PM != 0; only ever set on a discrete handle)
    bool sched_on, sched_eps, sched_alpha, sched_sweep;
    int32_t sched_R, sched_M;
    size_t sched_cap;
    void *d_sched_E, *d_sched_alpha, *d_sched_row, *d_sched_ep;
    // Eligibility traces of the q_learning / sarsa learner (mdpp_set_learner_traces; mdpp_discrete_trace.hpp): trace_kind
    // MDPP_TRACE_* or 0 (none) -- the learning launches take the trace kernels.  Device: one table Z per env beside Q,
    // entry-major float32 [S A][N], and every env's lambda float32 [N] (always filled: the PE form reads it, the uniform
    // form takes trace_lambda); per-env lambdas are bit 3 of learn_pe.
    // trace_pm: mdpp_learner_traces_per_env_mdp -- traces are accepted on a handle with one MDP per env whose learn_pm is on,
    // and together with the schedule of mdpp_learner_schedule_sweep there (the trace kernels with PM != 0; only ever set on a
    // discrete handle with num_tables != 1)
    int32_t trace_kind;
    float trace_lambda;
    bool trace_pm;
    void *d_trace_z, *d_trace_lambda;
    // the linear policy of closed-loop continuous rollouts (mdpp_set_linear_policy; mdpp_continuous_linear.hip): float32 parameters,
    // entry-major -- entry e = r (D + 1) + c of env i at [e N + i] (lin_per_env) or one shared set at [e]; allocated once for
    // N D (D + 1) entries
    void *d_lin_theta;
    bool lin_per_env, lin_ready;
    // a linear policy with memory (mdpp_set_linear_policy_history; mdpp_linear_history.hpp): lin_hist 1 or 2 -- E = D (lin_hist D + 1)
    // entries per policy, r (lin_hist D + 1) + c --, lin_cap the floats d_lin_theta was allocated for (N D (D + 1) until a
    // history = 2 policy is first set), d_lin_mem the memory p, float32 [D][N] in cur's layout, allocated with the first
    // history = 2 policy
    int lin_hist;
    size_t lin_cap;
    void *d_lin_mem;
    // the tabular TD learner of a GRID handle (mdpp_set_grid_learner; mdpp_grid_learn.hpp): one Q-table per env, entry-major
    // float32 [S A][N] with S = (g0 + 1)(g1 + 1), A = gl_A (4, or 5 with the noop); alpha / gamma / E always as [N] arrays on
    // the device; gl_cap: the entries per env the table buffer was allocated for
    void *d_gl_q, *d_gl_alpha, *d_gl_gamma, *d_gl_E;
    uint64_t gl_seed;
    int32_t gl_algo, gl_A;
    size_t gl_cap;
    bool gl_ready;
    // the grid learner's per-episode schedule (mdpp_set_grid_learner_schedule; mdpp_grid_learn.hpp SCHED): gl_sched_on: the
    // learning launches take their SCHED form.  Device: the thresholds uint32 [R][M] and / or the alphas float32 [R][M]
    // (gl_sched_eps / gl_sched_alpha: which table is in force), every env's row int32 [N] and episode counter int32 [N];
    // gl_sched_cap: the entries the two table buffers were allocated for
    bool gl_sched_on, gl_sched_eps, gl_sched_alpha;
    int32_t gl_sched_R, gl_sched_M;
    size_t gl_sched_cap;
    void *d_gl_sched_E, *d_gl_sched_alpha, *d_gl_sched_row, *d_gl_sched_ep;
    // Per-env noise levels of a grid handle (mdpp_set_grid_noise_levels; mdpp_grid_learn.hpp NLEV): gl_nl_on: the learner and
    // evaluation launches take their NLEV form and mdpp_step / mdpp_step_n are refused.  Device: every env's transition_noise
    // and reward_noise, float64 [N] each, allocated once and always both filled (a key without levels holds the creation
    // value); host: the values in force, for mdpp_get_grid_noise_levels
    bool gl_nl_on;
    void *d_gl_nl_p, *d_gl_nl_r;
    std::vector<double> gl_nl_tn, gl_nl_rn;
    mdpp::ContinuousArgs cargs;
    mdpp::GridArgs gargs;
};

namespace mdpp {
// Per-env discrete MDP generation (mdpp_generate.hip, mdpp_generate_discrete): what one lane needs for env e
struct GenArgs {
    int32_t S, A, L, diameter, n_term, maxc, repeats, unit;
    uint64_t total;             // sequence numbers picked from (per independent set without repeats)
    uint32_t n_sel;             // picks per draw
    uint32_t radix[16];         // without repeats: the digit radices, position 0 first
    const double *rews;         // device: the unshuffled reward_dist values (n_rews > 1), or null (every value 1.0)
    uint32_t n_rews;
    uint32_t nkeys, rbits_stride;
    const uint64_t *seeds;      // device [N]
    uint8_t *P;                 // [N][S][A]
    uint8_t *rbits;             // [N][rbits_stride] (unit) ...
    double *rtable;             // ... or [N][nkeys]
    uint64_t *sd;               // [N][8] seed dicts, or null
    ulonglong2 *env_s, *env_inc, *sp_s, *sp_inc, *im_s, *im_inc;   // PCG64 streams (null: not written)
    uint2 *im_half;
    uint64_t *scratch;          // [count][scratch_words]: bitset of `total` bits, picks, permutation of the values
    uint64_t scratch_words, set_words, perm_off;
};

// generator scratch per launch (sequence bitsets, picks, value permutations): envs go in chunks below this
constexpr size_t kGenScratchCap = (size_t)256 << 20;

// The checks of mdpp_gen_params against a handle's shape (S, A, L, image, unit rewards, nkeys, rbits stride) and the
// scalar fields of GenArgs they give; every pointer is left null for the caller.  MDPP_OK, or an error code with *err
// set.  Shared by mdpp_generate_discrete and the tests' host build of the generator, so both run one set of rules.
inline int gen_args_init(const mdpp_gen_params *p, int S, int A, int L, bool image, bool unit, uint32_t nkeys,
                         uint32_t rbits_stride, GenArgs &a, const char **err) {
    // the parameters must describe this handle's shape: every key and P entry the kernel writes is then in range
    const int d = p->diameter, n_term = p->n_term;
    const uint32_t nn = (uint32_t)(A - n_term);
    bool ok = d >= 1 && S == A * d && n_term >= 0 && n_term < A && p->n_sel >= 1 && p->n_sel <= p->total &&
              (p->image != 0) == image;
    if (ok && p->repeats) {
        uint64_t t = 1;
        for (int i = 0; i < L; i++) t *= nn;
        ok = p->total == t;
    } else if (ok) {
        uint64_t t = 1;
        ok = p->n_radices == L;
        for (int i = 0; ok && i < L; i++) {
            ok = p->radices[i] == nn - (uint32_t)(i / d) && p->radices[i] >= 1;
            t *= p->radices[i];
        }
        ok = ok && p->total == t;
    }
    const uint64_t n_seqs = (uint64_t)d * p->n_sel;
    if (ok && p->rews) ok = p->n_rews >= n_seqs && p->n_rews > 1;
    if (!ok) { *err = "generate_discrete: parameters do not match the handle"; return MDPP_EINVAL; }
    memset(&a, 0, sizeof(a));
    a.set_words = (p->total + 63u) / 64u;
    a.perm_off = a.set_words + (uint64_t)(p->repeats ? 1 : d) * p->n_sel;
    a.scratch_words = a.perm_off + (p->rews ? ((uint64_t)p->n_rews + 1u) / 2u : 0u);
    if ((size_t)a.scratch_words * 8u > kGenScratchCap) {
        *err = "generate_discrete: scratch per env above the cap";
        return MDPP_EUNSUPPORTED;
    }
    a.S = S; a.A = A; a.L = L; a.diameter = d; a.n_term = n_term; a.maxc = p->maximally_connected ? 1 : 0;
    a.repeats = p->repeats ? 1 : 0; a.unit = unit ? 1 : 0;
    a.total = p->total; a.n_sel = p->n_sel;
    for (int i = 0; i < 16; i++) a.radix[i] = p->repeats ? 0u : p->radices[i];
    a.n_rews = p->rews ? p->n_rews : 0u;
    a.nkeys = nkeys; a.rbits_stride = rbits_stride;
    return MDPP_OK;
}

// ---- host side: run-time values -> template arguments ------------------------------------------------------------
// with_bools(f, b0, b1, ...) calls f(c0, c1, ...) with ci = std::true_type / std::false_type for bi: inside the (generic)
// lambda ci() is a compile-time constant.  A launcher formats its kernel's name and instantiates the kernel from the SAME
// constants, in the same lambda, so the two cannot disagree; a combination that is not built is left out by an
// `if constexpr` inside the lambda.
template <class F> inline void with_bools(F &&f) { f(); }
template <class F, class... Bs> inline void with_bools(F &&f, bool b, Bs... rest) {
    if (b) with_bools([&](auto... cs) { f(std::true_type{}, cs...); }, rest...);
    else with_bools([&](auto... cs) { f(std::false_type{}, cs...); }, rest...);
}
// with_value<V0, V1, ...>(v, f) calls f(std::integral_constant<int, Vi>{}) for the Vi that equals v; false (f not called)
// when none does
template <int... Vs, class F> inline bool with_value(int v, F &&f) {
    return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}

// ---- what a step launch carries besides the handle's argument block -------------------------------------------------
// K steps x N envs, every array time-major.  name_out != nullptr: a dry run -- the launcher writes the name of the kernel
// it would launch (at most kNameLen bytes) and launches nothing
constexpr int kNameLen = 192;
// The episode summaries of a closed-loop launch that writes no [K][N] array (mdpp_step_n_learn_summary /
// mdpp_step_n_eval_summary): the caller's five [N] arrays on the device -- the running episode's return and length, the
// finished episodes' count and the sums of their returns and lengths.  With an episode log (mdpp_step_n_learn_log /
// mdpp_step_n_eval_log; log_cap == 0: none, the other three are not read) the caller's count [N] and the episode-major
// [log_cap][N] returns and lengths of the episodes that finished under it (include/mdpp.h "Episode summaries")
struct EpisodeSummaryArgs {
    double *ret;
    int32_t *len, *episodes;
    double *return_sum;
    int32_t *length_sum;
    int32_t *log_count;         // (no default member initialisers: with them EpisodeSummaryArgs{} is built field by field, and
    double *log_ret;            //  the kernels that take it as an unused default argument came out with other registers)
    int32_t *log_len;
    uint32_t log_cap;
};
template <class Act, class Obs>
struct StepIO {
    int K;
    const Act *actions;         // (the closed-loop launchers, mdpp_discrete_closed.hpp, WRITE the actions taken here)
    Obs *obs;
    float *reward;
    uint8_t *term, *trunc;
    Obs *final_obs;             // null: not asked for
    hipStream_t s;
    char *name_out;
    const EpisodeSummaryArgs *summary = nullptr;    // closed-loop launchers: not null = keep these, the five arrays above are unused
    // steps [k0, k0 + kc) of this launch: an env-step has act_elems action elements and obs_bytes bytes of observation
    StepIO piece(int k0, int kc, size_t N, size_t act_elems, size_t obs_bytes) const {
        const size_t off = (size_t)k0 * N;
        StepIO p = *this;
        p.K = kc;
        p.actions = actions + off * act_elems;
        p.obs = (Obs *)((char *)obs + off * obs_bytes);
        p.reward = reward + off; p.term = term + off; p.trunc = trunc + off;
        p.final_obs = final_obs ? (Obs *)((char *)final_obs + off * obs_bytes) : nullptr;
        return p;
    }
};
using DiscreteIO = StepIO<int32_t, void>;       // observations int32 or int64 (obs_i32); the grid's too
using ContinuousIO = StepIO<float, float>;
// (an irrelevant sub-space: action pairs, observation pairs)
inline DiscreteIO piece_of(const DiscreteArgs &a, const DiscreteIO &io, int k0, int kc) {
    const size_t w = a.irr ? 2 : 1;
    return io.piece(k0, kc, (size_t)a.N, w, w * (a.obs_i32 ? 4 : 8));
}
inline ContinuousIO piece_of(const ContinuousArgs &a, const ContinuousIO &io, int k0, int kc) {
    return io.piece(k0, kc, (size_t)a.N, (size_t)a.D, (size_t)a.D * sizeof(float));
}
// every step / rollout kernel takes (args, K, actions, obs, reward, term, trunc, final_obs)
template <class Kern, class A, class IO>
inline void launch_rollout(Kern kern, int grid, int block, size_t lds, const A &a, const IO &io) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), lds, io.s, a, io.K, io.actions, io.obs, io.reward, io.term, io.trunc,
                       io.final_obs);
}

// The per-launch fields of an argument block: the kernel-selection switches, the step counter (Philox keys), its device
// offset while launches are captured into a HIP graph, the head of the delay ring -- for a launch that starts k0 steps
// into this call
inline void stamp_piece(GridArgs &a, const mdpp_env *h, int k0) { a.ptick = h->tick + (uint64_t)k0; }
template <class A> inline void stamp_piece(A &a, const mdpp_env *h, int k0) {
    a.ptick = h->tick + (uint64_t)k0;
    a.tick = a.delay > 0 ? (uint32_t)(a.ptick % (uint64_t)a.delay) : 0u;
}
template <class A> inline void stamp_step(A &a, const mdpp_env *h) {
    a.opts = h->opts;
    a.dtick = h->graph_capture ? (const uint64_t *)h->d_tick_off : nullptr;     // (launches being captured into a HIP graph)
    stamp_piece(a, h, 0);
}
// The rollout kernels' buffer descriptors address < 4 GiB per array, so a long rollout goes out as several launches of at
// most kmax steps: body(piece, k0) launches one piece; false from it ends the loop (and is returned).  A dry run ends
// after the first piece: it names the launch.
template <class A, class IO, class Body>
inline bool for_each_piece(A &a, const mdpp_env *h, const IO &io, long long kmax, Body &&body) {
    for (int k0 = 0; k0 < io.K;) {
        const int kc = (int)((io.K - k0) < kmax ? (io.K - k0) : kmax);
        stamp_piece(a, h, k0);
        if (!body(piece_of(a, io, k0, kc), k0)) return false;
        if (io.name_out) return true;
        k0 += kc;
    }
    return true;
}
// After the launches of a step: the error check, then the handle's step counter
inline int step_done(mdpp_env *h, int K, const char *kernel) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { h->err = std::string(kernel) + " launch: " + hipGetErrorString(e); return MDPP_EHIP; }
    h->tick += (uint64_t)K;
    return MDPP_OK;
}

// implemented in the kernel translation units
int launch_discrete_step(mdpp_env *h, const DiscreteIO &io);
int launch_discrete_reset(mdpp_env *h, const uint8_t *mask, void *obs, hipStream_t s);
// state spaces of 256 ... 65 535 states: the general kernel alone, 16-bit table entries and history fields (mdpp_discrete_wide.hip)
int launch_discrete_step_wide(mdpp_env *h, const DiscreteIO &io);
int launch_discrete_reset_wide(mdpp_env *h, const uint8_t *mask, void *obs, hipStream_t s);
// sequence_length 8 ... 15: the same with a history of sixteen byte fields (mdpp_discrete_long.hip)
int launch_discrete_step_long(mdpp_env *h, const DiscreteIO &io);
int launch_discrete_reset_long(mdpp_env *h, const uint8_t *mask, void *obs, hipStream_t s);
bool launch_discrete_fast(const DiscreteArgs &a, const DiscreteIO &io);
int launch_continuous_step(mdpp_env *h, const ContinuousIO &io);
int launch_continuous_reset(mdpp_env *h, const uint8_t *mask, float *obs, hipStream_t s);
bool launch_discrete_step1(const DiscreteArgs &d, const Step1Args &proto, const DiscreteIO &io);
bool launch_discrete_quiet(const DiscreteArgs &a, const DiscreteIO &io);
bool launch_discrete_pipe(const DiscreteArgs &a, const DiscreteIO &io);
bool launch_discrete_lean(const DiscreteArgs &a, const DiscreteIO &io);
// the tables of `a` as the lean kernel's LDS image, into blob (kLeanTabUnits * 16 bytes); a.lean_blob itself is not read
hipError_t launch_lean_build_tables(const DiscreteArgs &a, void *blob, hipStream_t s);
bool launch_continuous_fast(const ContinuousArgs &a, const ContinuousIO &io);
bool launch_continuous_step1(const ContinuousArgs &a, const ContinuousIO &io);
bool launch_continuous_line(const ContinuousArgs &a, const ContinuousIO &io);
int launch_imagec_obs(mdpp_env *h, int K, const void *states, const void *final_states, const uint8_t *term,
                      const uint8_t *trunc, const uint8_t *mask, uint8_t *img_out, uint8_t *img_final, hipStream_t s);
// closed-loop rollout under the handle's tabular policy (mdpp_discrete_policy.hip; the step and the launcher they share:
// mdpp_discrete_closed.hpp): why the handle has none (empty: it is served); io.K steps, the sampled actions written to
// io.actions
std::string discrete_policy_refusal(const mdpp_env *h);
int launch_discrete_policy(mdpp_env *h, const DiscreteIO &io);
// io.K steps of the handle's tabular learner (mdpp_discrete_learn.hip), as above; Q between the caller's [N][S][A] and the
// handle's entry-major buffer
std::string discrete_learn_refusal(const mdpp_env *h);
int launch_discrete_learn(mdpp_env *h, const DiscreteIO &io);
int launch_learn_q_copy(mdpp_env *h, float *user_q, bool to_handle, hipStream_t s);
// (the learner's forms -- per-env hyper-parameters, double Q-learning, episode summaries with io.summary, per-env noise
// levels, one MDP per env -- are instantiations of mdpp_discrete_learn.hpp's launch_learn_form, one translation unit each
// (mdpp_discrete_learn_*.hip); launch_discrete_learn picks the handle's)
// ... of a learner with eligibility traces (h->trace_kind != 0; mdpp_discrete_trace.hip, the forms: mdpp_discrete_trace.hpp,
// one translation unit each); launch_discrete_learn hands such a handle on after filling the per-env arrays.  Z between the
// caller's [N][S][A] and the handle's entry-major buffer
int launch_discrete_trace(mdpp_env *h, const DiscreteIO &io, bool pe);
int launch_trace_z_copy(mdpp_env *h, float *user_z, bool to_handle, hipStream_t s);
// io.K steps of greedy evaluation of the learner's tables (mdpp_discrete_eval.hip; the forms with io.summary or per-env noise
// levels: mdpp_discrete_eval.hpp's launch_eval_form, in mdpp_discrete_eval_{summary,nlev,nlev_summary}.hip)
int launch_discrete_eval(mdpp_env *h, const DiscreteIO &io);
// the observation every env shows now, from the state record, to obs [N] (mdpp_discrete_eval.hip)
int launch_discrete_current_obs(mdpp_env *h, void *obs, hipStream_t s);
// closed-loop continuous rollout under the handle's linear policy (mdpp_continuous_linear.hip; the step: mdpp_continuous_closed.hpp):
// why the handle has none (empty: it is served); io.K steps, the actions taken written to io.actions, or with io.summary the
// summary form (mdpp_continuous_summary_linear.hip); the parameters between the caller's layout and the handle's buffer; the
// state in every env's record as its observation [N][D]
std::string continuous_linear_refusal(const mdpp_env *h);
int launch_continuous_linear(mdpp_env *h, const ContinuousIO &io);
int launch_linear_theta_copy(mdpp_env *h, float *user, bool to_handle, hipStream_t s);
// the memory of a history = 2 policy between the handle's [D][N] and the caller's [N][D] (mdpp_linear_memory)
int launch_linear_memory_copy(mdpp_env *h, float *user, bool to_handle, hipStream_t s);
// ... and with one (1+1)-ES per env on that policy (include/mdpp.h "Linear policy search"; mdpp_continuous_search.hip, the
// summary form: mdpp_continuous_summary_search.hip): the candidate is the handle's parameter buffer, sr the caller's arrays
int launch_continuous_search(mdpp_env *h, const ContinuousIO &io, const mdpp_linear_search &sr);
// ... and with one antithetic ES per wave of 64 such policies (include/mdpp.h "Linear policy ES"; mdpp_continuous_es.hip, the
// summary form: mdpp_continuous_summary_es.hip); launch_linear_es_init: the candidates of the current generation
int launch_continuous_es(mdpp_env *h, const ContinuousIO &io, const mdpp_linear_es &es);
int launch_linear_es_init(mdpp_env *h, const mdpp_linear_es &es, hipStream_t s);
int launch_continuous_current_obs(mdpp_env *h, float *obs, hipStream_t s);
int launch_grid_step(mdpp_env *h, const DiscreteIO &io);
int launch_grid_reset(mdpp_env *h, const uint8_t *mask, void *obs, hipStream_t s);
// io.K steps of the grid handle's tabular learner, or (eval) of greedy evaluation of its tables (mdpp_grid_learn.hip; with
// io.summary the summary form, mdpp_grid_summary_learn.hip; with a schedule in force or an episode log in io.summary the SCHED
// and LOG forms, mdpp_grid_sched_learn.hip, mdpp_grid_episodes_learn.hip; the kernel: mdpp_grid_learn.hpp): why the handle has none (empty:
// it is served); the action vectors taken written to io.actions [K][N][2]; Q between the caller's [N][S][A] and the
// handle's entry-major buffer
std::string grid_learn_refusal(const mdpp_env *h);
int launch_grid_learn(mdpp_env *h, const DiscreteIO &io, bool eval);
int launch_grid_q_copy(mdpp_env *h, float *user_q, bool to_handle, hipStream_t s);
// phase bits: 1 = draw + records, 2 = render (phase == 2 exactly: pipelined, the persistent grid leaves slots
// free for the next batch's state kernel; 6 = render only on the full grid); buf: scratch set (0 / 1)
int launch_image_obs(mdpp_env *h, int K, const int32_t *state_out, const int32_t *state_final,
                     const uint8_t *term, const uint8_t *trunc, const uint8_t *mask,
                     uint8_t *img_out, uint8_t *img_final, hipStream_t s, int phase = 3, int buf = 0);
// One step's draw + record + render in one kernel (mdpp_image.hip k_image_step1): 1 = launched, 0 = this handle keeps
// launch_image_obs, < 0 = error
int launch_image_step1(mdpp_env *h, const int32_t *state_out, const int32_t *state_final, const uint8_t *term,
                       const uint8_t *trunc, uint8_t *img_out, uint8_t *img_final, hipStream_t s);
const char *image_obs_kernel_name(const mdpp_env *h, int K);    // the renderer launch_image_obs() uses
} // namespace mdpp
// mdpp_generate.hip: envs [first, first + count) of a GenArgs block; PCG64(SeedSequence(seeds[i])) into a stream's buffers
hipError_t launch_generate_discrete(const mdpp::GenArgs &a, int first, int count);
hipError_t launch_seed_streams_seedseq(const uint64_t *seeds, int N, void *st, void *inc, void *half);
