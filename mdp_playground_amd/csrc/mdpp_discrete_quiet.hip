// Fused K-step rollout for quiet discrete envs that the specialised kernels of
// mdpp_discrete_fast.hip / mdpp_discrete_pipe.hip do not take: any S <= 255 and L <= 7, an optional
// irrelevant sub-space (irrelevant_features=True: action / observation pairs), one shared MDP with
// its tables in LDS, unit rewards, numpy PCG64 streams, no noise.
// Same arithmetic as k_discrete_step (mdpp_discrete.hip; reference rl_toy_env.py:1992-2125 and reset
// :2250-2278, irrelevant sub-space :2028-2035, :2063-2092), restructured like k_grid_rollout_fast:
//   * straight-line step body, every run-time option a select; no float64 in the step (the four
//     possible rewards are formed once, in the reference's float64 operation order);
//   * start states are drawn AHEAD of need into a per-lane register queue (with an irrelevant
//     sub-space a queued entry is the pair, drawn relevant-then-irrelevant like reset() does),
//     topped up for all lanes at once when some lane runs dry: with 2 of 8 states terminal some
//     lane of a wave resets on almost every step, and drawing inside the step runs the PCG64 step
//     and the cdf search for the whole wave each time;
//   * what is left in the queue at the end of the launch is un-drawn (inverse LCG step), so the
//     env stream is again exactly where the reference's would be.  Nothing else reads the env
//     stream on this path (no reward noise), so the draws are consumed in stream order.
// DUO: one wavefront per SIMD -- all a 65 536-env job gives a lane-per-env kernel -- leaves about
// half of the SIMD's issue slots idle (profiles/archive/r01_ablation_fast_kernel.txt).  With full 256-env
// blocks and K >= 32 the step is therefore split over TWO waves per SIMD (512-thread workgroups),
// like k_discrete_rollout_pipe does for the packed shapes:
//   E  waves 0-3  state recurrence of both sub-spaces, sequence key, episode counters, terminal
//                 test, same-step autoreset from the queue, the env's PCG64 stream; one 64-bit
//                 record per env step into an LDS ring
//   O  waves 4-7  reward-bitmask lookup, delay line, reward select and ALL global stores
//   H  waves 8-11 (ROLES = 3, autoreset on) own the env's PCG64 stream for the launch and keep a small
//                 LDS ring of pre-drawn start states filled; what the E lane did not take is un-drawn
// Lane l of waves w, w + 4 (and w + 8) serves the same env; the rings are single-producer /
// single-consumer with release / acquire counters at workgroup scope, polled once per 8 steps,
// every spin bounded (MDPP_STATUS_INTERNAL instead of a hang).
#include <stdlib.h>

#include <stdio.h>

#include <type_traits>

#include "mdpp_internal.hpp"
#include "mdpp_rng.hpp"

namespace mdpp {

#if defined(MDPP_Q_PRIO_E) || defined(MDPP_Q_PRIO_O) || defined(MDPP_Q_PRIO_H)
#define MDPP_Q_PRIO_FORCED 1       // (tools/ablate.py: the same priorities for every form)
#else
#define MDPP_Q_PRIO_FORCED 0
#endif
#ifndef MDPP_Q_PRIO_E
#define MDPP_Q_PRIO_E 0
#endif
#ifndef MDPP_Q_PRIO_O
#define MDPP_Q_PRIO_O 0
#endif
#ifndef MDPP_Q_PRIO_H
#define MDPP_Q_PRIO_H 0
#endif
constexpr int kQQ = 4;                         // start states queued per lane
// 128-bit buffer stores carry their WHOLE offset in the VGPR.  With a register in the soffset field the
// compiler's hazard recognizer assumes that the store-data hazard of > 64-bit stores (a VALU write to the
// data registers right behind the store) does not exist and inserts no wait state; on gfx950 it does
// exist: lanes 12-15 of every 16 stored the overwritten register (found by the role-split soak test).
constexpr int kQRsrc = 0x00020000;
#ifndef MDPP_Q_DEPTH
#define MDPP_Q_DEPTH 24
#endif
constexpr int kQDepth = MDPP_Q_DEPTH;          // E -> O ring depth in steps (multiple of the chunk of 8)
constexpr int kHD = 32;                        // Philox producers -> E ring depth in steps
constexpr int kXR = 16;                        // XR: stream positions the X wave evaluates ahead of E (per lane), kXB per batch
constexpr int kXB = 4;
constexpr uint32_t kQSpinLimit = 1u << 22;
constexpr uint32_t kQStatusInternal = 0x80000000u;

// record (E -> O), one per env step
//   lo: [7:0] observation (after a possible reset)  [15:8] state reached  [23:16] irrelevant obs  [31:24] irrelevant reached
//   hi: [0] terminated  [1] truncated  [2] reset happened  [3] history full (NaN gate)  [4] pay step  [31:5] sequence key
// start states H -> E: one 64-bit word per env, three 16-bit entries (rel | irr << 8) and, in the top
// 16 bits, the number of entries pushed so far (mod 2^16); E answers with the number it has taken
//
// PN / RN: transition noise / reward noise (numpy streams).  PN: E draws one uniform per step from the
// state space's stream and re-draws the next state from the categorical around the table's entry
// (:1604-1622), searched as integer thresholds like rho_0.  RN: the reward noise comes from the ENV
// stream, the one reset() draws from, and numpy's order is normal-of-the-step, then the reset draw:
// so E owns that stream, draws the step's standard normal (ziggurat tables in LDS) and hands it to O
// beside the record, start states are drawn at need instead of ahead, and there is no H role.
// PH: Philox streams (mdpp_rng.hpp): everything random about tick t is one word (or one float32 normal) of a block
// keyed by (seed, global env id, t >> 2, stream) -- the transition-noise word (philox_pnoise_*: "noisy" and which
// other state, no cdf), the reward normal, the start state --, nothing is loaded from or stored to HBM, start
// states are drawn at need (like RN: no queue, no H role, nothing to un-draw).
// NPH (PH, two roles, no irrelevant sub-space): Philox producer waves.  A counter-based stream has no serial
// state, so everything random about step k -- the P-noise uniform, the reward-noise normal, the start state
// a reset at that step would draw -- is a pure function of (seed, env, tick) and is made AHEAD of the step by
// NPH extra waves per SIMD (producer p takes the four-tick blocks b = p mod NPH: three Philox blocks and two packed
// Box-Muller pairs per four env steps) into an LDS ring; the E wave, whose dependent chain is the step time, then
// runs no generator at all (two Philox blocks and a Box-Muller pair per step on E were 0.15 of the HBM roofline
// on cfg2 + noise; one block + one pair per step on the producers 0.24).
// XR (round 6: ROLES = 3 with RN on numpy streams, no transition noise, one sub-space, same-step autoreset or none): reward
// noise put the env stream's generator INSIDE E's recurrence -- per step one PCG64 word and a ziggurat decision, per reset one
// more word and a categorical search, run by the whole wave whenever one lane resets: 2 200 cycles per step, 490 us per
// launch at S = 50 where the noise-free kernel takes 220.  The third wave now owns the env stream the way the H wave of
// k_discrete_rollout_lean<NRN> does (mdpp_discrete_lean.hip header): it evaluates EVERY position p of the stream as if a
// draw started there -- x_meta[p] = {start state word p would give a reset, kind: accepted at once / wedge accepted (2 words) /
// wedge rejected (2 words, the draw starts over) / tail (word count, start state behind its words)} and x_val[p] = that
// draw's value -- into 16-position rings per lane, up to 16 positions ahead of the position E publishes; E walks positions
// (three metas fetched one step ahead) and runs no generator at all; what E did not reach is un-drawn at the end.  With a
// sigma of 0 (rn_z0) no value is formed or read.
// UR = false (round 5): rewards that are not all 1.0 (reward_dist, :1528-1544 -- the reference's rainbow_reward_dist sweep) on
// numpy streams without an irrelevant sub-space: the O role looks the step's sequence key up in a float64 table in LDS
// (DiscreteArgs::rtable), the delay line holds KEYS in HBM (ring_keys[delay][N], the general kernel's, so the two kernels
// hand a handle to each other mid-episode), and the reward is formed in float64 in the reference's order like
// k_discrete_step<UNIT = false> does.  Until round 5 these handles ran on the one-role general kernel (0.14 of the HBM
// roofline at S = 24).
// SF (round 6): the E wave is ONE wave that issues ~270 instructions per env step in the general form (vector and scalar:
// every run-time option is a select or a mask operation on every step), and a wave issues about one instruction per 4 cycles --
// 1 000 cycles per step, the kernel's whole time at S = 50 (the O wave: 32 vector instructions per step).  SF fixes what the
// reference's S = 20-50 sweeps leave at their defaults -- sequence_length 1, same-step autoreset, no step limit, every step pays,
// one sub-space, no transition noise, S <= 128 -- at compile time: the sequence key IS the state, no history window to shift,
// no phase, no pending reset, the terminal flag rides in bit 7 of the P entry (one LDS round trip per step instead of two
// dependent ones), and the numpy-indexing fix-up of the action runs only when some lane's action is out of range.
// PE (round 6): one MDP PER ENV (RLToyVectorEnv(seeds=[...]): env i is the reference's RLToyEnv(seed=seeds[i]), tables per env in
// HBM -- what every golden uses).  These handles ran the one-role general kernel with each lane's tables in an LDS slot: one
// wave per SIMD doing everything, 1.1 us per step (0.13 of the HBM roofline at 65 536 envs).  Here the lane's tables -- P
// (terminal bit folded in under SF), terminal flags, reward bits, rho_0 thresholds; 280 B at 8 x 8 -- are staged into ITS slot
// of the workgroup's dynamic LDS once per launch (slot stride = the shared carve + the thresholds + 8 bytes: bank spread) and
// every table pointer of the E / O / H (or X) roles carries the lane's slot offset; everything else is the shared-MDP kernel.
// S <= 16 (no bucket table), unit rewards, one sub-space, numpy streams, no transition noise, three roles.
template <bool OBS64, bool IRR, int ROLES, bool PN, bool RN, bool PH = false, int NPH = 0, bool UR = true, bool SF = false, bool PE = false>
__global__ __launch_bounds__((ROLES + NPH) * kBlock) void k_discrete_rollout_quiet(DiscreteArgs a, int K,
                                                                   const int32_t *__restrict__ actions,
                                                                   void *__restrict__ obs, float *__restrict__ reward,
                                                                   uint8_t *__restrict__ term, uint8_t *__restrict__ trunc,
                                                                   void *__restrict__ final_obs) {
    const uint64_t ptick0 = tick_now(a);               // the step counter at this launch (through the device-side offset of a graph replay)
    const uint32_t rhead0 = ring_head_now(a, ptick0);    // ... and the head of the key delay line (UR = false)
    static_assert(UR || (!IRR && !PH && NPH == 0), "non-unit rewards: numpy streams, one sub-space");
    typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ float s_rsel[4];
    __shared__ __align__(16) uint32_t s_prod[kBlock / 64], s_cons[kBlock / 64];   // steps published by E wave w / consumed by O wave w
    // Per-lane stores.  Every store INSTRUCTION of the O wave costs the launch about the same whatever it carries (build without
    // the two 64-byte flag stores: 183 -> 162 us at S = 50, without any store 134), but whole-row stores as in
    // k_discrete_rollout_lean (O wave w takes rows w and w + 4 of a chunk for all 256 envs of the block, the rewards through LDS
    // staging buffers: 10 store instructions per chunk and wave instead of 32) measured no better (round 6, on one lease): S = 50
    // unit rewards 0.435 -> 0.435-0.453 of HBM, S = 24 with reward_dist 0.447 -> 0.417-0.421, S = 50 with the noise key 0.221 ->
    // 0.216 -- the hand-over between the workgroup's waves costs what the fewer stores save wherever the O wave is a long stage.
    // (s_rprod / s_rcons were that form's counters: nothing reads them, but they stay, zeroed, as they fix the kernels' LDS layout)
    __shared__ __align__(16) uint32_t s_rprod[kBlock / 64], s_rcons[kBlock / 64];
    __shared__ __align__(8) uint64_t s_start[ROLES == 3 ? kBlock : 1];   // H -> E
    __shared__ uint32_t s_head[ROLES == 3 ? kBlock : 1];                 // E -> H
    __shared__ uint32_t s_done;                                         // E waves that have finished
    constexpr bool ZIG = RN && !PH;                 // numpy's ziggurat tables
    constexpr bool ATNEED = RN || PH;               // start states drawn when an episode ends, not ahead
    __shared__ uint64_t s_ki[ZIG ? 256 : 1];
    __shared__ double s_wi[ZIG ? 256 : 1], s_fi[ZIG ? 256 : 1];
    constexpr bool XR = ROLES == 3 && RN && !PH;    // the third wave evaluates the env stream by position (header)
    static_assert(!XR || (!PN && !IRR && NPH == 0), "XR: reward noise alone, one sub-space");
    static_assert(!SF || (ROLES == 3 && !PN && !IRR && !PH && NPH == 0), "SF: three roles, numpy streams, one sub-space, no transition noise");
    static_assert(!(ATNEED && ROLES == 3) || XR, "reward noise and reset draws share the env stream: no start-state queue");
    static_assert(!PE || (ROLES == 3 && UR && !PN && !IRR && !PH && NPH == 0), "PE: three roles, unit rewards, numpy streams, one sub-space");
    constexpr int XRN = kXR;                        // positions X runs ahead of E (8 with batches of 4 serialised the two waves: 905 us per launch)
    __shared__ uint32_t x_meta[XR ? XRN : 1][kBlock];
    // (x_val -- the draws' values, unless sigma is 0 -- lives in DYNAMIC LDS behind the record ring: the launcher adds its 32 KiB only
    //  for handles that form values; with one MDP per env there is room for it only at sigma 0)
    __shared__ uint32_t x_hhead[XR ? kBlock : 1], x_epos[XR ? kBlock : 1];      // positions made by X / reached by E
    static_assert(NPH == 0 || (PH && ROLES == 2 && !IRR), "Philox producers: two roles, one sub-space");
    // producers -> E: per env and step {other-state index j | noisy << 8 | start state << 16} and the reward normal
    __shared__ __align__(8) uint32_t s_hm[NPH ? kHD * kBlock : 1];
    __shared__ float s_hz[(NPH && RN) ? kHD * kBlock : 1];
    __shared__ uint32_t s_t31[NPH ? 256 : 1];                           // rho_0 as 31-bit thresholds (producers)
    __shared__ uint32_t s_hprod[NPH ? NPH : 1][kBlock / 64];            // producer p has made every step < this of its blocks, for wave w
    constexpr bool DUO = ROLES >= 2, TRIO = ROLES == 3 && !XR;      // (TRIO: the start-state queue's H role)
    const bool rn_z0 = RN && !PH && a.r_noise == 0.0 && !(a.opts & MDPP_OPT_NO_SIGMA0);   // the reward_noise key present with sigma 0 (wave-uniform)
    // Wave priorities (s_setprio; round 6, tools/ablate.py on one lease).  XR: the position wave is the long stage -- X 3, E 2, O 1:
    // d_s50_rn0 0.216 -> 0.255 of HBM (E 1 / O 0 / X 3: 0.254; E 3 / O 1 / X 2: 0.240).  The start-state queue's three roles: E 3,
    // O 1, H 2 (0.404 -> 0.416, the other orders within a percent).  One and two roles: all equal, as before.
    constexpr int kPrioE = MDPP_Q_PRIO_FORCED ? MDPP_Q_PRIO_E : XR ? 2 : TRIO ? 3 : 0;
    constexpr int kPrioO = MDPP_Q_PRIO_FORCED ? MDPP_Q_PRIO_O : (XR || TRIO) ? 1 : 0;
    constexpr int kPrioH = MDPP_Q_PRIO_FORCED ? MDPP_Q_PRIO_H : XR ? 3 : TRIO ? 2 : 0;
    constexpr int kDepth = RN ? 16 : kQDepth;       // RN records carry a double: 16 B per step
    constexpr int kThreads = (ROLES + NPH) * kBlock;
    const int tid = threadIdx.x;
    // Workgroup b runs on XCD b % 8 (round-robin dispatch): with full blocks every XCD steps one contiguous eighth of the envs, so
    // that what its L2 writes back per output row is one contiguous range (as in k_discrete_rollout_lean)
    const uint32_t eblk = (DUO && (gridDim.x & 7u) == 0u) ? (blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3) : blockIdx.x;
    const int role = DUO ? tid / kBlock : 0;        // 0 = E, 1 = O, 2 = H
    const int l = DUO ? (tid & (kBlock - 1)) : tid, w = l >> 6;
    // shared MDP -> LDS (same carve as k_discrete_step) + the irrelevant sub-space's table and cdf
    // (PE: this lane's MDP into its slot -- the three threads that serve lane l share the copy)
    // (PE's own carve of a slot: P, terminal flags, reward bits, then the S8 thresholds, + 8 bytes of bank spread)
    const uint32_t pe_S8 = ((uint32_t)a.S + 7u) & ~7u;
    const uint32_t pe_term = (uint32_t)(a.S * a.A), pe_rew = (pe_term + (uint32_t)a.S + 7u) & ~7u, pe_T0 = (pe_rew + a.rbits_stride + 7u) & ~7u;
    const uint32_t pe_stride = PE ? pe_T0 + pe_S8 * 8u + 8u : 0u;
    const uint32_t pe_off = PE ? (uint32_t)l * pe_stride : 0u;
    if constexpr (PE) {
        const size_t ti = (size_t)eblk * kBlock + (size_t)l;          // (full blocks only: three roles)
        const int SA = a.S * a.A;
        unsigned char *slot = lds + pe_off;
        for (int k = role; k < SA; k += ROLES) {
            const uint8_t nx = a.P[ti * SA + k];
            slot[k] = SF ? (uint8_t)(nx | (a.is_term[ti * a.S + nx] ? 0x80u : 0u)) : nx;
        }
        for (int k = role; k < a.S; k += ROLES) slot[pe_term + k] = a.is_term[ti * a.S + k];
        for (uint32_t k = role; k < a.rbits_stride; k += ROLES) slot[pe_rew + k] = a.rbits[ti * a.rbits_stride + k];
        for (uint32_t k = role; k < pe_S8; k += ROLES)
            ((uint64_t *)(slot + pe_T0))[k] =
                k < (uint32_t)a.S ? (uint64_t)ceil(a.init_cdf[ti * a.S + k] * 9007199254740992.0) : ~0ULL;
    } else
    if constexpr (SF) {                              // entry = next state | is_terminal[next state] << 7 (S <= 128, host-checked)
        for (int k = tid; k < a.S * a.A; k += kThreads) { const uint8_t nx = a.P[k]; lds[a.lds_P + k] = (uint8_t)(nx | (a.is_term[nx] ? 0x80u : 0u)); }
    } else {
        for (int k = tid; k < a.S * a.A; k += kThreads) lds[a.lds_P + k] = a.P[k];
    }
    if constexpr (!PE) {
    for (int k = tid; k < a.S; k += kThreads) lds[a.lds_term + k] = a.is_term[k];
    if (UR) { for (uint32_t k = tid; k < a.rbits_stride; k += kThreads) lds[a.lds_rew + k] = a.rbits[k]; }
    else { for (uint32_t k = tid; k < a.nkeys; k += kThreads) ((double *)(lds + a.lds_rew))[k] = a.rtable[k]; }
    }
    if (ZIG) zig_stage(s_ki, s_wi, s_fi, tid, kThreads);
    const ZigLds zig{s_ki, s_wi, s_fi};
    // rho_0 as integer thresholds: cdf[j] <= u  <=>  ceil(cdf[j] * 2^53) <= r >> 11 (exact: u is
    // (r >> 11) * 2^-53), padded to a multiple of 8 with 2^64-1 so the search runs in unrolled blocks
    const uint32_t lds_P1 = a.lds_bytes, lds_T0 = (a.lds_bytes + (IRR ? (uint32_t)(a.S1 * a.A1) : 0u) + 15u) & ~15u;
    const uint32_t S8 = ((uint32_t)a.S + 7u) & ~7u, S18 = IRR ? (((uint32_t)a.S1 + 7u) & ~7u) : 0u;
    const uint32_t lds_T1 = lds_T0 + S8 * 8u;
    const uint32_t lds_TN = lds_T1 + S18 * 8u;                 // PN: S rows of S8 thresholds of the noise categoricals
    constexpr bool PNC = PN && !PH;                             // (Philox streams need no cdf: philox_pnoise_*)
    const uint32_t lds_TN1 = lds_TN + (PNC ? (uint32_t)a.S * S8 * 8u : 0u);   // ... and S1 rows of S18 for the irrelevant sub-space
    const uint32_t lds_end = PE ? (uint32_t)kBlock * pe_stride : lds_TN1 + ((PNC && IRR) ? (uint32_t)a.S1 * S18 * 8u : 0u);
    if (PNC) {
        for (uint32_t k = tid; k < (uint32_t)a.S * S8; k += kThreads) {
            const uint32_t row = k / S8, col = k - row * S8;
            ((uint64_t *)(lds + lds_TN))[k] =
                col < (uint32_t)a.S ? (uint64_t)ceil(a.noise_cdf[row * (uint32_t)a.S + col] * 9007199254740992.0) : ~0ULL;
        }
        if (IRR) {
            for (uint32_t k = tid; k < (uint32_t)a.S1 * S18; k += kThreads) {
                const uint32_t row = k / S18, col = k - row * S18;
                ((uint64_t *)(lds + lds_TN1))[k] =
                    col < (uint32_t)a.S1 ? (uint64_t)ceil(a.noise_cdf1[row * (uint32_t)a.S1 + col] * 9007199254740992.0) : ~0ULL;
            }
        }
    }
    if constexpr (!PE)
    for (uint32_t k = tid; k < S8; k += kThreads)
        ((uint64_t *)(lds + lds_T0))[k] = k < (uint32_t)a.S ? (uint64_t)ceil(a.init_cdf[k] * 9007199254740992.0) : ~0ULL;
    if (NPH)       // cdf[j] <= m31 2^-31  <=>  ceil(cdf[j] 2^31) <= m31; padding never counts
        for (uint32_t k = tid; k < 256u; k += kThreads)
            s_t31[k] = k < (uint32_t)a.S ? (uint32_t)(((uint64_t)ceil(a.init_cdf[k] * 9007199254740992.0) + 0x3FFFFFull) >> 22) : 0x80000000u;
    if (IRR) {
        for (int k = tid; k < a.S1 * a.A1; k += kThreads) lds[lds_P1 + k] = a.P1[k];
        for (uint32_t k = tid; k < S18; k += kThreads)
            ((uint64_t *)(lds + lds_T1))[k] = k < (uint32_t)a.S1 ? (uint64_t)ceil(a.init_cdf1[k] * 9007199254740992.0) : ~0ULL;
    }
    if (tid < 4) {
        // {paid, terminal} -> float32, formed in float64 in the reference's operation order (:1987-1990, :2107)
        double r = (tid & 2) ? 1.0 : 0.0;
        r *= a.scale;
        r += a.shift;
        if (tid & 1) r += a.term_add;
        s_rsel[tid] = (float)r;
    }
    if (tid < kBlock / 64) {
        s_prod[tid] = 0; s_cons[tid] = 0; s_rprod[tid] = 0; s_rcons[tid] = 0;
        if (NPH) for (int p = 0; p < NPH; p++) s_hprod[p][tid] = 0;
    }
    if (TRIO && tid < kBlock) { s_start[tid] = 0; s_head[tid] = 0; }
    if (XR && tid < kBlock) { x_hhead[tid] = 0; x_epos[tid] = 0; }
    if (tid == 0) s_done = 0;
    __syncthreads();
    // DUO: the record ring follows the tables in dynamic LDS
    uint64_t *ring = (uint64_t *)(lds + ((lds_end + 15u) & ~15u));
    double *ringz = (double *)(ring + kDepth * kBlock);         // RN: the step's standard normal (sigma 0: not allocated, not touched)
    double *x_val = ringz + kDepth * kBlock;                    // XR, values formed: [XRN][kBlock] (launcher: xr_val_bytes)
    const uint8_t *P = lds + (PE ? pe_off : a.lds_P), *is_term = lds + (PE ? pe_off + pe_term : a.lds_term),
                  *rbits = lds + (PE ? pe_off + pe_rew : a.lds_rew), *P1 = lds + lds_P1;
    const uint64_t *T0 = (const uint64_t *)(lds + (PE ? pe_off + pe_T0 : lds_T0)), *T1 = (const uint64_t *)(lds + lds_T1);
    const uint64_t *TN = (const uint64_t *)(lds + lds_TN), *TN1 = (const uint64_t *)(lds + lds_TN1);
    // Large state spaces (round 5; the reference's 24- and 50-state sweeps): rho_0's S thresholds are not searched one by one
    // (S = 50: 56 64-bit compares per draw, 150 vector instructions -- most of the H wave) but through a bucket table over the
    // top 12 bits of the 53-bit draw: s_bk[b] = {thresholds at or below the bucket's first value, thresholds strictly inside it};
    // a draw compares with the few thresholds inside its bucket (none for 99 % of the buckets).  Built here from T0.
    // (8 KiB of static LDS only in the instantiations that can use it: numpy streams, two or three roles)
    __shared__ uint16_t s_bk[(!PH && ROLES >= 2 && !PE) ? 4096 : 1];
    const bool use_bk = !PH && DUO && !PE && S8 > 16u;
    if (use_bk) {
        for (uint32_t b = tid; b < 4096u; b += kThreads) {
            const uint64_t lo = (uint64_t)b << 41, hi = lo + (1ULL << 41);
            uint32_t c0 = 0, n = 0;
            for (uint32_t j = 0; j < S8; j++) {
                const uint64_t t = T0[j];
                c0 += t <= lo ? 1u : 0u;
                n += (t > lo && t < hi) ? 1u : 0u;
            }
            s_bk[b] = (uint16_t)(c0 | (n << 8));
        }
        __syncthreads();
    }

    const uint32_t i = eblk * kBlock + l;
    if (!DUO && i >= (uint32_t)a.N) return;            // (DUO launches have full blocks only)
    const uint32_t N = (uint32_t)a.N, S = (uint32_t)a.S, A = (uint32_t)a.A, L = SF ? 1u : (uint32_t)a.L;
    const uint4 st = a.state[i];
    uint64_t hist = ((uint64_t)st.y << 32) | st.x;               // last L+1 states, newest in byte 0, 0xFF = NaN slot
    // next-step autoreset: "episode ended, reset at the next call" travels in bit 31 of the step counter (k_discrete_step);
    // the reset call ignores the action, draws nothing from the noise streams and returns (start state, 0.0, no flags)
    const bool nextmode = SF ? false : a.autoreset == MDPP_AUTORESET_NEXT_STEP;
    uint32_t steps = st.z & 0x7FFFFFFFu, ringbits = st.w, status = 0;
    bool pend = nextmode && (st.z >> 31) != 0u;
    uint32_t cur1 = IRR ? a.irr_state[i] : 0u;
    typedef typename std::conditional<PH, Philox, Pcg64>::type Gen;
    Gen g, sp, sp1;
    PhiloxTickWords pnw, pnw1;             // PH without producers: the current four ticks' noise words / normals
    PhiloxTickNormals rnz;
    const uint64_t pn_M = a.pn_M, pn_M1 = a.pn_M1;
    const uint64_t genv = (uint64_t)(a.env_id_offset + (int64_t)i);         // global env id (Philox key)
    if constexpr (!PH) {
        g.load(a.env_s, a.env_inc, i);
        if (PN) sp.load(a.sp_s, a.sp_inc, i);
        if (PN && IRR) sp1.load(a.sp1_s, a.sp1_inc, i);
    }
    // sequence key over the last L states, carried: key' = (key - oldest * S^(L-1)) * S + new
    uint32_t spow = 1;
    for (uint32_t j = 1; j < L; j++) spow *= S;
    uint32_t key = 0, valid = 0;                                 // valid: number of non-NaN states among the last L+1 (capped)
    for (int j = (int)L - 1; j >= 0; j--) {
        const uint32_t b = (uint32_t)(hist >> (8 * j)) & 0xFFu;
        key = key * S + (b == 0xFFu ? 0u : b);
    }
    for (uint32_t j = 0; j <= L; j++) valid += (((uint32_t)(hist >> (8 * j)) & 0xFFu) != 0xFFu) ? 1u : 0u;

    uint32_t queue[kQQ];                                          // rel | irr << 8, queue[0] next
#pragma unroll
    for (int q = 0; q < kQQ; q++) queue[q] = 0;
    uint32_t qn = 0;
    auto draw_state_g = [&](auto &g, const uint64_t tick) __attribute__((always_inline)) -> uint32_t {     // (g: the lane's env generator, in either form)
        // self._np_random.choice(S, p=rho_0): searchsorted(cdf, u, 'right') (:2255); then the
        // irrelevant start state the same way (:2259-2264)
        if constexpr (PH) {
            // Philox streams: one word of the start-state stream(s) of this tick, a 31-bit uniform (mdpp_rng.hpp):
            // cdf[j] <= m31 2^-31  <=>  ceil(cdf[j] 2^53) <= m31 << 22
            const uint64_t m = (uint64_t)philox_start_m31(a.philox_seed, genv, tick, kPhiloxStartStream) << 22;
            uint32_t s0 = 0;
            for (uint32_t b = 0; b < S8; b += 8) {
#pragma unroll
                for (uint32_t j = 0; j < 8; j++) s0 += (T0[b + j] <= m) ? 1u : 0u;
            }
            if (IRR) {
                const uint64_t m1 = (uint64_t)philox_start_m31(a.philox_seed, genv, tick, kPhiloxStartIrrStream) << 22;
                uint32_t s1 = 0;
                for (uint32_t b = 0; b < S18; b += 8) {
#pragma unroll
                    for (uint32_t j = 0; j < 8; j++) s1 += (T1[b + j] <= m1) ? 1u : 0u;
                }
                s0 |= s1 << 8;
            }
            return s0;
        }
        const uint64_t m = g.next64() >> 11;
        uint32_t s0 = 0;
        if (use_bk) {
            const uint32_t e = s_bk[(uint32_t)(m >> 41)];
            const uint32_t c0 = e & 0xFFu, nin = e >> 8;
            s0 = c0;
            for (uint32_t j = 0; __builtin_amdgcn_ballot_w64(j < nin) != 0; j++) s0 += (j < nin && T0[j < nin ? c0 + j : 0u] <= m) ? 1u : 0u;
        } else {
            for (uint32_t b = 0; b < S8; b += 8) {
#pragma unroll
                for (uint32_t j = 0; j < 8; j++) s0 += (T0[b + j] <= m) ? 1u : 0u;
            }
        }
        if (IRR) {
            const uint64_t m1 = g.next64() >> 11;
            uint32_t s1 = 0;
            for (uint32_t b = 0; b < S18; b += 8) {
#pragma unroll
                for (uint32_t j = 0; j < 8; j++) s1 += (T1[b + j] <= m1) ? 1u : 0u;
            }
            s0 |= s1 << 8;
        }
        return s0;
    };
    auto draw_state = [&](const uint64_t tick = 0) __attribute__((always_inline)) -> uint32_t { return draw_state_g(g, tick); };
    auto refill = [&]() __attribute__((always_inline)) {         // (always_inline: no generator / queue behind a pointer)
        for (int round = 0; round < kQQ; round++) {
            if (__builtin_amdgcn_ballot_w64(qn < (uint32_t)kQQ) == 0) break;
            if (qn < (uint32_t)kQQ) {
                const uint32_t c = draw_state();
#pragma unroll
                for (int q = 0; q < kQQ; q++) queue[q] = (qn == (uint32_t)q) ? c : queue[q];
                qn++;
            }
        }
    };
    if constexpr (NPH > 0) if (role >= 2) {
        // =========================================================== Philox producer (see NPH above)
        const int me = role - 2;
        __builtin_amdgcn_s_setprio(kPrioH);
        uint32_t hstatus = 0;
        const uint64_t G0 = ptick0 >> 2;
        const int nG = (int)(((ptick0 + (uint64_t)K - 1u) >> 2) - G0) + 1;
        const bool small = S <= 8u;                              // rho_0 thresholds in scalar registers
        uint32_t t31[8];
#pragma unroll
        for (int j = 0; j < 8; j++) t31[j] = __builtin_amdgcn_readfirstlane(s_t31[j]);
        const bool want_start = a.autoreset != 0;
        for (int r = me; r < nG; r += NPH) {
            const uint64_t blk = G0 + (uint64_t)r;
            const int kfirst = (int)((int64_t)(blk << 2) - (int64_t)ptick0);      // step of the block's word 0 (may be < 0)
            const int k_hi = min(K, kfirst + 4);
            uint32_t pw[4] = {0u, 0u, 0u, 0u}, sw[4] = {0u, 0u, 0u, 0u};
            float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (PN) philox_start_block(a.philox_seed, genv, blk, kPhiloxPNoiseStream, pw);
            if (RN) {
                uint32_t o[4];
                philox_start_block(a.philox_seed, genv, blk, kPhiloxRNoiseStream, o);
                philox_box_muller2(o, z[0], z[1], z[2], z[3]);
            }
            if (want_start) philox_start_block(a.philox_seed, genv, blk, kPhiloxStartStream, sw);
            if (k_hi > kHD) {                                    // slots k % kHD: E must be through step k_hi - 1 - kHD
                uint32_t spins = 0;
                while (__hip_atomic_load(&s_prod[w], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < (uint32_t)(k_hi - kHD)) {
                    __builtin_amdgcn_s_sleep(1);
                    if (++spins > kQSpinLimit) { hstatus |= kQStatusInternal; break; }
                }
            }
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int k = kfirst + q;
                if (k < 0 || k >= K) continue;                   // (wave-uniform)
                uint32_t ent = 0;
                if (PN) ent = philox_pnoise_index(pw[q], a.pn_T, pn_M);
                if (want_start) {
                    const uint32_t m31 = sw[q] >> 1;
                    uint32_t s0 = 0;
                    if (small) {
#pragma unroll
                        for (int j = 0; j < 7; j++) s0 += (t31[j] <= m31) ? 1u : 0u;     // (entry 7: cdf 1.0 or padding)
                    } else {
                        for (uint32_t b = 0; b < S8; b += 8) {
#pragma unroll
                            for (uint32_t jj = 0; jj < 8; jj++) s0 += (s_t31[b + jj] <= m31) ? 1u : 0u;
                        }
                    }
                    ent |= s0 << 16;
                }
                s_hm[(k % kHD) * kBlock + l] = ent;
                if (RN) s_hz[(k % kHD) * kBlock + l] = z[q];
            }
            if ((l & 63) == 0) __hip_atomic_store(&s_hprod[me][w], (uint32_t)k_hi, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        if (hstatus) atomicOr(&a.status[i], hstatus);
        return;
    }
    const bool autoreset = SF ? true : a.autoreset != 0, has_max = SF ? false : a.max_steps > 0;
    const uint32_t max_steps = (uint32_t)a.max_steps, every_n = SF ? 1u : (uint32_t)a.every_n, delay = (uint32_t)a.delay;
    const bool isE = !DUO || role == 0;
    // =============================================================== X: the env stream by position (header, XR)
    if constexpr (XR) if (role == 2) {
        __builtin_amdgcn_s_setprio(kPrioH);
        uint32_t hq = 0, spins = 0, xstatus = 0;        // positions made
        // (the limb form of the PCG64 step, mdpp_rng.hpp: 31 instead of 46 vector instructions per word -- this wave is a generator
        //  and little else; its fixed temporaries v150-v157 fit the 168 registers of a 768-thread kernel)
        Pcg64Limbs gx;
        gx.from(g);
        uint64_t look = gx.next64();                    // the word of position hq (the generator runs one word ahead)
        // start state of a reset whose word is r: #{j : ceil(cdf[j] 2^53) <= r >> 11} (draw_state's search)
        auto start_of = [&](uint64_t r) __attribute__((always_inline)) -> uint32_t {
            const uint64_t m = r >> 11;
            uint32_t s0 = 0;
            if (use_bk) {
                const uint32_t e = s_bk[(uint32_t)(m >> 41)];
                const uint32_t c0 = e & 0xFFu, nin = e >> 8;
                s0 = c0;
                for (uint32_t j = 0; __builtin_amdgcn_ballot_w64(j < nin) != 0; j++) s0 += (j < nin && T0[j < nin ? c0 + j : 0u] <= m) ? 1u : 0u;
            } else {
                for (uint32_t b = 0; b < S8; b += 8) {
#pragma unroll
                    for (uint32_t j = 0; j < 8; j++) s0 += (T0[b + j] <= m) ? 1u : 0u;
                }
            }
            return s0;
        };
        for (;;) {
            if (__hip_atomic_load(&s_done, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) == kBlock / 64) break;
            const uint32_t epos = __hip_atomic_load(&x_epos[l], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const bool go = hq + (uint32_t)kXB <= epos + (uint32_t)XRN;
            if (__builtin_amdgcn_ballot_w64(go) != 0) {
                // The generator runs ONE word ahead (`look` = the word of position hq): the uniform a wedge point of position p
                // takes is word p + 1, which the batch has in hand -- no copy of the generator, no saved states
                uint32_t rej = 0;
                uint64_t wdv[kXB + 1];
                if (go) {
                    wdv[0] = look;
#pragma unroll
                    for (int u = 0; u < kXB; u++) {
                        const uint64_t wd = wdv[u];
                        wdv[u + 1] = gx.next64();
                        const uint32_t idx = (uint32_t)wd & 0xffu;
                        const uint64_t rabs = (wd >> 9) & 0x000fffffffffffffULL;
                        const bool ok = rabs < zig.ki[idx];
                        rej |= ok ? 0u : (1u << u);
                        const uint32_t slot = (hq + (uint32_t)u) & (uint32_t)(XRN - 1);
                        if (!rn_z0) {                   // numpy: x = rabs * wi, negated where bit 8 of the word is set
                            const double x = (double)rabs * zig.wi[idx];
                            x_val[slot * kBlock + l] = ((uint32_t)wd & 0x100u) ? -x : x;
                        }
                        x_meta[slot][l] = start_of(wd) | (ok ? 0u : (2u << 8));     // (rejected: patched below)
                    }
                    look = wdv[kXB];
                }
                // the ziggurat's slow path for the rejected words of the batch
                while (__builtin_amdgcn_ballot_w64(rej != 0u) != 0) {
                    if (rej != 0u) {
                        const uint32_t j = (uint32_t)__builtin_ctz(rej);
                        rej &= rej - 1u;
                        uint64_t wd = 0, wn = 0;                // the rejected word and the one behind it
#pragma unroll
                        for (int u = 0; u < kXB; u++)
                            if (j == (uint32_t)u) { wd = wdv[u]; wn = wdv[u + 1]; }
                        const uint32_t idx = (uint32_t)wd & 0xffu;
                        const uint32_t slot = (hq + j) & (uint32_t)(XRN - 1);
                        const uint32_t ss = x_meta[slot][l] & 0xFFu;
                        const uint64_t rabs = (wd >> 9) & 0x000fffffffffffffULL;
                        if (__builtin_expect(idx == 0u, 0)) {   // tail: two uniforms per try (np_zig_tail), 3 in 10^4 draws
                            const double nor_r = 3.6541528853610087963519472518, nor_inv_r = 0.27366123732975827203338247596;
                            // its words: what the batch still holds behind position j, then a copy of the generator
                            Pcg64Limbs t = gx;
                            uint32_t have = (uint32_t)kXB - j, cnt = 1u;
                            auto word = [&]() -> uint64_t {
                                uint64_t r = 0;
                                if (have != 0u) {
#pragma unroll
                                    for (int u = 1; u <= kXB; u++) if ((uint32_t)kXB - have + 1u == (uint32_t)u) r = wdv[u];
                                    have -= 1u;
                                } else {
                                    r = t.next64();
                                }
                                cnt += 1u;
                                return r;
                            };
                            double val = 0.0;
                            for (;;) {
                                const double u1 = (double)(word() >> 11) * (1.0 / 9007199254740992.0);
                                const double u2 = (double)(word() >> 11) * (1.0 / 9007199254740992.0);
                                const double xx = -nor_inv_r * log1p(-u1);
                                const double yy = -log1p(-u2);
                                if (yy + yy > xx * xx) { val = ((rabs >> 8) & 0x1) ? -(nor_r + xx) : nor_r + xx; break; }
                                if (cnt > 250u) { xstatus |= kQStatusInternal; break; }
                            }
                            if (!rn_z0) x_val[slot * kBlock + l] = val;
                            // (bits 24-31: the start state of the word BEHIND the tail's words -- a long tail reaches beyond the
                            //  window X keeps ahead of E)
                            const uint32_t words = cnt, ssb = start_of(word());
                            x_meta[slot][l] = ss | (3u << 8) | (words << 16) | (ssb << 24);
                        } else {                                // wedge: one uniform; a rejected point starts the draw over two words on
                            const double x = (double)rabs * zig.wi[idx];                // (|x|: it is squared)
                            const double u1 = (double)(wn >> 11) * (1.0 / 9007199254740992.0);
                            const bool acc = ((zig.fi[idx - 1] - zig.fi[idx]) * u1 + zig.fi[idx]) < exp(-0.5 * x * x);
                            x_meta[slot][l] = ss | ((acc ? 1u : 2u) << 8);
                        }
                    }
                }
                if (go) hq += (uint32_t)kXB;
                __hip_atomic_store(&x_hhead[l], hq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                spins = 0;
            } else {
                __builtin_amdgcn_s_sleep(2);
                if (++spins > kQSpinLimit * 4u) { xstatus |= kQStatusInternal; break; }
            }
        }
        // un-draw what was made and not used (+ the word in hand): s_prev = (s - inc) * M^-1 (mod 2^128)
        gx.to(g);
        for (uint32_t q = hq + 1u - __hip_atomic_load(&x_epos[l], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP); q > 0; q--) {
            const uint64_t lo = g.s_lo - g.inc_lo;
            const uint64_t hi = g.s_hi - g.inc_hi - (g.s_lo < g.inc_lo ? 1ULL : 0ULL);
            g.s_lo = lo * a.minv_lo;
            g.s_hi = __umul64hi(lo, a.minv_lo) + lo * a.minv_hi + hi * a.minv_lo;
        }
        g.store(a.env_s, i);
        if (xstatus) atomicOr(&a.status[i], xstatus);
        return;
    }
    // =============================================================== H: start-state producer
    if constexpr (TRIO) if (role == 2) {
        __builtin_amdgcn_s_setprio(kPrioH);
        uint64_t vals = 0;
        uint32_t tail = 0, slot = 0;
        // (the limb form of the PCG64 step: 31 instead of 46 vector instructions per word; v150-v157 fit a 768-thread kernel)
        Pcg64Limbs gl;
        gl.from(g);
#ifndef MDPP_Q_HMIN
#define MDPP_Q_HMIN 16          /* H draws for the wave once this many lanes have room (or one runs low) */
#endif
        for (;;) {
            if (__hip_atomic_load(&s_done, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) == kBlock / 64) break;
            const uint32_t head = __hip_atomic_load(&s_head[l], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
            const uint32_t cnt = (tail - head) & 0xFFFFu;
            const bool want = autoreset && cnt < 3u;
            const uint64_t bw = __builtin_amdgcn_ballot_w64(want);
            const bool urgent = __builtin_amdgcn_ballot_w64(want && cnt <= 1u) != 0;
            if (__builtin_popcountll(bw) >= MDPP_Q_HMIN || urgent) {
                if (want) {
                    const uint64_t c = draw_state_g(gl, 0);
                    const uint32_t sh = slot * 16u;
                    vals = (vals & ~(0xFFFFull << sh)) | (c << sh);
                    slot = slot == 2u ? 0u : slot + 1u;
                    tail = (tail + 1u) & 0xFFFFu;
                    __hip_atomic_store(&s_start[l], vals | ((uint64_t)tail << 48), __ATOMIC_RELEASE,
                                       __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            } else {
                __builtin_amdgcn_s_sleep(4);
            }
        }
        // un-draw what the env lane did not use (its final count is net of what sat in its registers)
        gl.to(g);
        const uint32_t head = __hip_atomic_load(&s_head[l], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
        for (uint32_t q = ((tail - head) & 0xFFFFu) * (IRR ? 2u : 1u); q > 0; q--) {
            const uint64_t lo = g.s_lo - g.inc_lo;
            const uint64_t hi = g.s_hi - g.inc_hi - (g.s_lo < g.inc_lo ? 1ULL : 0ULL);
            g.s_lo = lo * a.minv_lo;
            g.s_hi = __umul64hi(lo, a.minv_lo) + lo * a.minv_hi + hi * a.minv_lo;
        }
        g.store(a.env_s, i);
        return;
    }
    // E's side of the start-state ring
    uint32_t head16 = 0, hslot = 0;
    auto pull = [&]() __attribute__((always_inline)) {
        const uint64_t rt = __hip_atomic_load(&s_start[l], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
        const uint32_t avail = ((uint32_t)(rt >> 48) - head16) & 0xFFFFu;
        const uint32_t room = (uint32_t)kQQ - qn;
        const uint32_t take = avail < room ? avail : room;
#pragma unroll
        for (uint32_t t = 0; t < 3; t++) {
            if (t < take) {
                const uint32_t e = (uint32_t)(rt >> (16u * hslot)) & 0xFFFFu;
#pragma unroll
                for (int q = 0; q < kQQ; q++) queue[q] = (qn == (uint32_t)q) ? e : queue[q];
                qn++;
                hslot = hslot == 2u ? 0u : hslot + 1u;
            }
        }
        head16 = (head16 + take) & 0xFFFFu;
        __hip_atomic_store(&s_head[l], head16, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
    // every lane must hold a start state before a step may end its episode
    auto ensure_start = [&]() __attribute__((always_inline)) {
        if (!TRIO) { refill(); return; }
        uint32_t spins = 0;
        while (__builtin_amdgcn_ballot_w64(autoreset && qn == 0u) != 0) {
            pull();
            if (__builtin_amdgcn_ballot_w64(autoreset && qn == 0u) == 0) break;
            __builtin_amdgcn_s_sleep(1);
            if (++spins > kQSpinLimit) { status |= kQStatusInternal; qn = 1; break; }
        }
    };
    if (autoreset && isE && !TRIO && !ATNEED) refill();
    uint32_t phase = steps % every_n;

    // rewards of the unit path: s_rsel[(paid << 1) | terminal], filled above.  An LDS table on
    // purpose: a private float[4] gets a per-lane index and lands in scratch memory (an L2 round trip
    // per step), and selects among four values derived from DiscreteArgs made the compiler copy the
    // whole argument struct to scratch.

    constexpr uint32_t AW = IRR ? 2 : 1, OB = OBS64 ? 8 : 4;
    const uint32_t total = (uint32_t)K * N;
    auto r_act = __builtin_amdgcn_make_buffer_rsrc((void *)actions, 0, total * AW * 4u, kQRsrc);
    auto r_obs = __builtin_amdgcn_make_buffer_rsrc(obs, 0, total * AW * OB, kQRsrc);
    auto r_fin = __builtin_amdgcn_make_buffer_rsrc(final_obs ? final_obs : obs, 0, total * AW * OB, kQRsrc);
    auto r_rew = __builtin_amdgcn_make_buffer_rsrc((void *)reward, 0, total * 4u, kQRsrc);
    auto r_term = __builtin_amdgcn_make_buffer_rsrc((void *)term, 0, total, kQRsrc);
    auto r_trunc = __builtin_amdgcn_make_buffer_rsrc((void *)trunc, 0, total, kQRsrc);
    const uint32_t vact = i * AW * 4u, vobs = i * AW * OB, v4 = i * 4u, v1 = i;
    const uint32_t row_act = N * AW * 4u, row_obs = N * AW * OB;

    constexpr int kPre = 8;
    auto load_act = [&](int k) __attribute__((always_inline)) -> u32x2 {
        const uint32_t kk = (uint32_t)min(k, K - 1);
        if (IRR) return __builtin_amdgcn_raw_buffer_load_b64(r_act, vact, kk * row_act, 0);
        return u32x2{__builtin_amdgcn_raw_buffer_load_b32(r_act, vact, kk * row_act, 0), 0u};
    };
    auto put_obs = [&](decltype(r_obs) rs, uint32_t so, uint32_t s0, uint32_t s1) __attribute__((always_inline)) {
        if (IRR) {
            if (OBS64) __builtin_amdgcn_raw_buffer_store_b128(u32x4{s0, 0u, s1, 0u}, rs, vobs + so * row_obs, 0, MDPP_ST_NT);   // (see kQRsrc)
            else __builtin_amdgcn_raw_buffer_store_b64(u32x2{s0, s1}, rs, vobs, so * row_obs, MDPP_ST_NT);
        } else {
            if (OBS64) __builtin_amdgcn_raw_buffer_store_b64(u32x2{s0, 0u}, rs, vobs, so * row_obs, MDPP_ST_NT);
            else __builtin_amdgcn_raw_buffer_store_b32(s0, rs, vobs, so * row_obs, MDPP_ST_NT);
        }
    };

    // XR, E's side: ep = position of the next draw; (xm0, xm1, xm2, xv) = x_meta[ep .. ep + 2], x_val[ep], fetched at the end of
    // the previous step; xhh = positions X has made, as last read
    uint32_t ep = 0, xhh = 0, xm0 = 0, xm1 = 0, xm2 = 0;
    double xv = 0.0;
    auto x_ensure = [&](uint32_t upto) __attribute__((always_inline)) {     // positions < upto are made
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(upto > xhh) != 0, 0)) {
            uint32_t spins = 0;
            xhh = __hip_atomic_load(&x_hhead[l], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
            while (__builtin_amdgcn_ballot_w64(upto > xhh) != 0) {
                __hip_atomic_store(&x_epos[l], ep, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);     // (X's window follows E)
                __builtin_amdgcn_s_sleep(1);
                xhh = __hip_atomic_load(&x_hhead[l], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (++spins > kQSpinLimit) { status |= kQStatusInternal; xhh = upto; break; }
            }
        }
    };
    auto x_fetch = [&]() __attribute__((always_inline)) {
        x_ensure(ep + 3u);
        xm0 = x_meta[ep & (uint32_t)(XRN - 1)][l];
        xm1 = x_meta[(ep + 1u) & (uint32_t)(XRN - 1)][l];
        xm2 = x_meta[(ep + 2u) & (uint32_t)(XRN - 1)][l];
        if (!rn_z0) xv = x_val[(ep & (uint32_t)(XRN - 1)) * kBlock + l];
    };
    if constexpr (XR) { if (role == 0) x_fetch(); }
    // ---- E: one step of the state recurrence -> record
    auto stepE = [&](const u32x2 act2, double &z, const int kstep) __attribute__((always_inline)) -> uint64_t {
        uint32_t hent = 0;           // NPH: what the producers made for this step
        if constexpr (NPH > 0) hent = s_hm[(kstep % kHD) * kBlock + l];
        const uint64_t ptick = ptick0 + (uint64_t)kstep;        // (Philox streams)
        if (!ATNEED && __builtin_expect(__builtin_amdgcn_ballot_w64(autoreset && qn == 0u) != 0, 0)) ensure_start();
        int action = (int)act2.x;
        bool bad = false;
        if (!SF || __builtin_expect(__builtin_amdgcn_ballot_w64((uint32_t)action >= A) != 0, 0)) {
            action += (action < 0 && action >= -(int)A) ? (int)A : 0;       // numpy negative indexing
            bad = action < 0 || action >= (int)A;
            action = bad ? 0 : action;
        }
        const uint32_t cur = (uint32_t)hist & 0xFFu;
        uint32_t nxt = P[SF ? __umul24(cur, A) + (uint32_t)action : cur * A + (uint32_t)action];   // D1
        bool done_sf = false;
        if constexpr (SF) { done_sf = nxt > 0x7Fu; nxt &= 0x7Fu; }          // (bit 7 of the entry: D7)
        if constexpr (PN && PH) {                                            // D2, Philox streams: mdpp_rng.hpp philox_pnoise_*
            uint32_t ent = hent;
            if constexpr (NPH == 0) ent = philox_pnoise_index(pnw.word(a.philox_seed, genv, ptick, kPhiloxPNoiseStream), a.pn_T, pn_M);
            const uint32_t j = ent & 0xFFu;
            nxt = (ent & 0x100u) ? j + (j >= nxt ? 1u : 0u) : nxt;          // (a reset call's result is dropped below)
        }
        if constexpr (PN && !PH) {                                           // D2 (:1604-1622)
            uint64_t m = 0;
            if (!pend) m = sp.next64() >> 11;
            const uint64_t *row = TN + nxt * S8;
            uint32_t c = 0;
            for (uint32_t b = 0; b < S8; b += 8) {
#pragma unroll
                for (uint32_t j = 0; j < 8; j++) c += (row[b + j] <= m) ? 1u : 0u;
            }
            nxt = c;
        }
        if constexpr (SF) {                                                  // sequence_length 1: the key is the state
            key = nxt;
        } else {
            const uint32_t oldest = (uint32_t)(hist >> (8 * (L - 1))) & 0xFFu;   // leaves the L-window
            key = (key - (oldest == 0xFFu ? 0u : oldest) * spow) * S + nxt;     // D4 key, carried
        }
        hist = (hist << 8) | nxt;                                            // D3
        valid = min(valid + 1u, L + 1u);
        steps += 1;
        phase = (phase + 1 >= every_n) ? 0u : phase + 1;
        bool done = done_sf;
        if constexpr (!SF) done = is_term[nxt] != 0;                         // D7
        uint32_t bad1 = 0;
        if (IRR) {                                                           // :2063-2082
            int action1 = (int)act2.y;
            action1 += (action1 < 0 && action1 >= -a.A1) ? a.A1 : 0;
            bad1 = (action1 < 0 || action1 >= a.A1) ? 1u : 0u;
            action1 = bad1 ? 0 : action1;
            cur1 = P1[cur1 * (uint32_t)a.A1 + (uint32_t)action1];
            if constexpr (PN && PH) {
                const uint32_t ent = philox_pnoise_index(pnw1.word(a.philox_seed, genv, ptick, kPhiloxIrrStream), a.pn_T, pn_M1);
                const uint32_t j = ent & 0xFFu;
                cur1 = (ent & 0x100u) ? j + (j >= cur1 ? 1u : 0u) : cur1;
            }
            if constexpr (PN && !PH) {                                       // its own P-noise stream (:2066-2080)
                uint64_t m1 = 0;
                if (!pend) m1 = sp1.next64() >> 11;
                const uint64_t *row = TN1 + cur1 * S18;
                uint32_t c = 0;
                for (uint32_t b = 0; b < S18; b += 8) {
#pragma unroll
                    for (uint32_t j = 0; j < 8; j++) c += (row[b + j] <= m1) ? 1u : 0u;
                }
                cur1 = c;
            }
        }
        status |= ((bad || bad1) && !pend) ? (uint32_t)MDPP_STATUS_BAD_ACTION : 0u;
        uint32_t x_cnt = 0, x_ss = 0;                                       // XR: the words this step's normal took, the start state behind them
        if constexpr (XR) {
            // this step's draws on the env stream: the normal that starts at position ep, then -- if the episode ends -- one word
            uint32_t kind = (xm0 >> 8) & 3u;
            if (__builtin_expect(__builtin_amdgcn_ballot_w64(kind >= 2u) != 0, 0)) {
                uint32_t guard = 0;
                while (__builtin_amdgcn_ballot_w64(kind == 2u) != 0) {      // wedge point rejected: the draw starts over two words on
                    const bool red = kind == 2u;
                    ep += red ? 2u : 0u;
                    const uint32_t o0 = xm0, o1 = xm1, o2 = xm2;
                    const double ox = xv;
                    x_fetch();
                    if (!red) { xm0 = o0; xm1 = o1; xm2 = o2; xv = ox; }
                    kind = (xm0 >> 8) & 3u;
                    if (++guard > 64u) { status |= kQStatusInternal; break; }
                }
            }
            x_cnt = kind == 0u ? 1u : 2u;
            x_ss = (kind == 0u ? xm1 : xm2) & 0xFFu;
            if (kind == 3u) { x_cnt = (xm0 >> 16) & 0xFFu; x_ss = xm0 >> 24; }      // tail: counted words, the start state behind them
            z = xv;
        } else
        if (RN) {                                                           // D6: drawn in reward_function, before any reset
            if constexpr (NPH > 0) z = (double)s_hz[(kstep % kHD) * kBlock + l];
            else if constexpr (PH) z = (double)rnz.normal(a.philox_seed, genv, ptick, kPhiloxRNoiseStream);
            else { z = 0.0; if (!pend) { if (rn_z0) np_skip_normal_lds(g, zig); else z = np_standard_normal_lds(g, zig); } }   // (sigma 0: 0.0 + 0.0 z is +0.0 for every z -- the stream's advance alone)
        }
        bool tr = has_max && steps >= max_steps;
        bool need = autoreset && (done || tr);
        bool done_out = done;
        if (nextmode) {                           // the reset one call later: what this lane just computed is dropped
            const bool ended = (done || tr) && !pend;
            need = pend;
            done_out = pend ? false : done;
            tr = pend ? false : tr;
            pend = ended;
        }
        if constexpr (XR) {                                                  // reset(): the word behind the normal's, evaluated by X
            queue[0] = need ? x_ss : queue[0];
            qn = need ? 1u : qn;
            ep += x_cnt + (need ? 1u : 0u);
            __hip_atomic_store(&x_epos[l], ep, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);     // (X's window follows E)
            x_fetch();
        } else
        if (ATNEED && __builtin_amdgcn_ballot_w64(need) != 0) {              // reset(): drawn now, in stream order
            if constexpr (NPH > 0) { queue[0] = need ? (hent >> 16) : queue[0]; }
            else if (need) { queue[0] = draw_state(ptick0 + (uint64_t)kstep); }
            qn = need ? 1u : qn;
        }
        uint32_t hi = (done_out ? 1u : 0u) | (tr ? 2u : 0u) | (need ? 4u : 0u) | (valid > L ? 8u : 0u) |
                      (phase == 0 ? 16u : 0u) | (key << 5);
        uint32_t lo = (nxt << 8) | (cur1 << 24);
        // reset(): pop the next queued start state where the episode ended (:2250-2278)
        const uint32_t s0 = queue[0] & 0xFFu, s1 = queue[0] >> 8;
#pragma unroll
        for (int q = 0; q + 1 < kQQ; q++) queue[q] = need ? queue[q + 1] : queue[q];
        qn -= need ? 1u : 0u;
        hist = need ? (0xFFFFFFFFFFFFFF00ULL | (uint64_t)s0) : hist;
        key = need ? s0 : key;
        valid = need ? 1u : valid;
        steps = need ? 0u : steps;
        phase = need ? 0u : phase;
        if (IRR) cur1 = need ? s1 : cur1;
        lo |= (need ? s0 : nxt) | (cur1 << 16);
        return ((uint64_t)hi << 32) | lo;
    };
    // ---- O: record -> reward, delay line, all global stores of step `so`
    auto emitO = [&](const uint64_t rec, const double z, const uint32_t so) __attribute__((always_inline)) {
        const uint32_t lo = (uint32_t)rec, hi = (uint32_t)(rec >> 32);
        const uint32_t k2 = hi >> 5;
        const uint32_t done = hi & 1u;
        float rout;
        uint32_t bit = 0;
        if constexpr (UR) {
        bit = (rbits[k2 >> 3] >> (k2 & 7u)) & 1u;
        bit = (hi & 8u) ? bit : 0u;                                          // NaN gate: fewer than L transitions yet
        const uint32_t outb = (ringbits >> ((delay - 1u) & 31u)) & 1u;      // D5 (shift register)
        ringbits = delay > 0 ? ((ringbits << 1) | bit) : ringbits;
        bit = delay > 0 ? outb : bit;
        bit = (hi & 16u) ? bit : 0u;                                         // D6
        }
        if constexpr (!UR) {                                                 // k_discrete_step<UNIT = false>, :1821-1845, :1968-1990
            uint32_t key = (hi & 8u) ? k2 : kNoKey;                          // NaN gate: no key yet
            if (delay > 0) {                                                 // D5: the key waits `delay` steps in HBM
                uint32_t *slot = a.ring_keys + (size_t)((rhead0 + so) % delay) * N + i;
                const uint32_t out = *slot;
                *slot = key;
                key = out;
            }
            double r = (key != kNoKey) ? ((const double *)rbits)[key] : 0.0;
            r = (hi & 16u) ? r : 0.0;                                        // D6: steps % every_n
            if (RN) r += 0.0 + a.r_noise * z;
            r *= a.scale;
            r += a.shift;
            if (done) r += a.term_add;
            rout = (float)r;
        } else if (RN) {                                                     // :1980-1990, :2107 in float64
            double r = bit ? 1.0 : 0.0;
            r += 0.0 + a.r_noise * z;
            r *= a.scale;
            r += a.shift;
            if (done) r += a.term_add;
            rout = (float)r;
        } else {
            rout = s_rsel[(bit << 1) | done];
        }
        const bool need = (hi & 4u) != 0;
        if (nextmode) rout = need ? 0.0f : rout;                             // the reset call pays 0.0
        if (final_obs && !nextmode && __builtin_amdgcn_ballot_w64(need) != 0) {
            if (need) put_obs(r_fin, so, (lo >> 8) & 0xFFu, lo >> 24);
        }
        ringbits = need ? 0u : ringbits;
        if constexpr (!UR) {                                                 // reset() empties the delay line (:2250)
            if (__builtin_amdgcn_ballot_w64(need) != 0 && delay > 0) {
                if (need) for (uint32_t dd = 0; dd < delay; dd++) a.ring_keys[(size_t)dd * N + i] = kNoKey;
            }
        }
        put_obs(r_obs, so, lo & 0xFFu, (lo >> 16) & 0xFFu);
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(rout), r_rew, v4, so * N * 4u, MDPP_ST_NT);
        __builtin_amdgcn_raw_buffer_store_b8((uint8_t)done, r_term, v1, so * N, MDPP_ST_NT);
        __builtin_amdgcn_raw_buffer_store_b8((uint8_t)((hi >> 1) & 1u), r_trunc, v1, so * N, MDPP_ST_NT);
    };

    if (!DUO) {
        u32x2 pre[kPre];
#pragma unroll
        for (int u = 0; u < kPre; u++) pre[u] = load_act(u);
        const int nfull = K / kPre;
        for (int c = 0; c < nfull; c++) {
#pragma unroll
            for (int u = 0; u < kPre; u++) {
                const u32x2 act = pre[u];
                pre[u] = load_act(c * kPre + kPre + u);
                double z = 0.0;
                const uint64_t rec = stepE(act, z, c * kPre + u);
                emitO(rec, z, (uint32_t)(c * kPre + u));
            }
        }
        for (int k = nfull * kPre; k < K; k++) {
            u32x2 act = pre[0];
#pragma unroll
            for (int u = 1; u < kPre; u++) act = (k - nfull * kPre == u) ? pre[u] : act;
            double z = 0.0;
            const uint64_t rec = stepE(act, z, k);
            emitO(rec, z, (uint32_t)k);
        }
    } else if (role == 0) {
        // -------------------------------------------------------------- E waves
        __builtin_amdgcn_s_setprio(kPrioE);
        // Actions are fetched kEAh chunks ahead of their use; the buffers rotate by NAME (the slot loop is unrolled): copying a
        // register whose load is in flight makes the wave wait for it.
#ifndef MDPP_Q_EAHEAD
#define MDPP_Q_EAHEAD 1         /* (1 / 2 / 4 chunks ahead measure the same: 172-173 us at S = 50 -- the loads of one chunk ahead are hidden) */
#endif
        constexpr int kEAh = (ROLES == 3 && !PN && !IRR && !PH && NPH == 0) ? MDPP_Q_EAHEAD : 1;     // (the larger step bodies do not unroll over the slots: the array would go to scratch)
        static_assert(kEAh == 1 || kEAh == 2 || kEAh == 4, "named buffers");
        u32x2 preq[kEAh][kPre];      // slot j holds the actions of the chunks c = j (mod kEAh)
#pragma unroll
        for (int q = 0; q < kEAh; q++)
#pragma unroll
            for (int u = 0; u < kPre; u++) preq[q][u] = load_act(q * kPre + u);
        const int nchunks = (K + kPre - 1) / kPre;
        // (no lambda around the chunk: an array indexed through a closure stays in scratch memory -- 80 B per lane and 340 us per
        //  launch instead of 183, measured; the slot loop below is unrolled, so preq[j] is a register array by name)
        for (int c0 = 0; c0 < nchunks; c0 += kEAh) {
#pragma unroll
        for (int j = 0; j < kEAh; j++) {
            const int c = c0 + j;
            if (c >= nchunks) continue;
            const int kbase = c * kPre;
            if (kbase + kPre > kDepth) {                // stay within the ring: at most kDepth - 8 steps ahead of O
                const uint32_t must = (uint32_t)(kbase + kPre - kDepth);
                uint32_t spins = 0;
                while (__hip_atomic_load(&s_cons[w], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < must) {
                    __builtin_amdgcn_s_sleep(1);
                    if (++spins > kQSpinLimit) { status |= kQStatusInternal; break; }
                }
            }
            if (TRIO && autoreset) pull();
            if constexpr (NPH > 0) {                    // the producers must be through this chunk's four-tick blocks
                const int upto = min(kbase + kPre, K);
                const uint64_t G0 = ptick0 >> 2;
                const int r_last = (int)(((ptick0 + (uint64_t)upto - 1u) >> 2) - G0);
#pragma unroll
                for (int p = 0; p < NPH; p++) {
                    if (r_last < p) continue;
                    const int r_p = r_last - ((r_last - p) % NPH);          // producer p's last block that starts before `upto`
                    const int64_t hi = (int64_t)((G0 + (uint64_t)r_p + 1u) << 2) - (int64_t)ptick0;
                    const uint32_t want = (uint32_t)(hi < (int64_t)K ? hi : (int64_t)K);
                    uint32_t spins = 0;
                    while (__hip_atomic_load(&s_hprod[p][w], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < want) {
                        __builtin_amdgcn_s_sleep(1);
                        if (++spins > kQSpinLimit) { status |= kQStatusInternal; break; }
                    }
                }
            }
            if (kbase + kPre <= K) {
#pragma unroll
                for (int u = 0; u < kPre; u++) {
                    const u32x2 act = preq[j][u];
                    preq[j][u] = load_act(kbase + kEAh * kPre + u);
                    double z = 0.0;
                    ring[((kbase + u) % kDepth) * kBlock + l] = stepE(act, z, kbase + u);
                    if (RN && !rn_z0) ringz[((kbase + u) % kDepth) * kBlock + l] = z;
                }
            } else {
                for (int k = kbase; k < K; k++) {
                    u32x2 act = preq[j][0];
#pragma unroll
                    for (int u = 1; u < kPre; u++) act = (k - kbase == u) ? preq[j][u] : act;
                    double z = 0.0;
                    ring[(k % kDepth) * kBlock + l] = stepE(act, z, k);
                    if (RN && !rn_z0) ringz[(k % kDepth) * kBlock + l] = z;
                }
            }
            if ((l & 63) == 0)
                __hip_atomic_store(&s_prod[w], (uint32_t)min(kbase + kPre, K), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        }
    } else {
        // -------------------------------------------------------------- O waves
        __builtin_amdgcn_s_setprio(kPrioO);
        const int nchunks = (K + kPre - 1) / kPre;
        for (int c = 0; c < nchunks; c++) {
            const int kbase = c * kPre;
            const uint32_t upto = (uint32_t)min(kbase + kPre, K);
            uint32_t spins = 0;
            while (__hip_atomic_load(&s_prod[w], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < upto) {
                __builtin_amdgcn_s_sleep(1);
                if (++spins > kQSpinLimit) { status |= kQStatusInternal; break; }
            }
            if (kbase + kPre <= K) {
                uint64_t rec[kPre];
                double zz[kPre];
#pragma unroll
                for (int u = 0; u < kPre; u++) {
                    rec[u] = ring[((kbase + u) % kDepth) * kBlock + l];
                    zz[u] = (RN && !rn_z0) ? ringz[((kbase + u) % kDepth) * kBlock + l] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < kPre; u++) emitO(rec[u], zz[u], (uint32_t)(kbase + u));
            } else {
                for (int k = kbase; k < K; k++)
                    emitO(ring[(k % kDepth) * kBlock + l], (RN && !rn_z0) ? ringz[(k % kDepth) * kBlock + l] : 0.0, (uint32_t)k);
            }
            if ((l & 63) == 0)
                __hip_atomic_store(&s_cons[w], upto, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
    if constexpr (!PH) {
        if (PN && isE) sp.store(a.sp_s, i);
        if (PN && IRR && isE) sp1.store(a.sp1_s, i);
    }
    if (XR && role == 0) {
        // the position E reached (X un-draws what lies beyond), then that this wave is through
        __hip_atomic_store(&x_epos[l], ep, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        if ((l & 63) == 0) __hip_atomic_fetch_add(&s_done, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else if (TRIO && role == 0) {
        // tell H how many of its start states were really used, then that this wave is through
        __hip_atomic_store(&s_head[l], (head16 - qn) & 0xFFFFu, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        if ((l & 63) == 0) __hip_atomic_fetch_add(&s_done, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (IRR) a.irr_state[i] = cur1;
    } else if (isE) {
        if constexpr (!PH) {
            // un-draw what was not used: s_prev = (s - inc) * M^-1 (mod 2^128)
            for (uint32_t q = qn * (IRR ? 2u : 1u); q > 0; q--) {
                const uint64_t lo = g.s_lo - g.inc_lo;
                const uint64_t hi = g.s_hi - g.inc_hi - (g.s_lo < g.inc_lo ? 1ULL : 0ULL);
                g.s_lo = lo * a.minv_lo;
                g.s_hi = __umul64hi(lo, a.minv_lo) + lo * a.minv_hi + hi * a.minv_lo;
            }
            g.store(a.env_s, i);
        }
        if (IRR) a.irr_state[i] = cur1;
    }
    if (!DUO) {
        a.state[i] = make_uint4((uint32_t)hist, (uint32_t)(hist >> 32), steps | (pend ? 0x80000000u : 0u), ringbits);
    } else {
        uint32_t *st32 = (uint32_t *)&a.state[i];
        if (role == 0) { st32[0] = (uint32_t)hist; st32[1] = (uint32_t)(hist >> 32); st32[2] = steps | (pend ? 0x80000000u : 0u); }
        else st32[3] = ringbits;                        // the delay line belongs to the O lane
    }
    if (status) atomicOr(&a.status[i], status);
}

#ifndef MDPP_QUIET_TU_NU
#define MDPP_QUIET_TU_NU 0         // 1: this translation unit holds the non-unit-reward instantiations (mdpp_discrete_quiet_nu.hip)
#endif
template <bool O64, bool IR, int ROLES, bool PN, bool RN, bool PH = false, int NPH = 0, bool UR = true, bool SF = false, bool PE = false>
static void quiet_launch(const DiscreteArgs &a, const DiscreteIO &io, size_t lds) {
    if (io.name_out) {              // (trailing default arguments are named only when set)
        snprintf(io.name_out, kNameLen, "k_discrete_rollout_quiet<OBS64=%d,IRR=%d,ROLES=%d,PN=%d,RN=%d,PHILOX=%d,NPH=%d%s%s%s>", O64, IR, ROLES, PN, RN,
                 PH, NPH, UR ? "" : ",UNIT=0", SF ? ",SF=1" : "", PE ? ",PE=1" : "");
        return;
    }
    auto kern = k_discrete_rollout_quiet<O64, IR, ROLES, PN, RN, PH, NPH, UR, SF, PE>;
    if (lds > 48 * 1024) {                        // tables + record ring beyond the default dynamic-LDS limit
        static size_t allowed = 0;                // (per instantiation)
        if (lds > allowed) {
            (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            allowed = lds;
        }
    }
    const int grid = (a.N + kBlock - 1) / kBlock;
    launch_rollout(kern, grid, (ROLES + NPH) * kBlock, lds, a, io);
}

#if MDPP_QUIET_TU_NU
// The non-unit-reward form (UR = false): numpy streams, no irrelevant sub-space, sequence rewards (not the custom R(s, a)
// matrix, whose key E does not make).  Same role rules as below.
bool launch_discrete_quiet_nu(const DiscreteArgs &a, const DiscreteIO &io) {
    const int K = io.K;
    if (!a.shared_tables || a.unit_rewards || a.rew_sa || !a.rew_in_lds || a.irr || a.philox || K < 16 || (a.opts & MDPP_OPT_NO_QUIET))
        return false;
    if (a.nkeys >= (1u << 27) || (a.delay > 0 && !a.ring_keys)) return false;       // (the record carries 27 bits of key)
    if (a.autoreset == MDPP_AUTORESET_NEXT_STEP) return false;                       // (the reset call's ring handling: general kernel)
    const bool pn = a.has_p_noise != 0, rn = a.has_r_noise != 0;
    if ((pn || rn) && (a.opts & MDPP_OPT_NO_QUIET_NOISE)) return false;
    if ((unsigned long long)K * a.N * 8ULL >= (1ULL << 32)) return false;
    const size_t S8 = (size_t)((a.S + 7) & ~7);
    size_t lds = ((a.lds_bytes + 15) & ~(size_t)15) + S8 * 8;
    if (pn) lds += (size_t)a.S * S8 * 8;
    if (lds > 60 * 1024) return false;
    const size_t depth = rn ? 16 : kQDepth;
    // (sigma 0 on numpy streams: the records carry no normal -- 32 KiB less, two workgroups per CU)
    const bool rz0 = rn && !a.philox && a.r_noise == 0.0 && !(a.opts & MDPP_OPT_NO_SIGMA0);
    const size_t lds_duo = ((lds + 15) & ~(size_t)15) + depth * kBlock * ((rn && !rz0) ? 16 : 8);
    const bool duo = (a.N % kBlock) == 0 && K >= 32 && lds_duo <= 120 * 1024 && !(a.opts & MDPP_OPT_NO_DUO);
    const bool trio = duo && a.autoreset && !rn && !(a.opts & MDPP_OPT_NO_TRIO);
    // XR (kernel header): reward noise alone -- a third wave evaluates the env stream by position (+ 52 KiB of static LDS)
    // (XR's static LDS: 16 KiB of position records, the ziggurat tables, the bucket table, counters ~ 36 KiB; its values ring -- 32 KiB,
    //  none at sigma 0 -- rides behind the record ring in dynamic LDS)
    const size_t xr_val_bytes = (rn && !(a.r_noise == 0.0 && !(a.opts & MDPP_OPT_NO_SIGMA0))) ? (size_t)kXR * kBlock * 8 : 0;
    const bool xr = duo && rn && !pn && lds_duo + xr_val_bytes <= 120 * 1024 && !(a.opts & MDPP_OPT_NO_TRIO);
    const int roles = (trio || xr) ? 3 : duo ? 2 : 1;
    // SF (kernel header): the reference's sweep defaults fixed at compile time
    const bool sf = roles == 3 && !pn && a.L == 1 && a.autoreset == MDPP_AUTORESET_SAME_STEP && a.max_steps == 0 && a.every_n == 1 &&
                    a.S <= 128 && !(a.opts & MDPP_OPT_NO_QUIET_SF);
    const size_t l = roles == 1 ? lds : lds_duo + (xr ? xr_val_bytes : 0);
    with_bools([&](auto O64, auto PN, auto RN, auto SF) {
        with_value<1, 2, 3>(roles, [&](auto R) {
            if constexpr (SF()) { if constexpr (R() == 3 && !PN()) quiet_launch<O64(), false, 3, PN(), RN(), false, 0, false, true>(a, io, l); }
            else if constexpr (R() == 3) { if constexpr (!RN() || !PN()) quiet_launch<O64(), false, 3, PN(), RN(), false, 0, false>(a, io, l); }
            else quiet_launch<O64(), false, R(), PN(), RN(), false, 0, false>(a, io, l);
        });
    }, !a.obs_i32, pn, rn, sf);
    return true;
}
#else
bool launch_discrete_quiet_nu(const DiscreteArgs &a, const DiscreteIO &io);
// Serves the launch if the handle and the launch shape qualify; false = not taken.
bool launch_discrete_quiet(const DiscreteArgs &a, const DiscreteIO &io) {
    if (!a.unit_rewards) return launch_discrete_quiet_nu(a, io);
    const int K = io.K;
    if (!a.shared_tables) {
        // PE (kernel header): one MDP per env, each lane's tables in its slot of the workgroup's LDS, three roles
        const bool rn = a.has_r_noise != 0;
        if (!a.rew_in_lds || a.irr || a.philox || a.has_p_noise || a.S > 16 || K < 32 || (a.N % kBlock) != 0 ||
            a.autoreset == MDPP_AUTORESET_NEXT_STEP || (!rn && !a.autoreset) ||
            (a.opts & (MDPP_OPT_NO_QUIET | MDPP_OPT_NO_DUO | MDPP_OPT_NO_TRIO)) || (rn && (a.opts & MDPP_OPT_NO_QUIET_NOISE)))
            return false;
        if ((unsigned long long)K * a.N * 8ULL >= (1ULL << 32)) return false;
        const size_t S8 = (size_t)((a.S + 7) & ~7);
        const size_t pe_rew = ((size_t)a.S * a.A + a.S + 7) & ~(size_t)7, pe_T0 = (pe_rew + a.rbits_stride + 7) & ~(size_t)7;
        const size_t stride = pe_T0 + S8 * 8 + 8;             // (the kernel's carve of a lane's slot)
        const size_t depth = rn ? 16 : kQDepth;
        const bool z0 = rn && a.r_noise == 0.0 && !(a.opts & MDPP_OPT_NO_SIGMA0);
        const size_t l = ((stride * kBlock + 15) & ~(size_t)15) + depth * kBlock * ((rn && !z0) ? 16 : 8) + ((rn && !z0) ? (size_t)kXR * kBlock * 8 : 0);
        if (l + (rn ? 32u : 20u) * 1024u > 160u * 1024u) return false;     // (+ the instantiation's static LDS: X's meta ring, ziggurat tables, counters)
        const bool sf = a.L == 1 && a.autoreset == MDPP_AUTORESET_SAME_STEP && a.max_steps == 0 && a.every_n == 1 &&
                        !(a.opts & MDPP_OPT_NO_QUIET_SF);
        with_bools([&](auto O64, auto RN, auto SF) {
            quiet_launch<O64(), false, 3, false, RN(), false, 0, true, SF(), true>(a, io, l);
        }, !a.obs_i32, rn, sf);
        return true;
    }
    if (!a.shared_tables || !a.unit_rewards || !a.rew_in_lds || a.fast_ok || K < 16 || (a.opts & MDPP_OPT_NO_QUIET))
        return false;
    if (a.philox && (a.opts & MDPP_OPT_NO_PHILOX_FAST)) return false;
    const bool ph = a.philox != 0;
    const bool pn = a.has_p_noise != 0, rn = a.has_r_noise != 0;
    if ((pn || rn) && (a.opts & MDPP_OPT_NO_QUIET_NOISE)) return false;
    const unsigned long long bytes = (unsigned long long)K * a.N * (a.irr ? 2 : 1) * 8ULL;
    if (bytes >= (1ULL << 32)) return false;                    // buffer descriptors address < 4 GiB per array
    const size_t S8 = (size_t)((a.S + 7) & ~7);
    size_t lds = a.lds_bytes;
    lds = ((lds + (a.irr ? (size_t)a.S1 * a.A1 : 0) + 15) & ~(size_t)15) + S8 * 8 + (a.irr ? (size_t)((a.S1 + 7) & ~7) * 8 : 0);
    const bool ph_ = a.philox != 0;
    if (pn && !ph_) lds += (size_t)a.S * S8 * 8;                // thresholds of the S noise categoricals (numpy streams)
    if (pn && !ph_ && a.irr) lds += (size_t)a.S1 * ((a.S1 + 7) & ~7) * 8;
    if (lds > 60 * 1024) return false;
    // two / three waves per SIMD (E / O / H roles) when the blocks are full and the rollout is long
    // enough to fill the ring
    const size_t depth = rn ? 16 : kQDepth;
    const bool rz0 = rn && !a.philox && a.r_noise == 0.0 && !(a.opts & MDPP_OPT_NO_SIGMA0);      // (as above)
    const size_t lds_duo = ((lds + 15) & ~(size_t)15) + depth * kBlock * ((rn && !rz0) ? 16 : 8);
    const bool duo = (a.N % kBlock) == 0 && K >= 32 && lds_duo <= 120 * 1024 && !(a.opts & MDPP_OPT_NO_DUO);
    const bool trio = duo && a.autoreset && !rn && !ph && !(a.opts & MDPP_OPT_NO_TRIO);
    // XR (kernel header): reward noise alone on numpy streams -- a third wave evaluates the env stream by position (+ 52 KiB of
    // static LDS); gymnasium's next-step autoreset (the reset call must not draw) stays on two roles
    const size_t xr_val_bytes = (rn && !(a.r_noise == 0.0 && !(a.opts & MDPP_OPT_NO_SIGMA0))) ? (size_t)kXR * kBlock * 8 : 0;
    const bool xr = duo && rn && !pn && !ph && !a.irr && a.autoreset != MDPP_AUTORESET_NEXT_STEP && lds_duo + xr_val_bytes <= 120 * 1024 &&
                    !(a.opts & MDPP_OPT_NO_TRIO);
    const int roles = (trio || xr) ? 3 : duo ? 2 : 1;
    // SF (kernel header): the reference's sweep defaults fixed at compile time
    const bool sf = roles == 3 && !pn && !ph && !a.irr && a.L == 1 && a.autoreset == MDPP_AUTORESET_SAME_STEP && a.max_steps == 0 &&
                    a.every_n == 1 && a.S <= 128 && !(a.opts & MDPP_OPT_NO_QUIET_SF);
    // Philox handles in two roles without an irrelevant sub-space: two producer waves on top (see NPH)
    const int nph = (ph && duo && !a.irr && a.autoreset && lds_duo + 72 * 1024 <= 150 * 1024 &&
                     !(a.opts & MDPP_OPT_NO_TRIO)) ? 2 : 0;
    const size_t l = roles == 1 ? lds : lds_duo + (xr ? xr_val_bytes : 0);
    with_bools([&](auto O64, auto IR, auto PN, auto RN, auto PH, auto NPH2, auto SF) {
        with_value<1, 2, 3>(roles, [&](auto R) {
            if constexpr (PH()) {       // (Philox: one or two roles; SF is a numpy-stream form)
                if constexpr (NPH2()) { if constexpr (!IR() && R() == 2 && !SF()) quiet_launch<O64(), IR(), 2, PN(), RN(), true, 2>(a, io, l); }
                else if constexpr (R() < 3 && !SF()) quiet_launch<O64(), IR(), R(), PN(), RN(), true>(a, io, l);
            }
            else if constexpr (SF()) { if constexpr (R() == 3 && !PN() && !IR()) quiet_launch<O64(), IR(), 3, PN(), RN(), false, 0, true, true>(a, io, l); }
            else if constexpr (R() == 3) { if constexpr (!RN() || (!PN() && !IR())) quiet_launch<O64(), IR(), 3, PN(), RN()>(a, io, l); }
            else quiet_launch<O64(), IR(), R(), PN(), RN()>(a, io, l);
        });
    }, !a.obs_i32, a.irr != 0, pn, rn, ph, nph == 2, sf);
    return true;
}
#endif   // !MDPP_QUIET_TU_NU

} // namespace mdpp
