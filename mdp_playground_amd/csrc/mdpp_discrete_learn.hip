// In-kernel tabular TD learners: one Q-learning or SARSA agent per env instance, its Q-table beside the env state, K steps of
// "select epsilon-greedily from the env's own Q, step, update that Q" in ONE launch (mdpp_step_n_learn).
//
// The learner of env g = env_id_offset + i is (algo, alpha, gamma, E = ceil(epsilon 2^31), seed, Q float32 [S][A]).  At step counter
// t in state s:
//   sel(s, t):  wE = word (t & 3) of block 0 of the Philox4x32-10 stream (seed, g, t >> 2, kPhiloxLearnExploreStream);
//               (wE >> 1) < E: explore,  a = (uint64(wA) A) >> 32  with wA the same word of kPhiloxLearnActionStream;
//               otherwise the lowest j maximising Q[s][j]
//   step:       mdpp_step_n's with that action -> float32 reward r as written, terminated, truncated, the true next state s'
//   target:     terminated: y = r;  q_learning: y = r + gamma max_j Q[s'][j];  sarsa: y = r + gamma Q[s'][a'], a' = sel(s', t + 1) on
//               Q BEFORE this step's update;  float32, one rounding per operation (the unit is built with -ffp-contract=off)
//   update:     q = Q[s][a];  d = y - q;  u = alpha d;  Q[s][a] = q + u
//   carry:      sarsa: when the env's next step of the same call starts from s' (no termination, no reset in between) it takes
//               a' and does not select again; a call's first step selects afresh (the one departure from textbook SARSA: there
//               is no per-env learner state besides Q)
//   reset call of a next-step-autoreset env: an action is selected from the state in the record, written and ignored; no update.
// The learner reads no stream of the env, so the launch leaves every stream, the state record and the step counter where
// mdpp_step_n fed with the same actions leaves them.
//
// The step restates k_discrete_step (mdpp_discrete.hip) D1-D7 and R1 WITH its NOISE branches (transition noise through the
// categorical's cdf / philox_pnoise_state, reward noise through numpy's ziggurat with the tables in LDS / PhiloxTickNormals)
// and without its IRR branches and episode statistics; fast_ok handles keep their queue of start states as in
// mdpp_discrete_policy.hip.  One lane per env, 256-thread workgroups, outputs through range-checked non-temporal buffer stores.
//
// Q lives in a buffer of the handle, entry-major [S A][N]: lanes of a wave touching their own entry of the same (s, a)
// coalesce.  QLDS = 1: each lane's table is staged once per launch into q_lds[(s A + a) 256 + tid] (bank = lane: no conflict
// whatever (s, a) each lane holds), every selection and update is LDS traffic, the tables are written back at the end.
// QLDS = 0 (256 S A 4 bytes do not fit beside the MDP's tables): the same indexing on the buffer itself.
// The blocks of the two learner streams do not depend on the state: the block of the NEXT four ticks is made while the
// current one is used (it also serves sel(s', t + 1) at a block's last tick).
#include "mdpp_internal.hpp"
#include "mdpp_rng.hpp"

namespace mdpp {

constexpr int kLearnRsrcFlags = 0x00020000;
typedef unsigned int learn_u32x2 __attribute__((ext_vector_type(2)));

// what the kernel takes besides the handle's DiscreteArgs
struct LearnArgs {
    float *q;                   // [S A][N] entry-major (device)
    int32_t *carry;             // [N] sarsa: the action carried between the pieces of one call (-1: none)
    int32_t *actions;           // [K][N] the actions taken (out)
    uint64_t seed;              // key of the learner's Philox streams
    uint32_t E;                 // ceil(epsilon 2^31): explore iff (wE >> 1) < E
    float alpha, gamma;
    int32_t algo;               // MDPP_LEARN_*
    int32_t carry_in, carry_out; // this launch is not the first / not the last piece of its call
};

template <bool PHILOX, bool NOISE, bool UNIT, bool QLDS>
__global__ __launch_bounds__(kBlock) void k_discrete_learn_rollout(DiscreteArgs a, LearnArgs p, int K,
                                                                   void *__restrict__ obs,
                                                                   float *__restrict__ reward,
                                                                   uint8_t *__restrict__ term,
                                                                   uint8_t *__restrict__ trunc) {
    const uint64_t ptick0 = tick_now(a);               // the step counter at this launch (through the device-side offset of a graph replay)
    const uint32_t rhead0 = ring_head_now(a, ptick0);  // ... and the head of a delay line kept in memory
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ uint64_t s_ki[NOISE ? 256 : 1];
    __shared__ double s_wi[NOISE ? 256 : 1], s_fi[NOISE ? 256 : 1];
    const int tid = threadIdx.x;
    const uint32_t i = blockIdx.x * kBlock + tid;
    const int S = a.S, A = a.A, L = a.L;
    const uint32_t N = (uint32_t)a.N;
    const uint32_t SA = (uint32_t)S * (uint32_t)A;
    float *const q_lds = (float *)(lds + a.lds_bytes) + tid;
    // stage the shared MDP (and numpy's ziggurat tables, the noise categoricals)
    if (NOISE) zig_stage(s_ki, s_wi, s_fi, tid, kBlock);
    const ZigLds zig{s_ki, s_wi, s_fi};
    for (uint32_t k = tid; k < SA; k += kBlock) lds[a.lds_P + k] = a.P[k];
    for (int k = tid; k < S; k += kBlock) {
        lds[a.lds_term + k] = a.is_term[k];
        ((double *)(lds + a.lds_init))[k] = a.init_cdf[k];
    }
    if (UNIT)
        for (uint32_t k = tid; k < a.rbits_stride; k += kBlock) lds[a.lds_rew + k] = a.rbits[k];
    else
        for (uint32_t k = tid; k < a.nkeys; k += kBlock) ((double *)(lds + a.lds_rew))[k] = a.rtable[k];
    const bool pn_lds = NOISE && a.has_p_noise && a.noise_in_lds;
    if (pn_lds)
        for (int k = tid; k < S * S; k += kBlock) ((double *)(lds + a.lds_noise))[k] = a.noise_cdf[k];
    __syncthreads();
    if (i >= N) return;
    const uint8_t *const tP = lds + a.lds_P, *const tterm = lds + a.lds_term, *const trbits = lds + a.lds_rew;
    const double *const trtable = (const double *)(lds + a.lds_rew), *const tinit = (const double *)(lds + a.lds_init);
    const double *const tnoise = (const double *)(lds + a.lds_noise);

    // this lane's Q-table: entry e at qg[e N] (the buffer) / q_lds[e 256] (its copy for the launch)
    float *const qg = p.q + i;
    if (QLDS)
        for (uint32_t e = 0; e < SA; e++) q_lds[e * kBlock] = qg[(size_t)e * N];
    auto qget = [&](uint32_t e) -> float {
        if constexpr (QLDS) return q_lds[e * kBlock];
        else return qg[(size_t)e * N];
    };
    auto qput = [&](uint32_t e, float v) {
        if constexpr (QLDS) q_lds[e * kBlock] = v;
        else qg[(size_t)e * N] = v;
    };

    const uint4 st = a.state[i];
    // fast_ok handles: word 1 is the queue of start states {24 bits of 4-bit entries, next one lowest; count in bits 24-26},
    // and history bytes 4-7 do not exist (L <= 3: never read)
    const bool queued = a.fast_ok != 0;
    uint64_t hist = ((uint64_t)(queued ? 0xFFFFFFFFu : st.y) << 32) | st.x;      // newest state in byte 0, 0xFF = NaN
    uint32_t qv = st.y & 0x00FFFFFFu, qc = (st.y >> 24) & 7u;
    uint32_t steps = st.z, ringbits = st.w;
    const bool next_step = a.autoreset == MDPP_AUTORESET_NEXT_STEP;
    bool pending = next_step && (steps >> 31) != 0;     // bit 31 of the step counter: the next call is this env's reset
    steps &= 0x7FFFFFFFu;
    uint32_t phase = steps % (uint32_t)a.every_n;       // steps % every_n, kept incrementally below

    const uint64_t genv = (uint64_t)(a.env_id_offset + (int64_t)i);
    Pcg64 env_pcg, sp_pcg;
    PhiloxTickWords pn_w;                               // Philox streams: the current four ticks' noise words / normals
    PhiloxTickNormals rn_z;
    const bool use_env = !PHILOX && ((NOISE && a.has_r_noise) || a.autoreset != 0);   // reward noise, in-rollout resets
    const bool use_sp = !PHILOX && NOISE && a.has_p_noise;
    if (use_env) env_pcg.load(a.env_s, a.env_inc, i);
    if (use_sp) sp_pcg.load(a.sp_s, a.sp_inc, i);

    // the four rewards of the noise-free unit path {paid, not paid} x {terminal, not}, formed once in the reference's float64
    // order (:1987-1990, :2107) and selected per step
    auto unit_reward = [&](bool paid, bool terminal) -> float {
        double r = paid ? 1.0 : 0.0;
        r *= a.scale;
        r += a.shift;
        if (terminal) r += a.term_add;
        return (float)r;
    };
    const float rs0 = unit_reward(false, false), rs1 = unit_reward(false, true), rs2 = unit_reward(true, false), rs3 = unit_reward(true, true);

    const uint32_t total = (uint32_t)K * N;             // (the launcher keeps 8 K N below 2^32)
    const bool obs64 = !a.obs_i32;
    auto r_act = __builtin_amdgcn_make_buffer_rsrc((void *)p.actions, 0, total * 4u, kLearnRsrcFlags);
    auto r_obs = __builtin_amdgcn_make_buffer_rsrc(obs, 0, total * (obs64 ? 8u : 4u), kLearnRsrcFlags);
    auto r_rew = __builtin_amdgcn_make_buffer_rsrc((void *)reward, 0, total * 4u, kLearnRsrcFlags);
    auto r_term = __builtin_amdgcn_make_buffer_rsrc((void *)term, 0, total, kLearnRsrcFlags);
    auto r_trunc = __builtin_amdgcn_make_buffer_rsrc((void *)trunc, 0, total, kLearnRsrcFlags);
    const uint32_t v1 = i, v4 = i * 4u, v8 = i * 8u;
    auto put_obs = [&](uint32_t s, uint32_t so) {       // (the width: wave-uniform)
        if (obs64) __builtin_amdgcn_raw_buffer_store_b64(learn_u32x2{s, 0u}, r_obs, v8, so * 8u, MDPP_ST_NT);
        else __builtin_amdgcn_raw_buffer_store_b32(s, r_obs, v4, so * 4u, MDPP_ST_NT);
    };

    // reset(): the first state of the next episode (:2255: one uniform, searchsorted(cdf, u, 'right'))
    auto start_state = [&](uint64_t ptick) -> uint32_t {
        if (PHILOX)          // one word of the start-state stream per tick (mdpp_rng.hpp)
            return (uint32_t)searchsorted_right(tinit, S, philox_start_uniform(philox_start_m31(a.philox_seed, genv, ptick, kPhiloxStartStream)));
        if (queued && qc != 0) {                        // the next draws of the stream, made ahead by another kernel
            const uint32_t s0 = qv & 0xFu;
            qv >>= 4; qc -= 1;
            return s0;
        }
        return (uint32_t)searchsorted_right(tinit, S, np_random(env_pcg));
    };
    auto episode_start = [&](uint32_t s0) {
        hist = 0xFFFFFFFFFFFFFF00ULL | (uint64_t)s0;
        steps = 0; phase = 0; ringbits = 0;
        if (!UNIT)
            for (int d = 0; d < a.delay; d++) a.ring_keys[(size_t)d * N + i] = kNoKey;
    };

    // the learner's words: the blocks of ticks 4 b .. 4 b + 3 in *_cur, the next ones made ahead in *_nxt
    uint32_t e_cur[4], e_nxt[4], x_cur[4], x_nxt[4];
    philox_start_block(p.seed, genv, ptick0 >> 2, kPhiloxLearnExploreStream, e_nxt);
    philox_start_block(p.seed, genv, ptick0 >> 2, kPhiloxLearnActionStream, x_nxt);
    uint64_t blk_cur = 0;

    // max_j Q[s][j] and the lowest j that attains it
    auto row_best = [&](uint32_t s, uint32_t &arg) -> float {
        const uint32_t e0 = s * (uint32_t)A;
        float best = qget(e0);
        uint32_t bj = 0;
        for (uint32_t j = 1; j < (uint32_t)A; j++) {
            const float v = qget(e0 + j);
            if (v > best) { best = v; bj = j; }
        }
        arg = bj;
        return best;
    };
    // sel(s, tick), tick in the current block or the first of the next
    auto select = [&](uint32_t s, uint64_t tick) -> uint32_t {
        const bool in_cur = (tick >> 2) == blk_cur;     // (wave-uniform)
        const uint32_t wE = in_cur ? philox_word_of(e_cur, tick) : philox_word_of(e_nxt, tick);
        if ((wE >> 1) < p.E) {
            const uint32_t wA = in_cur ? philox_word_of(x_cur, tick) : philox_word_of(x_nxt, tick);
            return (uint32_t)(((uint64_t)wA * (uint64_t)(uint32_t)A) >> 32);
        }
        uint32_t j;
        (void)row_best(s, j);
        return j;
    };

    const bool sarsa = p.algo == MDPP_LEARN_SARSA;
    bool have_carry = false;
    uint32_t carried = 0;
    if (p.carry_in) {
        const int32_t c = p.carry[i];
        have_carry = c >= 0;
        carried = have_carry ? (uint32_t)c : 0u;
    }

    for (int k = 0; k < K; k++) {
        const uint64_t ptick = ptick0 + (uint64_t)k;
        const uint32_t so = (uint32_t)k * N;
        if (k == 0 || (ptick & 3u) == 0u) {             // (wave-uniform)
#pragma unroll
            for (int q = 0; q < 4; q++) { e_cur[q] = e_nxt[q]; x_cur[q] = x_nxt[q]; }
            blk_cur = ptick >> 2;
            philox_start_block(p.seed, genv, blk_cur + 1u, kPhiloxLearnExploreStream, e_nxt);
            philox_start_block(p.seed, genv, blk_cur + 1u, kPhiloxLearnActionStream, x_nxt);
        }
        const uint32_t cur = (uint32_t)hist & 0xFFu;
        const uint32_t action = have_carry ? carried : select(cur, ptick);
        have_carry = false;
        __builtin_amdgcn_raw_buffer_store_b32(action, r_act, v4, so * 4u, MDPP_ST_NT);
        if (pending) {               // next-step autoreset: this call is the env's reset(), :2250-2278; the action is ignored, nothing is learnt
            const uint32_t s0 = start_state(ptick);
            episode_start(s0);
            put_obs(s0, so);
            __builtin_amdgcn_raw_buffer_store_b32(0u, r_rew, v4, so * 4u, MDPP_ST_NT);
            __builtin_amdgcn_raw_buffer_store_b8((uint8_t)0, r_term, v1, so, MDPP_ST_NT);
            __builtin_amdgcn_raw_buffer_store_b8((uint8_t)0, r_trunc, v1, so, MDPP_ST_NT);
            pending = false;
            continue;
        }
        uint32_t nxt = tP[cur * (uint32_t)A + action];                              // D1
        if (NOISE && a.has_p_noise) {                                               // D2
            // (Philox streams: one word of the tick decides "noisy" and which other state; numpy streams: the state space's own
            //  generator and the categorical's cdf, as in the reference)
            if (PHILOX) nxt = philox_pnoise_state(pn_w.word(a.philox_seed, genv, ptick, kPhiloxPNoiseStream), a.pn_T, a.pn_M, nxt);
            else if (pn_lds) nxt = (uint32_t)searchsorted_right(tnoise + (size_t)nxt * S, S, np_random(sp_pcg));
            else nxt = (uint32_t)searchsorted_right(a.noise_cdf + (size_t)nxt * S, S, np_random(sp_pcg));
        }
        hist = (hist << 8) | nxt;                                                   // D3
        steps += 1;
        phase = (phase + 1 == (uint32_t)a.every_n) ? 0u : phase + 1;
        uint32_t key = kNoKey;                                                      // D4 (NaN gate: L transitions since reset, :1822)
        if (((hist >> (8 * L)) & 0xFFu) != 0xFFu) {
            key = 0;
            for (int j = L - 1; j >= 0; j--) key = key * (uint32_t)S + (uint32_t)((hist >> (8 * j)) & 0xFFu);
        }
        // custom reward matrix: R(s, a) of this transition, whatever s' (noise included) was (:1259-1267)
        if (!UNIT && a.rew_sa) key = cur * (uint32_t)A + action;
        const bool done = tterm[nxt] != 0;                                          // D7
        float rout;
        if (UNIT) {
            uint32_t bit = 0;
            if (key != kNoKey) bit = (trbits[key >> 3] >> (key & 7u)) & 1u;
            if (a.delay > 0) {                                                      // D5 (shift register)
                const uint32_t out = (ringbits >> (a.delay - 1)) & 1u;
                ringbits = (ringbits << 1) | bit;
                bit = out;
            }
            if (phase != 0) bit = 0;                                                // D6
            if (NOISE && a.has_r_noise) {
                double r = bit ? 1.0 : 0.0;
                const double nz = 0.0 + a.r_noise * (PHILOX ? (double)rn_z.normal(a.philox_seed, genv, ptick, kPhiloxRNoiseStream) : np_standard_normal_lds(env_pcg, zig));
                r += nz;
                r *= a.scale;
                r += a.shift;
                if (done) r += a.term_add;
                rout = (float)r;
            } else {
                rout = done ? (bit ? rs3 : rs1) : (bit ? rs2 : rs0);
            }
        } else {
            if (a.delay > 0) {                                                      // D5 (key ring)
                uint32_t *slot = a.ring_keys + (size_t)((rhead0 + (uint32_t)k) % (uint32_t)a.delay) * N + i;
                const uint32_t out = *slot;
                *slot = key;
                key = out;
            }
            double r = (key != kNoKey) ? trtable[key] : 0.0;
            if (phase != 0) r = 0.0;                                                // D6
            if (NOISE && a.has_r_noise) {
                const double nz = 0.0 + a.r_noise * (PHILOX ? (double)rn_z.normal(a.philox_seed, genv, ptick, kPhiloxRNoiseStream) : np_standard_normal_lds(env_pcg, zig));
                r += nz;
            }
            r *= a.scale;
            r += a.shift;
            if (done) r += a.term_add;
            rout = (float)r;
        }
        const bool truncated = (a.max_steps > 0) && (steps >= (uint32_t)a.max_steps);

        // the learner: target from the true next state, on Q as it is before this step's update
        float y = rout;
        uint32_t a2 = 0;
        if (!done) {
            float qn;
            if (sarsa) {                                                            // (wave-uniform)
                a2 = select(nxt, ptick + 1u);
                qn = qget(nxt * (uint32_t)A + a2);
            } else {
                qn = row_best(nxt, a2);
            }
            const float g = p.gamma * qn;
            y = rout + g;
        }
        {
            const uint32_t e = cur * (uint32_t)A + action;
            const float q = qget(e);
            const float d = y - q;
            const float u = p.alpha * d;
            qput(e, q + u);
        }
        // sarsa: the next step of this call takes a' when it starts from s'
        have_carry = sarsa && !done && !(truncated && a.autoreset != MDPP_AUTORESET_DISABLED);
        carried = a2;

        uint32_t out_state = nxt;
        if (next_step) pending = done || truncated;
        if (a.autoreset == MDPP_AUTORESET_SAME_STEP && (done || truncated)) {
            // same-step autoreset: the terminal transition's reward and flags, the first observation of the next episode
            out_state = start_state(ptick);
            episode_start(out_state);
        }
        put_obs(out_state, so);
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(rout), r_rew, v4, so * 4u, MDPP_ST_NT);
        __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(done ? 1 : 0), r_term, v1, so, MDPP_ST_NT);
        __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(truncated ? 1 : 0), r_trunc, v1, so, MDPP_ST_NT);
    }

    if (QLDS)
        for (uint32_t e = 0; e < SA; e++) qg[(size_t)e * N] = q_lds[e * kBlock];
    if (p.carry_out) p.carry[i] = have_carry ? (int32_t)carried : -1;
    a.state[i] = make_uint4((uint32_t)hist, queued ? (qv | (qc << 24)) : (uint32_t)(hist >> 32),
                            steps | (pending ? 0x80000000u : 0u), ringbits);
    if (use_env) env_pcg.store(a.env_s, i);
    if (use_sp) sp_pcg.store(a.sp_s, i);
}

// Q between the caller's [N][S A] and the handle's [S A][N]
template <bool TO_HANDLE>
__global__ __launch_bounds__(kBlock) void k_learn_q_transpose(float *__restrict__ handle_q, float *__restrict__ user_q, uint32_t N, uint32_t SA) {
    const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (uint64_t)N * SA) return;
    const uint32_t e = (uint32_t)(t / N), i = (uint32_t)(t - (uint64_t)e * N);
    if (TO_HANDLE) handle_q[t] = user_q[(size_t)i * SA + e];
    else user_q[(size_t)i * SA + e] = handle_q[t];
}

int launch_learn_q_copy(mdpp_env *h, float *user_q, bool to_handle, hipStream_t s) {
    const uint32_t N = (uint32_t)h->cfg.num_envs, SA = (uint32_t)h->cfg.S * (uint32_t)h->cfg.A;
    const uint64_t total = (uint64_t)N * SA;
    const uint64_t grid = (total + kBlock - 1) / kBlock;
    if (grid > 0x7FFFFFFFull) { h->err = "k_learn_q_transpose: table too large"; return MDPP_EUNSUPPORTED; }
    if (to_handle) hipLaunchKernelGGL(k_learn_q_transpose<true>, dim3((uint32_t)grid), dim3(kBlock), 0, s, (float *)h->d_learn_q, user_q, N, SA);
    else hipLaunchKernelGGL(k_learn_q_transpose<false>, dim3((uint32_t)grid), dim3(kBlock), 0, s, (float *)h->d_learn_q, user_q, N, SA);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { h->err = std::string("k_learn_q_transpose launch: ") + hipGetErrorString(e); return MDPP_EHIP; }
    return MDPP_OK;
}

constexpr size_t kZigLdsBytes = 3u * 256u * 8u;        // the kernel's static LDS with a noise key

// Why this handle has no learner, or null: the kernel serves it
const char *discrete_learn_refusal(const mdpp_env *h) {
    const mdpp_config &c = h->cfg;
    const DiscreteArgs &a = h->dargs;
    if (c.kind != MDPP_KIND_DISCRETE) return "learner rollouts serve discrete envs only (this handle is continuous or a grid)";
    if (c.image) return "learner rollouts do not serve image observations";
    if (c.irrelevant) return "learner rollouts do not serve an irrelevant sub-space (irrelevant_features)";
    if (c.num_tables != 1) return "learner rollouts need one shared MDP (this handle has one MDP per env: seeds=[...])";
    if (c.S > 255) return "learner rollouts need at most 255 states (state_space_size)";
    if (c.L > 7) return "learner rollouts need sequence_length <= 7";
    if (c.episode_stats) return "learner rollouts do not keep episode_stats";
    const bool noise = c.has_transition_noise || c.has_reward_noise;
    if (!a.rew_in_lds || (size_t)a.lds_bytes + (noise ? kZigLdsBytes : 0u) > 64u * 1024u)
        return "learner rollouts need the MDP's tables within 64 KiB of LDS";
    return nullptr;
}

// K learning steps.  name_out != nullptr: a dry run, the kernel's name only
int launch_discrete_learn(mdpp_env *h, int K, int32_t *actions_out, void *obs, float *reward, uint8_t *term, uint8_t *trunc,
                          hipStream_t s, char *name_out) {
    if (const char *why = discrete_learn_refusal(h)) { h->err = std::string("mdpp_step_n_learn: ") + why; return MDPP_EUNSUPPORTED; }
    DiscreteArgs a = h->dargs;
    stamp_step(a, h);
    const int grid = (a.N + kBlock - 1) / kBlock;
    const size_t q_lds = (size_t)kBlock * (size_t)a.S * (size_t)a.A * sizeof(float);
    // pieces: the buffer descriptors address < 4 GiB per output array (8 bytes per env-step at most)
    long long kmax = ((1LL << 32) - 1) / (8LL * a.N);
    if (kmax < 1) { h->err = "k_discrete_learn_rollout: num_envs too large"; return MDPP_EUNSUPPORTED; }
    if ((a.opts & MDPP_OPT_LEARN_SHORT_PIECES) && kmax > 5) kmax = 5;      // (tests: the pieces' hand-over at a small size)
    const size_t ob = a.obs_i32 ? 4 : 8;
    int rc = MDPP_OK;
    with_bools([&](auto PH, auto NZ, auto UNIT) {
        // the LDS form when a workgroup's 256 tables fit beside the MDP's (and the device grants it)
        const bool qlds = !(a.opts & MDPP_OPT_NO_LEARN_LDS) && q_lds <= 160u * 1024u &&
                          dynamic_lds_ok((const void *)k_discrete_learn_rollout<PH(), NZ(), UNIT(), true>, (size_t)a.lds_bytes + q_lds);
        with_bools([&](auto QL) {
            auto kern = k_discrete_learn_rollout<PH(), NZ(), UNIT(), QL()>;
            if (name_out) {
                snprintf(name_out, kNameLen, "k_discrete_learn_rollout<PHILOX=%d,NOISE=%d,UNIT=%d,QLDS=%d>", PH(), NZ(), UNIT(), QL());
                return;
            }
            const size_t lds = (size_t)a.lds_bytes + (QL() ? q_lds : 0u);
            if (!QL() && !dynamic_lds_ok((const void *)kern, lds)) {
                h->err = "k_discrete_learn_rollout: the device refuses the launch's LDS";
                rc = MDPP_EUNSUPPORTED;
                return;
            }
            for (int k0 = 0; k0 < K;) {
                const int kc = (int)((K - k0) < kmax ? (K - k0) : kmax);
                const size_t off = (size_t)k0 * (size_t)a.N;
                stamp_piece(a, h, k0);
                const LearnArgs p{(float *)h->d_learn_q, (int32_t *)h->d_learn_carry, actions_out + off, h->learn_seed, h->learn_E,
                                  h->learn_alpha, h->learn_gamma, h->learn_algo, k0 > 0 ? 1 : 0, k0 + kc < K ? 1 : 0};
                hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), lds, s, a, p, kc, (void *)((char *)obs + off * ob), reward + off,
                                   term + off, trunc + off);
                k0 += kc;
            }
        }, qlds);
    }, a.philox != 0, a.has_p_noise || a.has_r_noise, a.unit_rewards != 0);
    if (rc != MDPP_OK || name_out) return rc;
    return step_done(h, K, "k_discrete_learn_rollout");
}

} // namespace mdpp
