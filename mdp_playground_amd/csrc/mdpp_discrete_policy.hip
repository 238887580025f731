// Closed-loop fused rollout of a discrete env under a tabular policy: the launch that does s -> s' also samples
// a ~ pi(. | s), so K steps of an agent that acts on what it observes are ONE launch (mdpp_step_n_policy).
//
// The policy is a table of thresholds T uint32 [S][A] (non-decreasing rows; T[s][j] = ceil(cdf_s[j] 2^31)) and a 64-bit
// seed.  Env g = env_id_offset + i at step counter t draws
//   w = word (t & 3) of block 0 of the Philox4x32-10 stream (policy seed, g, t >> 2, kPhiloxPolicyStream)   [mdpp_rng.hpp philox_start_block]
//   a = min(#{ j < A : T[s][j] <= (w >> 1) }, A - 1),      s = the state the env is in (the last observation returned for it)
// -- the rule of philox_start_m31 for start states: searchsorted(cdf_s, (w >> 1) 2^-31, 'right').  The policy reads no stream of
// the env, so the launch leaves every stream of the handle where mdpp_step_n fed with the same actions leaves it.
//
// The step itself restates k_discrete_step (mdpp_discrete.hip) without its NOISE and IRR branches, on the same lines of
// the reference's mdp_playground/envs/rl_toy_env.py:
//   D1 P lookup            :1602-1603      D5 delay FIFO        :1968-1973
//   D3 history shift       :2050-2058      D6 every-n / affine  :1975-1990
//   D4 sequence reward     :1821-1845      D7 terminal + reward :2102-2109      R1 reset :2250-2278, :2354-2369
//
// One lane per env, 256-thread workgroups, the general 16-byte record {hist bytes 0-3, hist bytes 4-7, steps, ring bits}.
// fast_ok handles (mdpp_discrete_fast.hip) keep their queue of start states drawn ahead in word 1 of the record instead of
// history bytes 4-7 (they have L <= 3): a reset here pops the queue first, in order, and draws from the env stream only when
// it is empty, as k_discrete_reset does -- so any kernel of the handle can follow this one and the other way round.
// The shared MDP's tables are staged in LDS in the handle's own carve (DiscreteArgs::lds_*), the thresholds behind them; a
// row of at most 8 actions is padded to 8 entries (0xFFFFFFFF: never <= a 31-bit draw), read as two 16-byte LDS reads and
// counted without a branch; longer rows are searched (the same count on a non-decreasing row).  The policy's words do
// not depend on the state: the block of the NEXT four ticks is made while the current one is used, so the chain a step
// waits for is  threshold row of s -> count -> P[s][a].
#include "mdpp_internal.hpp"
#include "mdpp_rng.hpp"

namespace mdpp {

constexpr int kPolicyRsrcFlags = 0x00020000;
typedef unsigned int pol_u32x2 __attribute__((ext_vector_type(2)));

// what the kernel takes besides the handle's DiscreteArgs
struct PolicyArgs {
    const uint32_t *thr;        // [S][A] thresholds (device)
    uint64_t seed;              // policy seed: key of the policy's Philox stream
    int32_t *actions;           // [K][N] the sampled actions (out)
};

// uint32 per threshold row in LDS
__host__ __device__ inline uint32_t policy_row_words(int A) { return A <= 8 ? 8u : (uint32_t)A; }

template <bool PHILOX, bool UNIT, bool OBS64, bool A8>
__global__ __launch_bounds__(kBlock) void k_discrete_policy_rollout(DiscreteArgs a, PolicyArgs p, int K,
                                                                    void *__restrict__ obs,
                                                                    float *__restrict__ reward,
                                                                    uint8_t *__restrict__ term,
                                                                    uint8_t *__restrict__ trunc) {
    const uint64_t ptick0 = tick_now(a);               // the step counter at this launch (through the device-side offset of a graph replay)
    const uint32_t rhead0 = ring_head_now(a, ptick0);  // ... and the head of a delay line kept in memory
    extern __shared__ __align__(16) unsigned char lds[];
    const int tid = threadIdx.x;
    const uint32_t i = blockIdx.x * kBlock + tid;
    const int S = a.S, A = a.A, L = a.L;
    const uint32_t N = (uint32_t)a.N;
    const uint32_t W = A8 ? 8u : (uint32_t)A;
    uint32_t *const lds_thr = (uint32_t *)(lds + a.lds_bytes);
    // stage the shared MDP and the policy
    for (int k = tid; k < S * A; k += kBlock) lds[a.lds_P + k] = a.P[k];
    for (int k = tid; k < S; k += kBlock) {
        lds[a.lds_term + k] = a.is_term[k];
        ((double *)(lds + a.lds_init))[k] = a.init_cdf[k];
    }
    if (UNIT)
        for (uint32_t k = tid; k < a.rbits_stride; k += kBlock) lds[a.lds_rew + k] = a.rbits[k];
    else
        for (uint32_t k = tid; k < a.nkeys; k += kBlock) ((double *)(lds + a.lds_rew))[k] = a.rtable[k];
    for (uint32_t k = tid; k < (uint32_t)S * W; k += kBlock) {
        const uint32_t s = k / W, j = k - s * W;
        lds_thr[k] = j < (uint32_t)A ? p.thr[s * (uint32_t)A + j] : 0xFFFFFFFFu;
    }
    __syncthreads();
    if (i >= N) return;
    const uint8_t *const tP = lds + a.lds_P, *const tterm = lds + a.lds_term, *const trbits = lds + a.lds_rew;
    const double *const trtable = (const double *)(lds + a.lds_rew), *const tinit = (const double *)(lds + a.lds_init);

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
    Pcg64 env_pcg;
    const bool use_env = !PHILOX && a.autoreset != 0;   // the env stream: in-rollout resets only
    if (use_env) env_pcg.load(a.env_s, a.env_inc, i);

    // the four rewards of the unit path {paid, not paid} x {terminal, not}, formed once in the reference's float64 order
    // (:1987-1990, :2107) and selected per step
    auto unit_reward = [&](bool paid, bool terminal) -> float {
        double r = paid ? 1.0 : 0.0;
        r *= a.scale;
        r += a.shift;
        if (terminal) r += a.term_add;
        return (float)r;
    };
    const float rs0 = unit_reward(false, false), rs1 = unit_reward(false, true), rs2 = unit_reward(true, false), rs3 = unit_reward(true, true);

    const uint32_t total = (uint32_t)K * N;             // (the launcher keeps 8 K N below 2^32)
    auto r_act = __builtin_amdgcn_make_buffer_rsrc((void *)p.actions, 0, total * 4u, kPolicyRsrcFlags);
    auto r_obs = __builtin_amdgcn_make_buffer_rsrc(obs, 0, total * (OBS64 ? 8u : 4u), kPolicyRsrcFlags);
    auto r_rew = __builtin_amdgcn_make_buffer_rsrc((void *)reward, 0, total * 4u, kPolicyRsrcFlags);
    auto r_term = __builtin_amdgcn_make_buffer_rsrc((void *)term, 0, total, kPolicyRsrcFlags);
    auto r_trunc = __builtin_amdgcn_make_buffer_rsrc((void *)trunc, 0, total, kPolicyRsrcFlags);
    const uint32_t v1 = i, v4 = i * 4u, v8 = i * 8u;
    auto put_obs = [&](uint32_t s, uint32_t so) {
        if (OBS64) __builtin_amdgcn_raw_buffer_store_b64(pol_u32x2{s, 0u}, r_obs, v8, so * 8u, MDPP_ST_NT);
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

    // the policy's words: the block of ticks 4 b .. 4 b + 3 in w_cur, the next one made ahead in w_nxt
    uint32_t w_cur[4], w_nxt[4];
    philox_start_block(p.seed, genv, ptick0 >> 2, kPhiloxPolicyStream, w_nxt);

    for (int k = 0; k < K; k++) {
        const uint64_t ptick = ptick0 + (uint64_t)k;
        const uint32_t so = (uint32_t)k * N;
        if (k == 0 || (ptick & 3u) == 0u) {             // (wave-uniform)
#pragma unroll
            for (int q = 0; q < 4; q++) w_cur[q] = w_nxt[q];
            philox_start_block(p.seed, genv, (ptick >> 2) + 1u, kPhiloxPolicyStream, w_nxt);
        }
        const uint32_t m = philox_word_of(w_cur, ptick) >> 1;
        const uint32_t cur = (uint32_t)hist & 0xFFu;
        // a = min(#{ j : T[cur][j] <= m }, A - 1)
        uint32_t cnt = 0;
        if (A8) {
            const uint4 t0 = ((const uint4 *)lds_thr)[2u * cur], t1 = ((const uint4 *)lds_thr)[2u * cur + 1u];
            cnt = (t0.x <= m) + (t0.y <= m) + (t0.z <= m) + (t0.w <= m) + (t1.x <= m) + (t1.y <= m) + (t1.z <= m) + (t1.w <= m);
        } else {
            const uint32_t *row = lds_thr + cur * W;
            for (uint32_t n = (uint32_t)A; n > 0;) {    // first j with T[j] > m on a non-decreasing row
                const uint32_t half = n >> 1;
                const bool le = row[cnt + half] <= m;
                cnt = le ? cnt + half + 1u : cnt;
                n = le ? n - half - 1u : half;
            }
        }
        const uint32_t action = cnt < (uint32_t)A - 1u ? cnt : (uint32_t)A - 1u;
        __builtin_amdgcn_raw_buffer_store_b32(action, r_act, v4, so * 4u, MDPP_ST_NT);
        if (pending) {               // next-step autoreset: this call is the env's reset(), :2250-2278; the action is ignored
            const uint32_t s0 = start_state(ptick);
            episode_start(s0);
            put_obs(s0, so);
            __builtin_amdgcn_raw_buffer_store_b32(0u, r_rew, v4, so * 4u, MDPP_ST_NT);
            __builtin_amdgcn_raw_buffer_store_b8((uint8_t)0, r_term, v1, so, MDPP_ST_NT);
            __builtin_amdgcn_raw_buffer_store_b8((uint8_t)0, r_trunc, v1, so, MDPP_ST_NT);
            pending = false;
            continue;
        }
        const uint32_t nxt = tP[cur * (uint32_t)A + action];                        // D1
        hist = (hist << 8) | nxt;                                                   // D3
        steps += 1;
        phase = (phase + 1 == (uint32_t)a.every_n) ? 0u : phase + 1;
        uint32_t key = kNoKey;                                                      // D4 (NaN gate: L transitions since reset, :1822)
        if (((hist >> (8 * L)) & 0xFFu) != 0xFFu) {
            key = 0;
            for (int j = L - 1; j >= 0; j--) key = key * (uint32_t)S + (uint32_t)((hist >> (8 * j)) & 0xFFu);
        }
        // custom reward matrix: R(s, a) of this transition (:1259-1267)
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
            rout = done ? (bit ? rs3 : rs1) : (bit ? rs2 : rs0);
        } else {
            if (a.delay > 0) {                                                      // D5 (key ring)
                uint32_t *slot = a.ring_keys + (size_t)((rhead0 + (uint32_t)k) % (uint32_t)a.delay) * N + i;
                const uint32_t out = *slot;
                *slot = key;
                key = out;
            }
            double r = (key != kNoKey) ? trtable[key] : 0.0;
            if (phase != 0) r = 0.0;                                                // D6
            r *= a.scale;
            r += a.shift;
            if (done) r += a.term_add;
            rout = (float)r;
        }
        const bool truncated = (a.max_steps > 0) && (steps >= (uint32_t)a.max_steps);
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

    a.state[i] = make_uint4((uint32_t)hist, queued ? (qv | (qc << 24)) : (uint32_t)(hist >> 32),
                            steps | (pending ? 0x80000000u : 0u), ringbits);
    if (use_env) env_pcg.store(a.env_s, i);
}

// Why this handle has no closed-loop launch, or null: the kernel serves it
const char *discrete_policy_refusal(const mdpp_env *h) {
    const mdpp_config &c = h->cfg;
    const DiscreteArgs &a = h->dargs;
    if (c.kind != MDPP_KIND_DISCRETE) return "policy rollouts serve discrete envs only (this handle is continuous or a grid)";
    if (c.image) return "policy rollouts do not serve image observations";
    if (c.irrelevant) return "policy rollouts do not serve an irrelevant sub-space (irrelevant_features)";
    if (c.num_tables != 1) return "policy rollouts need one shared MDP (this handle has one MDP per env: seeds=[...])";
    if (c.S > 255) return "policy rollouts need at most 255 states (state_space_size)";
    if (c.L > 7) return "policy rollouts need sequence_length <= 7";
    if (c.has_transition_noise) return "policy rollouts do not serve a transition_noise key";
    if (c.has_reward_noise) return "policy rollouts do not serve a reward_noise key";
    if (c.episode_stats) return "policy rollouts do not keep episode_stats";
    const uint64_t lds = (uint64_t)a.lds_bytes + 4ull * (uint64_t)c.S * policy_row_words(c.A);
    if (!a.rew_in_lds || lds > 64u * 1024u) return "policy rollouts need the MDP's tables and the thresholds within 64 KiB of LDS";
    return nullptr;
}

// K closed-loop steps from the handle's policy.  name_out != nullptr: a dry run, the kernel's name only
int launch_discrete_policy(mdpp_env *h, int K, int32_t *actions_out, void *obs, float *reward, uint8_t *term, uint8_t *trunc,
                           hipStream_t s, char *name_out) {
    if (const char *why = discrete_policy_refusal(h)) { h->err = std::string("mdpp_step_n_policy: ") + why; return MDPP_EUNSUPPORTED; }
    DiscreteArgs a = h->dargs;
    stamp_step(a, h);
    const int grid = (a.N + kBlock - 1) / kBlock;
    const size_t lds = (size_t)a.lds_bytes + 4u * (size_t)a.S * policy_row_words(a.A);
    // pieces: the buffer descriptors address < 4 GiB per output array (8 bytes per env-step at most)
    const long long kmax = ((1LL << 32) - 1) / (8LL * a.N);
    if (kmax < 1) { h->err = "k_discrete_policy_rollout: num_envs too large"; return MDPP_EUNSUPPORTED; }
    const size_t ob = a.obs_i32 ? 4 : 8;
    int rc = MDPP_OK;
    with_bools([&](auto PH, auto UNIT, auto O64, auto A8) {
        auto kern = k_discrete_policy_rollout<PH(), UNIT(), O64(), A8()>;
        if (name_out) {
            snprintf(name_out, kNameLen, "k_discrete_policy_rollout<PHILOX=%d,UNIT=%d,OBS64=%d,A8=%d>", PH(), UNIT(), O64(), A8());
            return;
        }
        if (!dynamic_lds_ok((const void *)kern, lds)) {
            h->err = "k_discrete_policy_rollout: the device refuses the launch's LDS";
            rc = MDPP_EUNSUPPORTED;
            return;
        }
        for (int k0 = 0; k0 < K;) {
            const int kc = (int)((K - k0) < kmax ? (K - k0) : kmax);
            const size_t off = (size_t)k0 * (size_t)a.N;
            stamp_piece(a, h, k0);
            const PolicyArgs p{(const uint32_t *)h->d_policy_thr, h->policy_seed, actions_out + off};
            hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), lds, s, a, p, kc, (void *)((char *)obs + off * ob), reward + off,
                               term + off, trunc + off);
            k0 += kc;
        }
    }, a.philox != 0, a.unit_rewards != 0, !a.obs_i32, a.A <= 8);
    if (rc != MDPP_OK || name_out) return rc;
    return step_done(h, K, "k_discrete_policy_rollout");
}

} // namespace mdpp
