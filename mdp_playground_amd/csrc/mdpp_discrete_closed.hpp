// The closed-loop step of a discrete env, stated once: K steps of "an agent picks a from the state the env is in, the env
// steps, the agent sees the transition" in ONE launch.  k_discrete_policy_rollout (mdpp_discrete_policy.hip), the learners'
// kernels (mdpp_discrete_learn.hpp) and the greedy evaluation's (mdpp_discrete_eval.hpp) are this body, closed_loop_rollout,
// around their own Agent; so is the launcher (launch_closed_loop) and the rule for which handles are served.
//
// What the learners and the evaluation share on the host -- both keep per-env Q-tables -- is here too, each stated once:
//   closed_agent_lds       the placement: which of the Q-tables, the envs' MDP slots and the per-level cdfs go to LDS
//   launch_closed_form     the launcher of one form: the step's compile-time facts, the placement, the kernel, its name, its LDS
// A header of theirs holds the agent, the two __global__ kernels (the ziggurat LDS, where the agent's LDS starts, the agent,
// the step), a form type for launch_closed_form and the entry templates its translation units instantiate.  The kernels'
// bodies and the agents' table access are written out in each header: a shared body function, a shared table struct and a
// shared "where the agent's LDS starts" each changed the instructions of kernels that exist.
//
// The step restates k_discrete_step (mdpp_discrete.hip) without its IRR branches and episode statistics, on the same lines
// of the reference's mdp_playground/envs/rl_toy_env.py:
//   D1 P lookup            :1602-1603      D5 delay FIFO        :1968-1973
//   D2 transition noise    :1605-1625      D6 every-n / affine  :1975-1990
//   D3 history shift       :2050-2058      D7 terminal + reward :2102-2109
//   D4 sequence reward     :1821-1845      R1 reset             :2250-2278, :2354-2369
// NOISE = true adds D2 (the categorical's cdf / philox_pnoise_state) and the reward noise (numpy's ziggurat with the tables
// in LDS / PhiloxTickNormals).  The agent reads no stream of the env, so the launch leaves every stream, the state record
// and the step counter where mdpp_step_n fed with the same actions leaves them.
//
// One lane per env, 256-thread workgroups, the general 16-byte record {hist bytes 0-3, hist bytes 4-7, steps, ring bits}.
// fast_ok handles (mdpp_discrete_fast.hip) keep their queue of start states drawn ahead in word 1 of the record instead of
// history bytes 4-7 (they have L <= 3): a reset here pops the queue first, in order, and draws from the env stream only when
// it is empty, as k_discrete_reset does -- so any kernel of the handle can follow this one and the other way round.
// The shared MDP's tables are staged in LDS in the handle's own carve (DiscreteArgs::lds_*); what the agent stages goes
// behind them (from lds + a.lds_bytes).  Outputs leave through range-checked non-temporal buffer stores.
//
// An Agent is a struct of force-inlined members (no virtual calls, no function pointers):
//   stage(tid)                 cooperative LDS staging, before the barrier
//   begin(i, genv, ptick0)     per lane, after the `i >= N` return
//   next_block(genv, ptick)    at a launch's first step and at every tick that starts a Philox block (wave-uniform)
//   act(cur, ptick)            the action of this step; also called on a reset call, from the state in the record
//   learn(cur, action, nxt, reward, done, truncated_with_reset, ptick)
//                              after the reward is formed, before a same-step reset: nxt is the true next state
//   episode_end(ended)         after every step that is not a reset call, where the summary rule below is applied: ended =
//                              terminated or truncated (empty but for the scheduled learner, mdpp_discrete_learn.hpp SCHED)
//   finish(i)                  per lane, after the last step
//
// SUMMARY = true (mdpp_step_n_learn_summary / mdpp_step_n_eval_summary): the same K steps with no [K][N] output.  The lane
// loads the five values of its env from sm after begin(), applies at every step that is not a reset call
//   ret += (double)reward;  len += 1;  terminated or truncated: episodes += 1, return_sum += ret, length_sum += len, ret = len = 0
// and stores them after finish().  The five output pointers are unused (null).  A compile-time choice: the SUMMARY = false
// instantiations are the code they were.
// An episode log (sm.log_cap = M != 0, a run-time field: no kernel is added or renamed for it): the lane loads count[i] with
// its five values and, where the rule finds terminated or truncated, before ret and len are zeroed,
//   count < M: log_ret[count][i] = ret, log_len[count][i] = len;  count += 1
// -- the values just added to return_sum / length_sum; the element index count N + i is kept in 64 bits and moved on by N per
// episode (the host keeps M N below 2^31); the stores are non-temporal, like the [K][N] outputs' (MDPP_ST_NT) -- and stores
// count[i] with the five.  No atomics: env i's column is this lane's alone.  Rows the launch does not reach are not touched.
// LOG = true is the body of the learner's k_discrete_learn_summary_log kernels (mdpp_discrete_learn.hpp), which the launcher
// takes when sm.log_cap != 0; the summary kernels themselves are LOG = false, the code they were.  (As a run-time branch in the
// summary kernels' step loop the log cost the launches WITHOUT one 3-6 %, executed or not: the loops are latency-bound and any
// addition moved their schedule.  Two copies of the loop inside one kernel still shared its register allocation.)
//
// NLEV = true (per-env noise levels, mdpp_set_noise_levels; with NOISE only): env i has its own reward-noise sigma and its own
// transition-noise level.  After the `i >= N` return the lane loads its level byte, its sigma and its level's Philox
// threshold T -- T == 0 is the level "no transition noise" -- and keeps them in registers.  The reward-noise term is
// 0.0 + sigma z with the draw every lane makes.  D2: Philox streams take the lane's (T, M) -- the pair is loaded once, the
// level never changes inside a launch; numpy streams search the lane's own [S][S] block of the per-level cdfs and draw from
// the space stream only where T != 0 (the reference's `if self.transition_noise:`, lane by lane).  The per-level cdfs are
// staged in LDS behind the MDP's tables (from lds + a.lds_bytes, nl.lds_bytes of them; the agent's LDS moves behind) when
// the host found room, else read in global memory.  The handle's own cdf (a.noise_cdf / a.lds_noise) is not staged.
// A compile-time choice like SUMMARY: the NLEV = false instantiations are the code they were.
//
// PM (one MDP per env, mdpp_learner_per_env_mdp): 0 is the shared MDP above.  PM = 1: lane i reads table
// set i of a.P / is_term / init_cdf / rbits / rtable in global memory, with k_discrete_step's strides.  PM = 2: the lane stages
// its own set once per launch into LDS, laid out as the learners lay out Q: dword w of lane tid at byte (w 256 + tid) 4, w
// counted in the handle's own carve (a.lds_P / 4 ..., a.lds_noise / 4 dwords per lane).  Bank = lane: no conflict whatever
// (s, a) each lane holds -- a per-lane slot of the carve's own stride (216 B at 8 x 8: 54 dwords, 54 l mod 32 reaches 16
// banks) would make every dependent read 2-way conflicted.  P, the terminal flags and the reward bits are bytes taken out of
// their dword, a cdf entry or a reward two dwords.  Tail lanes of the last workgroup stage table set N - 1.  The transition
// noise's cdf and the ziggurat tables stay shared: the cdf lies behind the slots (PM = 2) or at the start of LDS (PM = 1),
// the agent's LDS behind it (closed_agent_lds_offset).  There is no queue of start states (fast_ok needs shared tables).
// A compile-time choice, so that every table pointer has one provenance (ds_read or global_load, never flat); the PM = 0
// instantiations are the code they were.
//
// NLEV with PM != 0 (mdpp_noise_levels_per_env_mdp: a noise x seed sweep in one launch): both of the above at once.  The
// per-level cdfs depend on S and p only, so they stay ONE [levels][S][S] table shared by the envs' MDPs; they take the place
// of the handle's own cdf, which is not staged: at closed_noise_lds_offset<PM> (behind the slots for PM = 2, at the start of
// dynamic LDS for PM = 1), nl.lds_bytes of them, the agent's LDS behind (closed_agent_lds_offset with nl.lds_bytes).  The
// workgroup stages the cdfs co-operatively and every lane its slots (tail lanes: set N - 1) BEFORE the barrier and the
// `i >= N` return; the level byte, sigma and (T, M) are loaded after it, so no tail lane reads level[i] beyond N.
#pragma once
#include "mdpp_internal.hpp"
#include "mdpp_rng.hpp"

namespace mdpp {

constexpr int kClosedRsrcFlags = 0x00020000;
typedef unsigned int closed_u32x2 __attribute__((ext_vector_type(2)));

// what an NLEV kernel takes besides the handle's DiscreteArgs (mdpp_set_noise_levels; device pointers)
struct NoiseLevelArgs {
    const uint8_t *level;       // [N] the env's transition-noise level
    const double *sigma;        // [N] the env's reward-noise sigma
    const double *cdf;          // [levels][S][S] the categoricals' cdfs per level (a level of value 0: never read)
    const uint32_t *T;          // [levels] philox_pnoise_threshold of the level's value (0 <=> the value is 0)
    const uint64_t *M;          // [levels] philox_pnoise_magic(T, S)
    uint32_t levels;
    uint32_t lds_bytes;         // the cdfs are staged in LDS at lds + a.lds_bytes and take this much (16-aligned); 0: global memory
};

// A NOISE kernel's static LDS (kZigLdsBytes): numpy's ziggurat tables, staged by the workgroup; the step's barrier covers them
template <bool NOISE>
__device__ __forceinline__ ZigLds closed_loop_zig_lds() {
    __shared__ uint64_t s_ki[NOISE ? 256 : 1];
    __shared__ double s_wi[NOISE ? 256 : 1], s_fi[NOISE ? 256 : 1];
    if (NOISE) zig_stage(s_ki, s_wi, s_fi, threadIdx.x, kBlock);
    return ZigLds{s_ki, s_wi, s_fi};
}

// PM = 2: this lane's column of the workgroup's MDP slots, as the step reads it
struct ClosedSlots {
    const uint32_t *w;          // dword 0 of this lane: dword k at w[k 256]
    uint32_t oP, oterm, orew, oinit;    // the carve in dwords
    __device__ __forceinline__ uint32_t byte_of(uint32_t o, uint32_t k) const { return (w[(o + (k >> 2)) * kBlock] >> ((k & 3u) * 8u)) & 0xFFu; }
    __device__ __forceinline__ double double_of(uint32_t o, uint32_t k) const {
        return __hiloint2double((int)w[(o + 2u * k + 1u) * kBlock], (int)w[(o + 2u * k) * kBlock]);
    }
    __device__ __forceinline__ uint32_t next(uint32_t k) const { return byte_of(oP, k); }
    __device__ __forceinline__ bool terminal(uint32_t s) const { return byte_of(oterm, s) != 0u; }
    __device__ __forceinline__ uint32_t reward_byte(uint32_t k) const { return byte_of(orew, k); }
    __device__ __forceinline__ double reward(uint32_t k) const { return double_of(orew, k); }
    __device__ __forceinline__ int start(int S, double u) const {       // searchsorted_right on the lane's cdf
        int c = 0;
        for (int j = 0; j < S; j++) c += (double_of(oinit, (uint32_t)j) <= u) ? 1 : 0;
        return c;
    }
};
// PM = 2: n bytes / n doubles of src into dword o onwards of the lane whose dword 0 is w
__device__ __forceinline__ void closed_stage_bytes(uint32_t *w, uint32_t o, const uint8_t *src, uint32_t n) {
    for (uint32_t k = 0; k < n; k += 4u) {
        uint32_t v = 0;
        for (uint32_t b = 0; b < 4u && k + b < n; b++) v |= (uint32_t)src[k + b] << (8u * b);
        w[(o + (k >> 2)) * kBlock] = v;
    }
}
__device__ __forceinline__ void closed_stage_doubles(uint32_t *w, uint32_t o, const double *src, uint32_t n) {
    for (uint32_t k = 0; k < n; k++) {
        const double v = src[k];
        w[(o + 2u * k) * kBlock] = (uint32_t)__double2loint(v);
        w[(o + 2u * k + 1u) * kBlock] = (uint32_t)__double2hiint(v);
    }
}
// Where the shared transition-noise cdf lies in a PM kernel's dynamic LDS, and where the agent's LDS starts behind it
// (PM = 0: a.lds_noise and a.lds_bytes, the handle's own carve)
template <int PM>
__host__ __device__ __forceinline__ uint32_t closed_noise_lds_offset(const DiscreteArgs &a) {
    return PM == 2 ? (uint32_t)kBlock * a.lds_noise : PM == 1 ? 0u : a.lds_noise;
}
template <int PM>
__host__ __device__ __forceinline__ uint32_t closed_agent_lds_offset(const DiscreteArgs &a) {
    return PM == 0 ? a.lds_bytes : closed_noise_lds_offset<PM>(a) + (a.lds_bytes - a.lds_noise);
}
// ... in an NLEV kernel, whose per-level cdfs (nl_lds bytes; 0: they are read in global memory) lie where the shared cdf
// would: behind the whole carve (PM = 0: the shared cdf keeps its room, unstaged), in its place (PM != 0)
template <int PM>
__host__ __device__ __forceinline__ uint32_t closed_nlev_lds_offset(const DiscreteArgs &a) {
    return PM == 0 ? a.lds_bytes : closed_noise_lds_offset<PM>(a);
}
template <int PM>
__host__ __device__ __forceinline__ uint32_t closed_agent_lds_offset(const DiscreteArgs &a, uint32_t nl_lds) {
    return closed_nlev_lds_offset<PM>(a) + nl_lds;
}

// (a is the kernel's by-value argument, taken by const reference: see tick_now in mdpp_internal.hpp for what a write costs)
template <bool PHILOX, bool NOISE, bool UNIT, bool SUMMARY = false, bool NLEV = false, int PM = 0, bool LOG = false, class Agent>
__device__ __forceinline__ void closed_loop_rollout(const DiscreteArgs &a, int K, const bool obs64, int32_t *actions,
                                                    void *__restrict__ obs, float *__restrict__ reward,
                                                    uint8_t *__restrict__ term, uint8_t *__restrict__ trunc,
                                                    unsigned char *lds, const ZigLds &zig, Agent &agent,
                                                    const EpisodeSummaryArgs &sm = EpisodeSummaryArgs{},
                                                    const NoiseLevelArgs &nl = NoiseLevelArgs{}) {
    static_assert(NOISE || !NLEV, "per-env noise levels are levels of a NOISE kernel");
    static_assert(SUMMARY || !LOG, "the episode log is kept by the summary form");
    const uint64_t ptick0 = tick_now(a);               // the step counter at this launch (through the device-side offset of a graph replay)
    const uint32_t rhead0 = ring_head_now(a, ptick0);  // ... and the head of a delay line kept in memory
    const int tid = threadIdx.x;
    const uint32_t i = blockIdx.x * kBlock + tid;
    const int S = a.S, A = a.A, L = a.L;
    const uint32_t N = (uint32_t)a.N;
    // stage the shared MDP (and the noise categoricals), then what the agent keeps in LDS
    if constexpr (PM == 0) {
        for (uint32_t k = tid; k < (uint32_t)S * (uint32_t)A; k += kBlock) lds[a.lds_P + k] = a.P[k];
        for (int k = tid; k < S; k += kBlock) {
            lds[a.lds_term + k] = a.is_term[k];
            ((double *)(lds + a.lds_init))[k] = a.init_cdf[k];
        }
        if (UNIT)
            for (uint32_t k = tid; k < a.rbits_stride; k += kBlock) lds[a.lds_rew + k] = a.rbits[k];
        else
            for (uint32_t k = tid; k < a.nkeys; k += kBlock) ((double *)(lds + a.lds_rew))[k] = a.rtable[k];
    }
    if constexpr (PM == 2) {         // ... or this lane's own MDP into its column of the slots (tail lanes: the last env's)
        uint32_t *const w = (uint32_t *)lds + tid;
        const size_t ti = (size_t)(i < N ? i : N - 1u);
        closed_stage_bytes(w, a.lds_P / 4u, a.P + ti * (size_t)(S * A), (uint32_t)(S * A));
        closed_stage_bytes(w, a.lds_term / 4u, a.is_term + ti * (size_t)S, (uint32_t)S);
        closed_stage_doubles(w, a.lds_init / 4u, a.init_cdf + ti * (size_t)S, (uint32_t)S);
        if (UNIT) closed_stage_bytes(w, a.lds_rew / 4u, a.rbits + ti * (size_t)a.rbits_stride, a.rbits_stride);
        else closed_stage_doubles(w, a.lds_rew / 4u, a.rtable + ti * (size_t)a.nkeys, a.nkeys);
    }
    const bool pn_lds = !NLEV && NOISE && a.has_p_noise && a.noise_in_lds;
    if (pn_lds)
        for (int k = tid; k < S * S; k += kBlock) ((double *)(lds + (PM == 0 ? a.lds_noise : closed_noise_lds_offset<PM>(a))))[k] = a.noise_cdf[k];
    if constexpr (NLEV) {
        if (!PHILOX && a.has_p_noise && nl.lds_bytes != 0u)
            for (uint32_t k = tid; k < nl.levels * (uint32_t)(S * S); k += kBlock) ((double *)(lds + closed_nlev_lds_offset<PM>(a)))[k] = nl.cdf[k];
    }
    agent.stage(tid);
    __syncthreads();
    if (i >= N) return;
    // the tables: in LDS (PM = 0), this lane's set in global memory (PM = 1); PM = 2 reads its slots through ts instead
    const uint8_t *const tP = PM == 1 ? a.P + (size_t)i * (size_t)(S * A) : lds + a.lds_P;
    const uint8_t *const tterm = PM == 1 ? a.is_term + (size_t)i * (size_t)S : lds + a.lds_term;
    const uint8_t *const trbits = PM == 1 ? a.rbits + (size_t)i * (size_t)a.rbits_stride : lds + a.lds_rew;
    const double *const trtable = PM == 1 ? a.rtable + (size_t)i * (size_t)a.nkeys : (const double *)(lds + a.lds_rew);
    const double *const tinit = PM == 1 ? a.init_cdf + (size_t)i * (size_t)S : (const double *)(lds + a.lds_init);
    const double *const tnoise = (const double *)(lds + (PM == 0 ? a.lds_noise : closed_noise_lds_offset<PM>(a)));
    const ClosedSlots ts{(const uint32_t *)lds + tid, a.lds_P / 4u, a.lds_term / 4u, a.lds_rew / 4u, a.lds_init / 4u};
    const uint64_t genv = (uint64_t)(a.env_id_offset + (int64_t)i);
    // NLEV: this lane's sigma, its level's (T, M) and where its level's cdfs start (in doubles)
    double lane_sigma = 0.0;
    uint32_t lane_T = 0u, lane_cdf = 0u;
    uint64_t lane_M = 0ull;
    if constexpr (NLEV) {
        const uint32_t lev = nl.level[i];
        lane_sigma = nl.sigma[i];
        lane_T = nl.T[lev];
        if (PHILOX) lane_M = nl.M[lev];
        else lane_cdf = lev * (uint32_t)(S * S);
    }
    agent.begin(i, genv, ptick0);
    double ep_ret = 0.0, ep_return_sum = 0.0;           // SUMMARY: this env's five values
    int32_t ep_len = 0, ep_count = 0, ep_length_sum = 0;
    uint32_t ep_logged = 0;                             // LOG: the episodes the log has seen this env finish ...
    uint64_t log_at = 0;                                // ... and the element ep_logged N + i of its next row
    if constexpr (SUMMARY) {
        ep_ret = sm.ret[i]; ep_len = sm.len[i];
        ep_count = sm.episodes[i]; ep_return_sum = sm.return_sum[i]; ep_length_sum = sm.length_sum[i];
        if constexpr (LOG) {
            ep_logged = (uint32_t)sm.log_count[i];
            log_at = (uint64_t)ep_logged * (uint64_t)N + (uint64_t)i;
        }
    }

    const uint4 st = a.state[i];
    // fast_ok handles: word 1 is the queue of start states {24 bits of 4-bit entries, next one lowest; count in bits 24-26},
    // and history bytes 4-7 do not exist (L <= 3: never read)
    const bool queued = PM == 0 && a.fast_ok != 0;
    uint64_t hist = ((uint64_t)(queued ? 0xFFFFFFFFu : st.y) << 32) | st.x;      // newest state in byte 0, 0xFF = NaN
    uint32_t qv = st.y & 0x00FFFFFFu, qc = (st.y >> 24) & 7u;
    uint32_t steps = st.z, ringbits = st.w;
    const bool next_step = a.autoreset == MDPP_AUTORESET_NEXT_STEP;
    bool pending = next_step && (steps >> 31) != 0;     // bit 31 of the step counter: the next call is this env's reset
    steps &= 0x7FFFFFFFu;
    uint32_t phase = steps % (uint32_t)a.every_n;       // steps % every_n, kept incrementally below

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
    auto reward_noise = [&](uint64_t ptick) -> double {
        if constexpr (NLEV)
            return 0.0 + lane_sigma * (PHILOX ? (double)rn_z.normal(a.philox_seed, genv, ptick, kPhiloxRNoiseStream) : np_standard_normal_lds(env_pcg, zig));
        else return 0.0 + a.r_noise * (PHILOX ? (double)rn_z.normal(a.philox_seed, genv, ptick, kPhiloxRNoiseStream) : np_standard_normal_lds(env_pcg, zig));
    };

    const uint32_t total = SUMMARY ? 0u : (uint32_t)K * N;     // (the launcher keeps 8 K N below 2^32; SUMMARY: nothing is stored)
    auto r_act = __builtin_amdgcn_make_buffer_rsrc((void *)actions, 0, total * 4u, kClosedRsrcFlags);
    auto r_obs = __builtin_amdgcn_make_buffer_rsrc(obs, 0, total * (obs64 ? 8u : 4u), kClosedRsrcFlags);
    auto r_rew = __builtin_amdgcn_make_buffer_rsrc((void *)reward, 0, total * 4u, kClosedRsrcFlags);
    auto r_term = __builtin_amdgcn_make_buffer_rsrc((void *)term, 0, total, kClosedRsrcFlags);
    auto r_trunc = __builtin_amdgcn_make_buffer_rsrc((void *)trunc, 0, total, kClosedRsrcFlags);
    const uint32_t v1 = i, v4 = i * 4u, v8 = i * 8u;
    auto put_obs = [&](uint32_t s, uint32_t so) {       // (the width: a constant or wave-uniform)
        if constexpr (SUMMARY) { (void)s; (void)so; }
        else if (obs64) __builtin_amdgcn_raw_buffer_store_b64(closed_u32x2{s, 0u}, r_obs, v8, so * 8u, MDPP_ST_NT);
        else __builtin_amdgcn_raw_buffer_store_b32(s, r_obs, v4, so * 4u, MDPP_ST_NT);
    };

    // reset(): the first state of the next episode (:2255: one uniform, searchsorted(cdf, u, 'right'))
    auto start_state = [&](uint64_t ptick) -> uint32_t {
        if (PHILOX) {        // one word of the start-state stream per tick (mdpp_rng.hpp)
            if constexpr (PM == 2) return (uint32_t)ts.start(S, philox_start_uniform(philox_start_m31(a.philox_seed, genv, ptick, kPhiloxStartStream)));
            else return (uint32_t)searchsorted_right(tinit, S, philox_start_uniform(philox_start_m31(a.philox_seed, genv, ptick, kPhiloxStartStream)));
        }
        if (queued && qc != 0) {                        // the next draws of the stream, made ahead by another kernel
            const uint32_t s0 = qv & 0xFu;
            qv >>= 4; qc -= 1;
            return s0;
        }
        if constexpr (PM == 2) return (uint32_t)ts.start(S, np_random(env_pcg));
        else return (uint32_t)searchsorted_right(tinit, S, np_random(env_pcg));
    };
    auto episode_start = [&](uint32_t s0) {
        hist = 0xFFFFFFFFFFFFFF00ULL | (uint64_t)s0;
        steps = 0; phase = 0; ringbits = 0;
        if (!UNIT)
            for (int d = 0; d < a.delay; d++) a.ring_keys[(size_t)d * N + i] = kNoKey;
    };

    for (int k = 0; k < K; k++) {
        const uint64_t ptick = ptick0 + (uint64_t)k;
        const uint32_t so = (uint32_t)k * N;
        if (k == 0 || (ptick & 3u) == 0u) agent.next_block(genv, ptick);            // (wave-uniform)
        const uint32_t cur = (uint32_t)hist & 0xFFu;
        const uint32_t action = agent.act(cur, ptick);
        if constexpr (!SUMMARY) __builtin_amdgcn_raw_buffer_store_b32(action, r_act, v4, so * 4u, MDPP_ST_NT);
        if (pending) {               // next-step autoreset: this call is the env's reset(), :2250-2278; the action is ignored, nothing is learnt
            const uint32_t s0 = start_state(ptick);
            episode_start(s0);
            put_obs(s0, so);
            if constexpr (!SUMMARY) {
                __builtin_amdgcn_raw_buffer_store_b32(0u, r_rew, v4, so * 4u, MDPP_ST_NT);
                __builtin_amdgcn_raw_buffer_store_b8((uint8_t)0, r_term, v1, so, MDPP_ST_NT);
                __builtin_amdgcn_raw_buffer_store_b8((uint8_t)0, r_trunc, v1, so, MDPP_ST_NT);
            }
            pending = false;
            continue;
        }
        uint32_t nxt;
        if constexpr (PM == 2) nxt = ts.next(cur * (uint32_t)A + action);
        else nxt = tP[cur * (uint32_t)A + action];                              // D1
        if (NOISE && a.has_p_noise) {                                               // D2
            // (Philox streams: one word of the tick decides "noisy" and which other state; numpy streams: the state space's own
            //  generator and the categorical's cdf, as in the reference)
            if constexpr (NLEV) {
                if (PHILOX) nxt = philox_pnoise_state(pn_w.word(a.philox_seed, genv, ptick, kPhiloxPNoiseStream), lane_T, lane_M, nxt);
                else if (lane_T != 0u) {            // (a lane of level 0 makes no draw: its space stream does not move)
                    const double u = np_random(sp_pcg);
                    const uint32_t row = lane_cdf + nxt * (uint32_t)S;
                    if (nl.lds_bytes != 0u) nxt = (uint32_t)searchsorted_right((const double *)(lds + closed_nlev_lds_offset<PM>(a)) + row, S, u);
                    else nxt = (uint32_t)searchsorted_right(nl.cdf + row, S, u);
                }
            }
            else if (PHILOX) nxt = philox_pnoise_state(pn_w.word(a.philox_seed, genv, ptick, kPhiloxPNoiseStream), a.pn_T, a.pn_M, nxt);
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
        bool done;
        if constexpr (PM == 2) done = ts.terminal(nxt);
        else done = tterm[nxt] != 0;                                          // D7
        float rout;
        if (UNIT) {
            uint32_t bit = 0;
            if constexpr (PM == 2) { if (key != kNoKey) bit = (ts.reward_byte(key >> 3) >> (key & 7u)) & 1u; }
            else if (key != kNoKey) bit = (trbits[key >> 3] >> (key & 7u)) & 1u;
            if (a.delay > 0) {                                                      // D5 (shift register)
                const uint32_t out = (ringbits >> (a.delay - 1)) & 1u;
                ringbits = (ringbits << 1) | bit;
                bit = out;
            }
            if (phase != 0) bit = 0;                                                // D6
            if (NOISE && a.has_r_noise) {
                double r = bit ? 1.0 : 0.0;
                r += reward_noise(ptick);
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
            double r;
            if constexpr (PM == 2) r = (key != kNoKey) ? ts.reward(key) : 0.0;
            else r = (key != kNoKey) ? trtable[key] : 0.0;
            if (phase != 0) r = 0.0;                                                // D6
            if (NOISE && a.has_r_noise) r += reward_noise(ptick);
            r *= a.scale;
            r += a.shift;
            if (done) r += a.term_add;
            rout = (float)r;
        }
        const bool truncated = (a.max_steps > 0) && (steps >= (uint32_t)a.max_steps);
        agent.learn(cur, action, nxt, rout, done, truncated && a.autoreset != MDPP_AUTORESET_DISABLED, ptick);

        uint32_t out_state = nxt;
        if (next_step) pending = done || truncated;
        if (a.autoreset == MDPP_AUTORESET_SAME_STEP && (done || truncated)) {
            // same-step autoreset: the terminal transition's reward and flags, the first observation of the next episode
            out_state = start_state(ptick);
            episode_start(out_state);
        }
        put_obs(out_state, so);
        agent.episode_end(done || truncated);
        if constexpr (SUMMARY) {
            ep_ret += (double)rout;
            ep_len += 1;
            if (done || truncated) {
                if constexpr (LOG) {        // the episode log: row ep_logged of the episode-major [log_cap][N] arrays, while there is one
                    if (ep_logged < sm.log_cap) {
                        __builtin_nontemporal_store(ep_ret, sm.log_ret + log_at);
                        __builtin_nontemporal_store(ep_len, sm.log_len + log_at);
                    }
                    ep_logged += 1;
                    log_at += (uint64_t)N;
                }
                ep_count += 1;
                ep_return_sum += ep_ret;
                ep_length_sum += ep_len;
                ep_ret = 0.0; ep_len = 0;
            }
        } else {
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(rout), r_rew, v4, so * 4u, MDPP_ST_NT);
            __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(done ? 1 : 0), r_term, v1, so, MDPP_ST_NT);
            __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(truncated ? 1 : 0), r_trunc, v1, so, MDPP_ST_NT);
        }
    }

    agent.finish(i);
    if constexpr (SUMMARY) {
        sm.ret[i] = ep_ret; sm.len[i] = ep_len;
        sm.episodes[i] = ep_count; sm.return_sum[i] = ep_return_sum; sm.length_sum[i] = ep_length_sum;
        if constexpr (LOG) sm.log_count[i] = (int32_t)ep_logged;
    }
    a.state[i] = make_uint4((uint32_t)hist, queued ? (qv | (qc << 24)) : (uint32_t)(hist >> 32),
                            steps | (pending ? 0x80000000u : 0u), ringbits);
    if (use_env) env_pcg.store(a.env_s, i);
    if (use_sp) sp_pcg.store(a.sp_s, i);
}

// ---- host side ---------------------------------------------------------------------------------------------------------
constexpr size_t kZigLdsBytes = 3u * 256u * 8u;        // a NOISE kernel's static LDS: the ziggurat tables

// Why this handle has no closed-loop launch ("<noun> rollouts ..."), or empty: the kernel serves it.  agent_lds: the LDS
// the agent needs whatever the launch (bytes), tables: what has to fit, for the message.  per_env_mdp: the agent has kernels
// for one MDP per env (PM), which a handle flagged by mdpp_learner_per_env_mdp runs: its tables are placed per launch
// (closed_agent_lds), so the LDS rule -- a shared MDP staged per workgroup -- does not apply to it
inline std::string closed_loop_refusal(const mdpp_env *h, const char *noun, bool serves_noise, uint64_t agent_lds, const char *tables,
                                       bool per_env_mdp = false) {
    const mdpp_config &c = h->cfg;
    const DiscreteArgs &a = h->dargs;
    const char *why = nullptr;
    const bool noise = c.has_transition_noise || c.has_reward_noise;
    if (c.kind != MDPP_KIND_DISCRETE) why = "serve discrete envs only (this handle is continuous or a grid)";
    else if (c.image) why = "do not serve image observations";
    else if (c.irrelevant) why = "do not serve an irrelevant sub-space (irrelevant_features)";
    else if (c.num_tables != 1 && !(per_env_mdp && h->learn_pm)) why = "need one shared MDP (this handle has one MDP per env: seeds=[...])";
    else if (c.S > 255) why = "need at most 255 states (state_space_size)";
    else if (c.L > 7) why = "need sequence_length <= 7";
    else if (!serves_noise && c.has_transition_noise) why = "do not serve a transition_noise key";
    else if (!serves_noise && c.has_reward_noise) why = "do not serve a reward_noise key";
    else if (c.episode_stats) why = "do not keep episode_stats";
    else if (c.num_tables == 1 && (!a.rew_in_lds || (uint64_t)a.lds_bytes + agent_lds + (noise ? kZigLdsBytes : 0u) > 64u * 1024u))
        return std::string(noun) + " rollouts need " + tables + " within 64 KiB of LDS";
    return why ? std::string(noun) + " rollouts " + why : std::string();
}

// ---- per-env noise levels (mdpp_set_noise_levels): what a launch of the NLEV kernels needs from the handle
// the per-level cdfs as LDS bytes (16-aligned)
inline uint32_t noise_levels_cdf_lds_bytes(const mdpp_env *h) {
    return ((uint32_t)h->nl_levels * (uint32_t)h->cfg.S * (uint32_t)h->cfg.S * 8u + 15u) & ~15u;
}
// The envs' MDP slots of a PM = 2 kernel as LDS bytes: the carve up to the shared noise cdf, per lane
inline size_t closed_pm_slots_lds_bytes(const mdpp_env *h) { return (size_t)kBlock * (size_t)h->dargs.lds_noise; }
// The closed-loop agents' LDS placement, the one rule of every learner and evaluation launch: which of the agent's Q-tables
// (q_lds bytes), the envs' MDP slots and the per-level cdfs go to LDS, the rest being read in global memory.  The three are
// ranked by what leaving each in global memory was measured to cost on one MDP per env with levels -- the Q-tables (+49-56 %:
// touched several times a step), the slots (+17-26 %), the cdfs (+15-18 %: a row once a step) -- so the subsets are tried in
// the order {Q, slots, cdfs}, {Q, slots}, {Q, cdfs}, {Q}, {slots, cdfs}, {slots}, {cdfs}, {}, and the first one granted is
// taken; {} is taken without asking.  A subset with a candidate that does not exist or is not allowed is skipped:
//   Q       q_lds != 0 (the agent keeps tables there), at most 160 KiB, not under MDPP_OPT_NO_LEARN_LDS
//   slots   pm only (the handle runs the PM kernels: PM = 2 with them, PM = 1 reads the MDPs in global memory); rew_in_lds,
//           at most 64 KiB per workgroup (256 B per lane) -- the bound closed_loop_refusal puts on a shared MDP's staged
//           tables, here a placement: 20 x 20 (608 B per lane) reads its MDPs in global memory --, not under MDPP_OPT_NO_PM_LDS
//   cdfs    a handle with per-env noise levels only, under noise_in_lds's rule (at most 32 KiB; numpy streams with a
//           transition_noise key: the others read no cdf); not under MDPP_OPT_NO_NLEV_LDS (shared MDP) / MDPP_OPT_NO_PM_NLEV_LDS (pm)
// granted(q, slots, cdfs, bytes): the device grants `bytes` of dynamic LDS to the kernel of that subset.  bytes: the chosen
// candidates and what the kernel stages whatever the placement -- the handle's carve on a shared MDP (with levels its own cdf
// keeps its room, unstaged), the shared noise cdf (a.lds_bytes - a.lds_noise) with pm, nothing with pm and levels (the per-level
// cdfs take the shared cdf's place).
struct ClosedLdsPlacement { bool q, slots, cdfs; };
template <class Granted>
inline ClosedLdsPlacement closed_agent_lds(const mdpp_env *h, size_t q_lds, bool pm, Granted &&granted) {
    const DiscreteArgs &a = h->dargs;
    const size_t slots = closed_pm_slots_lds_bytes(h), cdf = noise_levels_cdf_lds_bytes(h);
    const size_t fixed = !pm ? (size_t)a.lds_bytes : h->nl_on ? 0u : (size_t)(a.lds_bytes - a.lds_noise);
    const bool q_ok = q_lds != 0 && q_lds <= 160u * 1024u && !(h->opts & MDPP_OPT_NO_LEARN_LDS);
    const bool m_ok = pm && a.rew_in_lds && slots <= 64u * 1024u && !(h->opts & MDPP_OPT_NO_PM_LDS);
    const bool c_ok = h->nl_on && !a.philox && a.has_p_noise && cdf <= 32u * 1024u && !(h->opts & (pm ? MDPP_OPT_NO_PM_NLEV_LDS : MDPP_OPT_NO_NLEV_LDS));
    for (unsigned drop = 0; drop < 7u; drop++) {        // bit 2: without Q, bit 1: without the slots, bit 0: without the cdfs
        const bool q = !(drop & 4u), m = !(drop & 2u), c = !(drop & 1u);
        if ((q && !q_ok) || (m && !m_ok) || (c && !c_ok)) continue;
        if (granted(q, m, c, fixed + (q ? q_lds : 0u) + (m ? slots : 0u) + (c ? cdf : 0u))) return {q, m, c};
    }
    return {false, false, false};
}
inline NoiseLevelArgs noise_level_args(const mdpp_env *h, uint32_t cdf_lds) {
    return NoiseLevelArgs{(const uint8_t *)h->d_nl_level, (const double *)h->d_nl_sigma, (const double *)h->d_nl_cdf,
                          (const uint32_t *)h->d_nl_T, (const uint64_t *)h->d_nl_M, (uint32_t)h->nl_levels, cdf_lds};
}

// K closed-loop steps of kern with lds bytes of dynamic LDS.  name: the kernel's, with its template arguments -- a dry run
// (io.name_out) writes it and launches nothing.  agent_args(k0, kc, actions) makes the kernel's second argument for the
// launch of steps [k0, k0 + kc), whose actions go to `actions`.  lds_granted: the caller has asked dynamic_lds_ok for this
// kernel and size already.  SUMMARY: kern is a SUMMARY kernel, taking (args, agent args, K, *io.summary) -- it addresses no
// [K][N] array, so the call is one launch (MDPP_OPT_LEARN_SHORT_PIECES still cuts it).
template <bool SUMMARY, class Kern, class AgentArgs>
inline int launch_closed_loop(mdpp_env *h, const DiscreteIO &io, Kern kern, size_t lds, bool lds_granted, const char *name,
                              AgentArgs &&agent_args) {
    const std::string kernel(name, strcspn(name, "<"));
    DiscreteArgs a = h->dargs;
    stamp_step(a, h);
    // pieces: the buffer descriptors address < 4 GiB per output array (8 bytes per env-step at most)
    long long kmax = SUMMARY ? (long long)INT32_MAX : ((1LL << 32) - 1) / (8LL * a.N);
    if (kmax < 1) { h->err = kernel + ": num_envs too large"; return MDPP_EUNSUPPORTED; }
    if ((a.opts & MDPP_OPT_LEARN_SHORT_PIECES) && kmax > 5) kmax = 5;      // (tests: the pieces' hand-over at a small size)
    if (io.name_out) { snprintf(io.name_out, kNameLen, "%s", name); return MDPP_OK; }
    if (!lds_granted && !dynamic_lds_ok((const void *)kern, lds)) { h->err = kernel + ": the device refuses the launch's LDS"; return MDPP_EUNSUPPORTED; }
    const int grid = (a.N + kBlock - 1) / kBlock;
    // (io.actions, an input of every other launcher, is this one's OUTPUT: the caller's buffer for the actions taken; piece_of
    //  offsets it like the other arrays -- these handles have no irrelevant sub-space -- and the const comes off at the launch)
    for_each_piece(a, h, io, kmax, [&](const DiscreteIO &p, int k0) {
        if constexpr (SUMMARY)
            hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), lds, io.s, a, agent_args(k0, p.K, nullptr), p.K, *io.summary);
        else
            hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), lds, io.s, a, agent_args(k0, p.K, const_cast<int32_t *>(p.actions)), p.K,
                               p.obs, p.reward, p.term, p.trunc);
        return true;
    });
    return step_done(h, io.K, kernel.c_str());
}

// K steps of one form of an agent that keeps per-env Q-tables, the one launcher of the learners and the evaluation:
// the step's compile-time facts from the handle, the placement (closed_agent_lds), the kernel of both, its name and its
// dynamic LDS.  PMH: the handle has one MDP per env and runs the PM = 1 / PM = 2 kernels, else PM = 0.  A form F says
//   F::LOG                     the form has _log kernels, F::kernel_log<...>(), launched when io.summary carries an episode log
//   F::SUMMARY, F::NLEV        the step's form (NLEV: of a handle with per-env noise levels -- NOISE = 1 whatever its keys)
//   F::TABLES                  how many tables Q has (1, or 2 for double Q)
//   F::kernel<PH, NZ, UNIT, QL, PM>()                      the __global__ function
//   F::name(out, ph, nz, unit, ql, pm)                     its name with its template arguments, kNameLen bytes at most
//   F::args(h, io, k0, kc, actions, cdf_lds)               the kernel's second argument for the piece [k0, k0 + kc) of io's
//                                                          steps, with cdf_lds bytes of per-level cdfs staged in LDS
template <class F, bool PMH>
int launch_closed_form(mdpp_env *h, const DiscreteIO &io) {
    const DiscreteArgs &a = h->dargs;
    const size_t q_lds = (size_t)kBlock * (size_t)a.S * (size_t)a.A * sizeof(float) * F::TABLES;
    int rc = MDPP_OK;
    with_bools([&](auto PH, auto NZ, auto UNIT) {
        if constexpr (!F::NLEV || NZ()) {
            const ClosedLdsPlacement at = closed_agent_lds(h, q_lds, PMH, [&](bool q, bool m, bool, size_t bytes) {
                const void *k = nullptr;
                with_bools([&](auto QL, auto ML) {
                    if constexpr (PMH || !ML()) k = (const void *)F::template kernel<PH(), NZ(), UNIT(), QL(), PMH ? (ML() ? 2 : 1) : 0>();
                }, q, m);
                return dynamic_lds_ok(k, bytes);
            });
            const uint32_t cdf_lds = at.cdfs ? noise_levels_cdf_lds_bytes(h) : 0u;
            with_bools([&](auto QL, auto ML) {
                if constexpr (PMH || !ML()) {
                    constexpr int PM = PMH ? (ML() ? 2 : 1) : 0;
                    char name[kNameLen];
                    F::name(name, PH(), NZ(), UNIT(), QL(), PM);
                    const size_t agent_at = F::NLEV ? (size_t)closed_agent_lds_offset<PM>(a, cdf_lds) : (size_t)closed_agent_lds_offset<PM>(a);
                    // (granted already unless the placement is {}, which was not asked about)
                    const auto args = [&](int k0, int kc, int32_t *actions) { return F::args(h, io, k0, kc, actions, cdf_lds); };
                    bool with_log = false;
                    if constexpr (F::SUMMARY && F::LOG) with_log = io.summary && io.summary->log_cap != 0u;
                    if constexpr (F::SUMMARY && F::LOG) {
                        // with an episode log: the form's _log kernel -- same placement, same LDS, same reported name; asked about
                        // its LDS itself (the placement asked the summary kernel)
                        if (with_log) rc = launch_closed_loop<true>(h, io, F::template kernel_log<PH(), NZ(), UNIT(), QL(), PM>(), agent_at + (QL() ? q_lds : 0u), false, name, args);
                    }
                    if (!with_log)
                        rc = launch_closed_loop<F::SUMMARY>(h, io, F::template kernel<PH(), NZ(), UNIT(), QL(), PM>(), agent_at + (QL() ? q_lds : 0u),
                                                            at.q || at.slots || at.cdfs, name, args);
                }
            }, at.q, at.slots);
        }
    }, a.philox != 0, F::NLEV || a.has_p_noise || a.has_r_noise, a.unit_rewards != 0);
    return rc;
}

} // namespace mdpp
