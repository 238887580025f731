// In-kernel tabular TD learners: one Q-learning or SARSA agent per env instance, its Q-table beside the env state, K steps of
// "select epsilon-greedily from the env's own Q, step, update that Q" in ONE launch (mdpp_step_n_learn).  The step itself is
// closed_loop_rollout (mdpp_discrete_closed.hpp) WITH its NOISE branches; this file holds the agent.
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
//
// Q lives in a buffer of the handle, entry-major [S A][N]: lanes of a wave touching their own entry of the same (s, a)
// coalesce.  QLDS = 1: each lane's table is staged once per launch into q_lds[(s A + a) 256 + tid] behind the MDP's tables
// (bank = lane: no conflict whatever (s, a) each lane holds), every selection and update is LDS traffic, the tables are
// written back at the end.  QLDS = 0 (256 S A 4 bytes do not fit beside the MDP's tables): the same indexing on the buffer.
// The blocks of the two learner streams do not depend on the state: the block of the NEXT four ticks is made while the
// current one is used (it also serves sel(s', t + 1) at a block's last tick).
//
// PE = 1 (per-env hyper-parameters, mdpp_set_learner_params): the lane loads alpha[i], gamma[i], E[i] once in begin() -- three
// coalesced dword loads -- and keeps them in registers; i is the handle's local env index.  When any one parameter is
// per-env the host hands all three as arrays, so there is one PE form.
//
// DOUBLE = 1 (double Q-learning, MDPP_LEARN_DOUBLE_Q): two tables per env, A then B, in the same entry-major buffer
// [2 S A][N] (entry e of B at S A + e; in LDS likewise, 256 x 2 S A floats per workgroup):
//   sel(s, t):  explore as above; greedy: the lowest j maximising QA[s][j] + QB[s][j] (one float32 addition per j, strict >)
//   update:     wU = the tick's word of kPhiloxLearnUpdateStream (made one block ahead like the other two); wU >> 31 == 0:
//               X = A, Y = B, otherwise X = B, Y = A;  terminated: y = r;  otherwise a* = the lowest argmax_j X[s'][j],
//               y = r + gamma Y[s'][a*];  q = X[s][a];  d = y - q;  u = alpha d;  X[s][a] = q + u
//   no carry; a reset call selects, writes and ignores an action, updates nothing and leaves its wU unused.
//
// PE and DOUBLE are template parameters: the uniform q_learning / sarsa instantiations are the code they were.  Each
// (PE, DOUBLE) pair other than (0, 0) is instantiated in a translation unit of its own (mdpp_discrete_learn_pe.hip,
// mdpp_discrete_learn_double.hip, mdpp_discrete_learn_double_pe.hip define the macros below and include this file).
//
// k_discrete_learn_summary (mdpp_step_n_learn_summary) is the same agent around closed_loop_rollout's SUMMARY form: the same
// steps, selections and updates, five per-env episode numbers instead of the [K][N] arrays.  Its instantiations live in four
// further translation units (mdpp_discrete_learn*_summary.hip: MDPP_LEARN_TU_SUMMARY), one per (PE, DOUBLE) pair.
//
// Per-env noise levels (mdpp_set_noise_levels): k_discrete_learn_rollout_nlev / k_discrete_learn_summary_nlev are the PE
// learner around closed_loop_rollout's NLEV form, NOISE = 1 always -- kernels of their own names, so that every kernel above
// keeps its symbol.  The per-level cdfs, when staged, lie between the MDP's tables and the Q-tables in LDS.  Four more
// translation units (mdpp_discrete_learn*_pe_nlev*.hip: MDPP_LEARN_TU_NLEV), one per (DOUBLE, SUMMARY) pair.
#include "mdpp_discrete_closed.hpp"

#ifndef MDPP_LEARN_TU_NLEV
#define MDPP_LEARN_TU_NLEV 0       // 1: this translation unit holds the per-env noise-level kernels (PE = 1) of its (DOUBLE, SUMMARY) pair, and nothing else
#endif
#ifndef MDPP_LEARN_TU_PE
#define MDPP_LEARN_TU_PE 0         // 1: this translation unit holds the PE = 1 instantiations
#endif
#ifndef MDPP_LEARN_TU_DOUBLE
#define MDPP_LEARN_TU_DOUBLE 0     // 1: ... the DOUBLE = 1 instantiations
#endif
#ifndef MDPP_LEARN_TU_SUMMARY
#define MDPP_LEARN_TU_SUMMARY 0    // 1: ... k_discrete_learn_summary's of that (PE, DOUBLE) pair, and nothing else
#endif

namespace mdpp {

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
// ... of the PE form: the per-env parameters, [N] each (device); alpha, gamma and E above are unused
struct LearnArgsPE : LearnArgs {
    const float *pe_alpha, *pe_gamma;
    const uint32_t *pe_E;
};

template <bool QLDS, bool PE, bool DOUBLE>
struct LearnAgent {
    const std::conditional_t<PE, LearnArgsPE, LearnArgs> &p;
    float *q_lds;               // this lane's column of the workgroup's tables: entry e at q_lds[e 256]
    uint32_t A, SA, N;          // (DOUBLE: SA is ONE table's entries; B's entry e is SA + e)
    float *qg;                  // this lane's table in the buffer: entry e at qg[e N]
    bool sarsa, have_carry;
    uint32_t carried;
    // the learner's words: the blocks of ticks 4 b .. 4 b + 3 in *_cur (b = blk_cur), the next ones made ahead in *_nxt
    uint32_t e_cur[4], e_nxt[4], x_cur[4], x_nxt[4];
    uint32_t u_cur[4], u_nxt[4];    // DOUBLE: which table learns
    uint64_t blk_cur;
    float pe_alpha, pe_gamma;   // PE: this lane's parameters
    uint32_t pe_E;

    __device__ __forceinline__ float alpha() const { if constexpr (PE) return pe_alpha; else return p.alpha; }
    __device__ __forceinline__ float gamma() const { if constexpr (PE) return pe_gamma; else return p.gamma; }
    __device__ __forceinline__ uint32_t E() const { if constexpr (PE) return pe_E; else return p.E; }
    __device__ __forceinline__ uint32_t entries() const { return DOUBLE ? 2u * SA : SA; }

    __device__ __forceinline__ float qget(uint32_t e) const {
        if constexpr (QLDS) return q_lds[e * kBlock];
        else return qg[(size_t)e * N];
    }
    __device__ __forceinline__ void qput(uint32_t e, float v) {
        if constexpr (QLDS) q_lds[e * kBlock] = v;
        else qg[(size_t)e * N] = v;
    }
    __device__ __forceinline__ void stage(int) {}
    __device__ __forceinline__ void begin(uint32_t i, uint64_t genv, uint64_t ptick0) {
        qg = p.q + i;
        if constexpr (PE) { pe_alpha = p.pe_alpha[i]; pe_gamma = p.pe_gamma[i]; pe_E = p.pe_E[i]; }
        if (QLDS)
            for (uint32_t e = 0; e < entries(); e++) q_lds[e * kBlock] = qg[(size_t)e * N];
        philox_start_block(p.seed, genv, ptick0 >> 2, kPhiloxLearnExploreStream, e_nxt);
        philox_start_block(p.seed, genv, ptick0 >> 2, kPhiloxLearnActionStream, x_nxt);
        if constexpr (DOUBLE) philox_start_block(p.seed, genv, ptick0 >> 2, kPhiloxLearnUpdateStream, u_nxt);
        blk_cur = 0;
        sarsa = !DOUBLE && p.algo == MDPP_LEARN_SARSA;
        have_carry = false;
        carried = 0;
        if (p.carry_in) {
            const int32_t c = p.carry[i];
            have_carry = c >= 0;
            carried = have_carry ? (uint32_t)c : 0u;
        }
    }
    __device__ __forceinline__ void next_block(uint64_t genv, uint64_t ptick) {
#pragma unroll
        for (int q = 0; q < 4; q++) { e_cur[q] = e_nxt[q]; x_cur[q] = x_nxt[q]; }
        if constexpr (DOUBLE) {
#pragma unroll
            for (int q = 0; q < 4; q++) u_cur[q] = u_nxt[q];
        }
        blk_cur = ptick >> 2;
        philox_start_block(p.seed, genv, blk_cur + 1u, kPhiloxLearnExploreStream, e_nxt);
        philox_start_block(p.seed, genv, blk_cur + 1u, kPhiloxLearnActionStream, x_nxt);
        if constexpr (DOUBLE) philox_start_block(p.seed, genv, blk_cur + 1u, kPhiloxLearnUpdateStream, u_nxt);
    }
    // max_j Q[s][j] and the lowest j that attains it
    __device__ __forceinline__ float row_best(uint32_t s, uint32_t &arg) const { return row_best_at(s * A, arg); }
    // ... of the row that starts at entry e0
    __device__ __forceinline__ float row_best_at(uint32_t e0, uint32_t &arg) const {
        float best = qget(e0);
        uint32_t bj = 0;
        for (uint32_t j = 1; j < A; j++) {
            const float v = qget(e0 + j);
            if (v > best) { best = v; bj = j; }
        }
        arg = bj;
        return best;
    }
    // DOUBLE: the lowest j maximising QA[s][j] + QB[s][j]
    __device__ __forceinline__ uint32_t row_best_sum(uint32_t s) const {
        const uint32_t e0 = s * A;
        float best = qget(e0) + qget(SA + e0);
        uint32_t bj = 0;
        for (uint32_t j = 1; j < A; j++) {
            const float v = qget(e0 + j) + qget(SA + e0 + j);
            if (v > best) { best = v; bj = j; }
        }
        return bj;
    }
    // sel(s, tick), tick in the current block or the first of the next
    __device__ __forceinline__ uint32_t select(uint32_t s, uint64_t tick) const {
        const bool in_cur = (tick >> 2) == blk_cur;     // (wave-uniform)
        const uint32_t wE = in_cur ? philox_word_of(e_cur, tick) : philox_word_of(e_nxt, tick);
        if ((wE >> 1) < E()) {
            const uint32_t wA = in_cur ? philox_word_of(x_cur, tick) : philox_word_of(x_nxt, tick);
            return (uint32_t)(((uint64_t)wA * (uint64_t)A) >> 32);
        }
        if constexpr (DOUBLE) return row_best_sum(s);
        uint32_t j;
        (void)row_best(s, j);
        return j;
    }
    __device__ __forceinline__ uint32_t act(uint32_t cur, uint64_t ptick) {
        const uint32_t action = have_carry ? carried : select(cur, ptick);
        have_carry = false;
        return action;
    }
    // target from the true next state, on Q as it is before this step's update
    __device__ __forceinline__ void learn(uint32_t cur, uint32_t action, uint32_t nxt, float rout, bool done, bool truncated_with_reset, uint64_t ptick) {
        if constexpr (DOUBLE) {
            // X: the table this tick's word picks, Y: the other one (x0, y0: their first entries)
            const uint32_t x0 = (philox_word_of(u_cur, ptick) >> 31) ? SA : 0u, y0 = SA - x0;
            float y = rout;
            if (!done) {
                uint32_t a2;
                (void)row_best_at(x0 + nxt * A, a2);
                const float g = gamma() * qget(y0 + nxt * A + a2);
                y = rout + g;
            }
            const uint32_t e = x0 + cur * A + action;
            const float q = qget(e);
            const float d = y - q;
            const float u = alpha() * d;
            qput(e, q + u);
            return;
        }
        float y = rout;
        uint32_t a2 = 0;
        if (!done) {
            float qn;
            if (sarsa) {                                                            // (wave-uniform)
                a2 = select(nxt, ptick + 1u);
                qn = qget(nxt * A + a2);
            } else {
                qn = row_best(nxt, a2);
            }
            const float g = gamma() * qn;
            y = rout + g;
        }
        const uint32_t e = cur * A + action;
        const float q = qget(e);
        const float d = y - q;
        const float u = alpha() * d;
        qput(e, q + u);
        // sarsa: the next step of this call takes a' when it starts from s'
        have_carry = sarsa && !done && !truncated_with_reset;
        carried = a2;
    }
    __device__ __forceinline__ void finish(uint32_t i) {
        if (QLDS)
            for (uint32_t e = 0; e < entries(); e++) qg[(size_t)e * N] = q_lds[e * kBlock];
        if (p.carry_out) p.carry[i] = have_carry ? (int32_t)carried : -1;
    }
};

template <bool PHILOX, bool NOISE, bool UNIT, bool QLDS, bool PE = false, bool DOUBLE = false>
__global__ __launch_bounds__(kBlock) void k_discrete_learn_rollout(DiscreteArgs a, std::conditional_t<PE, LearnArgsPE, LearnArgs> p, int K,
                                                                   void *__restrict__ obs,
                                                                   float *__restrict__ reward,
                                                                   uint8_t *__restrict__ term,
                                                                   uint8_t *__restrict__ trunc) {
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ uint64_t s_ki[NOISE ? 256 : 1];          // numpy's ziggurat tables (kZigLdsBytes)
    __shared__ double s_wi[NOISE ? 256 : 1], s_fi[NOISE ? 256 : 1];
    if (NOISE) zig_stage(s_ki, s_wi, s_fi, threadIdx.x, kBlock);
    LearnAgent<QLDS, PE, DOUBLE> agent{p, (float *)(lds + a.lds_bytes) + threadIdx.x, (uint32_t)a.A, (uint32_t)a.S * (uint32_t)a.A, (uint32_t)a.N};
    closed_loop_rollout<PHILOX, NOISE, UNIT>(a, K, !a.obs_i32, p.actions, obs, reward, term, trunc, lds, ZigLds{s_ki, s_wi, s_fi}, agent);
}

// ... keeping episode summaries instead of writing the [K][N] arrays (p.actions is unused)
template <bool PHILOX, bool NOISE, bool UNIT, bool QLDS, bool PE = false, bool DOUBLE = false>
__global__ __launch_bounds__(kBlock) void k_discrete_learn_summary(DiscreteArgs a, std::conditional_t<PE, LearnArgsPE, LearnArgs> p, int K,
                                                                   EpisodeSummaryArgs sm) {
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ uint64_t s_ki[NOISE ? 256 : 1];
    __shared__ double s_wi[NOISE ? 256 : 1], s_fi[NOISE ? 256 : 1];
    if (NOISE) zig_stage(s_ki, s_wi, s_fi, threadIdx.x, kBlock);
    LearnAgent<QLDS, PE, DOUBLE> agent{p, (float *)(lds + a.lds_bytes) + threadIdx.x, (uint32_t)a.A, (uint32_t)a.S * (uint32_t)a.A, (uint32_t)a.N};
    closed_loop_rollout<PHILOX, NOISE, UNIT, true>(a, K, false, nullptr, nullptr, nullptr, nullptr, nullptr, lds, ZigLds{s_ki, s_wi, s_fi}, agent, sm);
}

// the kernel of one form: full output, or summaries
template <bool SUMMARY, bool PH, bool NZ, bool UNIT, bool QL, bool PE, bool DOUBLE>
static constexpr auto learn_kernel() {
    if constexpr (SUMMARY) return k_discrete_learn_summary<PH, NZ, UNIT, QL, PE, DOUBLE>;
    else return k_discrete_learn_rollout<PH, NZ, UNIT, QL, PE, DOUBLE>;
}

// K learning steps of one (PE, DOUBLE) form
template <bool PE, bool DOUBLE, bool SUMMARY = false>
static int launch_learn_form(mdpp_env *h, const DiscreteIO &io) {
    const DiscreteArgs &a = h->dargs;
    const size_t q_lds = (size_t)kBlock * (size_t)a.S * (size_t)a.A * sizeof(float) * (DOUBLE ? 2u : 1u);
    int rc = MDPP_OK;
    with_bools([&](auto PH, auto NZ, auto UNIT) {
        // the LDS form when a workgroup's 256 tables fit beside the MDP's (and the device grants it)
        const bool qlds = !(h->opts & MDPP_OPT_NO_LEARN_LDS) && q_lds <= 160u * 1024u &&
                          dynamic_lds_ok((const void *)learn_kernel<SUMMARY, PH(), NZ(), UNIT(), true, PE, DOUBLE>(), (size_t)a.lds_bytes + q_lds);
        with_bools([&](auto QL) {
            char name[kNameLen];
            snprintf(name, kNameLen, "%s<PHILOX=%d,NOISE=%d,UNIT=%d,QLDS=%d%s%s>", SUMMARY ? "k_discrete_learn_summary" : "k_discrete_learn_rollout",
                     PH(), NZ(), UNIT(), QL(), PE ? ",PE=1" : "", DOUBLE ? ",DOUBLE=1" : "");
            rc = launch_closed_loop(h, io, learn_kernel<SUMMARY, PH(), NZ(), UNIT(), QL(), PE, DOUBLE>(), (size_t)a.lds_bytes + (QL() ? q_lds : 0u), QL(), name,
                                    [&](int k0, int kc, int32_t *actions) {
                const LearnArgs base{(float *)h->d_learn_q, (int32_t *)h->d_learn_carry, actions, h->learn_seed, h->learn_E,
                                     h->learn_alpha, h->learn_gamma, h->learn_algo, k0 > 0 ? 1 : 0, k0 + kc < io.K ? 1 : 0};
                if constexpr (PE) return LearnArgsPE{base, (const float *)h->d_learn_alpha, (const float *)h->d_learn_gamma, (const uint32_t *)h->d_learn_E};
                else return base;
            });
        }, qlds);
    }, a.philox != 0, a.has_p_noise || a.has_r_noise, a.unit_rewards != 0);
    return rc;
}

#if MDPP_LEARN_TU_NLEV
// ... of the per-env noise-level form: the PE parameters and the levels
struct LearnArgsNL : LearnArgsPE {
    NoiseLevelArgs nl;
};

template <bool PHILOX, bool UNIT, bool QLDS, bool DOUBLE>
__global__ __launch_bounds__(kBlock) void k_discrete_learn_rollout_nlev(DiscreteArgs a, LearnArgsNL p, int K, void *__restrict__ obs,
                                                                        float *__restrict__ reward, uint8_t *__restrict__ term,
                                                                        uint8_t *__restrict__ trunc) {
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ uint64_t s_ki[256];                      // numpy's ziggurat tables (kZigLdsBytes)
    __shared__ double s_wi[256], s_fi[256];
    zig_stage(s_ki, s_wi, s_fi, threadIdx.x, kBlock);
    LearnAgent<QLDS, true, DOUBLE> agent{p, (float *)(lds + a.lds_bytes + p.nl.lds_bytes) + threadIdx.x, (uint32_t)a.A, (uint32_t)a.S * (uint32_t)a.A, (uint32_t)a.N};
    closed_loop_rollout<PHILOX, true, UNIT, false, true>(a, K, !a.obs_i32, p.actions, obs, reward, term, trunc, lds, ZigLds{s_ki, s_wi, s_fi}, agent,
                                                         EpisodeSummaryArgs{}, p.nl);
}

template <bool PHILOX, bool UNIT, bool QLDS, bool DOUBLE>
__global__ __launch_bounds__(kBlock) void k_discrete_learn_summary_nlev(DiscreteArgs a, LearnArgsNL p, int K, EpisodeSummaryArgs sm) {
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ uint64_t s_ki[256];
    __shared__ double s_wi[256], s_fi[256];
    zig_stage(s_ki, s_wi, s_fi, threadIdx.x, kBlock);
    LearnAgent<QLDS, true, DOUBLE> agent{p, (float *)(lds + a.lds_bytes + p.nl.lds_bytes) + threadIdx.x, (uint32_t)a.A, (uint32_t)a.S * (uint32_t)a.A, (uint32_t)a.N};
    closed_loop_rollout<PHILOX, true, UNIT, true, true>(a, K, false, nullptr, nullptr, nullptr, nullptr, nullptr, lds, ZigLds{s_ki, s_wi, s_fi}, agent, sm, p.nl);
}

template <bool SUMMARY, bool PH, bool UNIT, bool QL, bool DOUBLE>
static constexpr auto learn_kernel_nlev() {
    if constexpr (SUMMARY) return k_discrete_learn_summary_nlev<PH, UNIT, QL, DOUBLE>;
    else return k_discrete_learn_rollout_nlev<PH, UNIT, QL, DOUBLE>;
}

// K learning steps of a handle with per-env noise levels
template <bool DOUBLE, bool SUMMARY>
static int launch_learn_form_nlev(mdpp_env *h, const DiscreteIO &io) {
    const DiscreteArgs &a = h->dargs;
    const size_t q_lds = (size_t)kBlock * (size_t)a.S * (size_t)a.A * sizeof(float) * (DOUBLE ? 2u : 1u);
    int rc = MDPP_OK;
    with_bools([&](auto PH, auto UNIT) {
        // Q-tables and per-level cdfs in LDS, then the tables alone, then the cdfs alone, then neither
        bool qlds = false, clds = false;
        noise_levels_lds(h, q_lds, [&](bool q, size_t bytes) {
            return q ? dynamic_lds_ok((const void *)learn_kernel_nlev<SUMMARY, PH(), UNIT(), true, DOUBLE>(), bytes)
                     : dynamic_lds_ok((const void *)learn_kernel_nlev<SUMMARY, PH(), UNIT(), false, DOUBLE>(), bytes);
        }, qlds, clds);
        const uint32_t cdf_lds = clds ? noise_levels_cdf_lds_bytes(h) : 0u;
        with_bools([&](auto QL) {
            char name[kNameLen];
            snprintf(name, kNameLen, "%s<PHILOX=%d,NOISE=1,UNIT=%d,QLDS=%d,PE=1%s,NLEV=1>", SUMMARY ? "k_discrete_learn_summary" : "k_discrete_learn_rollout",
                     PH(), UNIT(), QL(), DOUBLE ? ",DOUBLE=1" : "");
            rc = launch_closed_loop(h, io, learn_kernel_nlev<SUMMARY, PH(), UNIT(), QL(), DOUBLE>(), (size_t)a.lds_bytes + cdf_lds + (QL() ? q_lds : 0u),
                                    qlds || clds, name, [&](int k0, int kc, int32_t *actions) {
                const LearnArgs base{(float *)h->d_learn_q, (int32_t *)h->d_learn_carry, actions, h->learn_seed, h->learn_E,
                                     h->learn_alpha, h->learn_gamma, h->learn_algo, k0 > 0 ? 1 : 0, k0 + kc < io.K ? 1 : 0};
                return LearnArgsNL{LearnArgsPE{base, (const float *)h->d_learn_alpha, (const float *)h->d_learn_gamma, (const uint32_t *)h->d_learn_E},
                                   noise_level_args(h, cdf_lds)};
            });
        }, qlds);
    }, a.philox != 0, a.unit_rewards != 0);
    return rc;
}

#if MDPP_LEARN_TU_SUMMARY && MDPP_LEARN_TU_DOUBLE
int launch_discrete_learn_double_pe_nlev_summary(mdpp_env *h, const DiscreteIO &io) { return launch_learn_form_nlev<true, true>(h, io); }
#elif MDPP_LEARN_TU_SUMMARY
int launch_discrete_learn_pe_nlev_summary(mdpp_env *h, const DiscreteIO &io) { return launch_learn_form_nlev<false, true>(h, io); }
#elif MDPP_LEARN_TU_DOUBLE
int launch_discrete_learn_double_pe_nlev(mdpp_env *h, const DiscreteIO &io) { return launch_learn_form_nlev<true, false>(h, io); }
#else
int launch_discrete_learn_pe_nlev(mdpp_env *h, const DiscreteIO &io) { return launch_learn_form_nlev<false, false>(h, io); }
#endif

#elif MDPP_LEARN_TU_SUMMARY && MDPP_LEARN_TU_PE && MDPP_LEARN_TU_DOUBLE
int launch_discrete_learn_double_pe_summary(mdpp_env *h, const DiscreteIO &io) { return launch_learn_form<true, true, true>(h, io); }
#elif MDPP_LEARN_TU_SUMMARY && MDPP_LEARN_TU_DOUBLE
int launch_discrete_learn_double_summary(mdpp_env *h, const DiscreteIO &io) { return launch_learn_form<false, true, true>(h, io); }
#elif MDPP_LEARN_TU_SUMMARY && MDPP_LEARN_TU_PE
int launch_discrete_learn_pe_summary(mdpp_env *h, const DiscreteIO &io) { return launch_learn_form<true, false, true>(h, io); }
#elif MDPP_LEARN_TU_SUMMARY
int launch_discrete_learn_summary(mdpp_env *h, const DiscreteIO &io) { return launch_learn_form<false, false, true>(h, io); }
#elif MDPP_LEARN_TU_PE && MDPP_LEARN_TU_DOUBLE
int launch_discrete_learn_double_pe(mdpp_env *h, const DiscreteIO &io) { return launch_learn_form<true, true>(h, io); }
#elif MDPP_LEARN_TU_DOUBLE
int launch_discrete_learn_double(mdpp_env *h, const DiscreteIO &io) { return launch_learn_form<false, true>(h, io); }
#elif MDPP_LEARN_TU_PE
int launch_discrete_learn_pe(mdpp_env *h, const DiscreteIO &io) { return launch_learn_form<true, false>(h, io); }
#else

// Q between the caller's [N][T S A] and the handle's [T S A][N] (T = 2 tables for double Q-learning, A then B; else 1)
template <bool TO_HANDLE>
__global__ __launch_bounds__(kBlock) void k_learn_q_transpose(float *__restrict__ handle_q, float *__restrict__ user_q, uint32_t N, uint32_t SA) {
    const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (uint64_t)N * SA) return;
    const uint32_t e = (uint32_t)(t / N), i = (uint32_t)(t - (uint64_t)e * N);
    if (TO_HANDLE) handle_q[t] = user_q[(size_t)i * SA + e];
    else user_q[(size_t)i * SA + e] = handle_q[t];
}

int launch_learn_q_copy(mdpp_env *h, float *user_q, bool to_handle, hipStream_t s) {
    const uint32_t N = (uint32_t)h->cfg.num_envs;
    const uint32_t SA = (uint32_t)h->cfg.S * (uint32_t)h->cfg.A * (h->learn_algo == MDPP_LEARN_DOUBLE_Q ? 2u : 1u);
    const uint64_t total = (uint64_t)N * SA;
    const uint64_t grid = (total + kBlock - 1) / kBlock;
    if (grid > 0x7FFFFFFFull) { h->err = "k_learn_q_transpose: table too large"; return MDPP_EUNSUPPORTED; }
    if (to_handle) hipLaunchKernelGGL(k_learn_q_transpose<true>, dim3((uint32_t)grid), dim3(kBlock), 0, s, (float *)h->d_learn_q, user_q, N, SA);
    else hipLaunchKernelGGL(k_learn_q_transpose<false>, dim3((uint32_t)grid), dim3(kBlock), 0, s, (float *)h->d_learn_q, user_q, N, SA);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { h->err = std::string("k_learn_q_transpose launch: ") + hipGetErrorString(e); return MDPP_EHIP; }
    return MDPP_OK;
}

// PE form: a parameter that is uniform travels as an array of equal entries
__global__ __launch_bounds__(kBlock) void k_learn_fill(uint32_t *__restrict__ dst, uint32_t v, uint32_t N) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < N) dst[i] = v;
}

// Why this handle has no learner, or empty: the kernel serves it
std::string discrete_learn_refusal(const mdpp_env *h) { return closed_loop_refusal(h, "learner", true, 0, "the MDP's tables"); }

// K learning steps
int launch_discrete_learn(mdpp_env *h, const DiscreteIO &io) {
    const std::string why = discrete_learn_refusal(h);
    if (!why.empty()) { h->err = "mdpp_step_n_learn: " + why; return MDPP_EUNSUPPORTED; }
    const bool dbl = h->learn_algo == MDPP_LEARN_DOUBLE_Q;
    if (h->nl_on && !h->learn_pe) {
        // per-env noise levels run the PE form: while all three parameters are uniform their arrays are filled here, and
        // again when a value has changed since (the scalar setters do not mark them while nothing is per-env)
        const bool fresh = h->nl_fill_valid && h->nl_fill_alpha == h->learn_alpha && h->nl_fill_gamma == h->learn_gamma && h->nl_fill_E == h->learn_E;
        if (!fresh && !io.name_out) {
            for (void **d : {&h->d_learn_alpha, &h->d_learn_gamma, &h->d_learn_E})
                if (!*d && hipMalloc(d, (size_t)h->cfg.num_envs * 4u) != hipSuccess) { h->err = "mdpp_step_n_learn: hipMalloc of the per-env parameter arrays failed"; return MDPP_EHIP; }
            h->learn_pe_stale = 7u;
        }
    } else {
        h->nl_fill_valid = false;
    }
    if (!h->learn_pe && !h->nl_on) {
        if (io.summary) return dbl ? launch_discrete_learn_double_summary(h, io) : launch_discrete_learn_summary(h, io);
        return dbl ? launch_discrete_learn_double(h, io) : launch_learn_form<false, false>(h, io);
    }
    if (h->learn_pe_stale && !io.name_out) {
        const uint32_t N = (uint32_t)h->cfg.num_envs, grid = (N + kBlock - 1) / kBlock;
        uint32_t abits, gbits;
        memcpy(&abits, &h->learn_alpha, 4);
        memcpy(&gbits, &h->learn_gamma, 4);
        void *const dst[3] = {h->d_learn_alpha, h->d_learn_gamma, h->d_learn_E};
        const uint32_t val[3] = {abits, gbits, h->learn_E};
        for (int b = 0; b < 3; b++)
            if (h->learn_pe_stale & (1u << b)) hipLaunchKernelGGL(k_learn_fill, dim3(grid), dim3(kBlock), 0, io.s, (uint32_t *)dst[b], val[b], N);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) { h->err = std::string("k_learn_fill launch: ") + hipGetErrorString(e); return MDPP_EHIP; }
        h->learn_pe_stale = 0;
        if (!h->learn_pe) { h->nl_fill_valid = true; h->nl_fill_alpha = h->learn_alpha; h->nl_fill_gamma = h->learn_gamma; h->nl_fill_E = h->learn_E; }
    }
    if (h->nl_on) {
        if (io.summary) return dbl ? launch_discrete_learn_double_pe_nlev_summary(h, io) : launch_discrete_learn_pe_nlev_summary(h, io);
        return dbl ? launch_discrete_learn_double_pe_nlev(h, io) : launch_discrete_learn_pe_nlev(h, io);
    }
    if (io.summary) return dbl ? launch_discrete_learn_double_pe_summary(h, io) : launch_discrete_learn_pe_summary(h, io);
    return dbl ? launch_discrete_learn_double_pe(h, io) : launch_discrete_learn_pe(h, io);
}
#endif

} // namespace mdpp
