// Greedy evaluation of the in-kernel learners' tables (mdpp_step_n_eval): K steps of "take the best action of the env's own Q,
// step" in ONE launch, the tables read and never written.  The step is closed_loop_rollout (mdpp_discrete_closed.hpp) with its
// NOISE branches; this file holds the agent.
//
// Env i in state s takes
//   one table:  the lowest j maximising Q[s][j], scanned from j = 0 with a strict >
//   DOUBLE = 1: the lowest j maximising QA[s][j] + QB[s][j], one float32 addition per j
// -- the greedy branch of the learners' sel (mdpp_discrete_learn.hip).  There is no exploration, no target, no update and no
// carry: the agent makes no Philox block (next_block is empty: no word of streams 15, 16, 17), loads no alpha, gamma or E (so
// ONE form serves uniform and per-env handles), learn() is empty.  On the reset call of a next-step-autoreset env the action
// is selected from the state in the record, written and ignored, as there.
//
// The tables are the learner's buffer, entry-major [T S A][N] (T = 2 for DOUBLE, A then B).  QLDS = 1: the lane stages its
// tables once per launch into q_lds[e 256 + tid] behind the MDP's tables (bank = lane) and every selection is LDS traffic;
// nothing is written back.  QLDS = 0 (they do not fit, or MDPP_OPT_NO_LEARN_LDS): the same indexing on the buffer.
//
// k_discrete_eval_summary (mdpp_step_n_eval_summary) is the same agent around the SUMMARY form of the step; its
// instantiations live in mdpp_discrete_eval_summary.hip (MDPP_EVAL_TU_SUMMARY), which includes this file.
//
// Per-env noise levels (mdpp_set_noise_levels): k_discrete_eval_rollout_nlev / k_discrete_eval_summary_nlev are the same agent
// around the NLEV form of the step (NOISE = 1 always), kernels of their own names in mdpp_discrete_eval_nlev.hip and
// mdpp_discrete_eval_nlev_summary.hip (MDPP_EVAL_TU_NLEV), which include this file.
#include "mdpp_discrete_closed.hpp"

#ifndef MDPP_EVAL_TU_NLEV
#define MDPP_EVAL_TU_NLEV 0        // 1: this translation unit holds the per-env noise-level kernels (of MDPP_EVAL_TU_SUMMARY's form), and nothing else
#endif
#ifndef MDPP_EVAL_TU_SUMMARY
#define MDPP_EVAL_TU_SUMMARY 0     // 1: this translation unit holds k_discrete_eval_summary's instantiations, and nothing else
#endif

namespace mdpp {

// what the kernel takes besides the handle's DiscreteArgs
struct EvalArgs {
    const float *q;             // [T S A][N] entry-major (device)
    int32_t *actions;           // [K][N] the actions taken (out; unused by the summary kernel)
};

template <bool QLDS, bool DOUBLE>
struct EvalAgent {
    const EvalArgs &p;
    float *q_lds;               // this lane's column of the workgroup's tables: entry e at q_lds[e 256]
    uint32_t A, SA, N;          // (DOUBLE: SA is ONE table's entries; B's entry e is SA + e)
    const float *qg;            // this lane's table in the buffer: entry e at qg[e N]

    __device__ __forceinline__ float qget(uint32_t e) const {
        if constexpr (QLDS) return q_lds[e * kBlock];
        else return qg[(size_t)e * N];
    }
    __device__ __forceinline__ void stage(int) {}
    __device__ __forceinline__ void begin(uint32_t i, uint64_t, uint64_t) {
        qg = p.q + i;
        if (QLDS)
            for (uint32_t e = 0; e < (DOUBLE ? 2u * SA : SA); e++) q_lds[e * kBlock] = qg[(size_t)e * N];
    }
    __device__ __forceinline__ void next_block(uint64_t, uint64_t) {}
    __device__ __forceinline__ uint32_t act(uint32_t cur, uint64_t) const {
        const uint32_t e0 = cur * A;
        float best = qget(e0);
        if constexpr (DOUBLE) best = best + qget(SA + e0);
        uint32_t bj = 0;
        for (uint32_t j = 1; j < A; j++) {
            float v = qget(e0 + j);
            if constexpr (DOUBLE) v = v + qget(SA + e0 + j);
            if (v > best) { best = v; bj = j; }
        }
        return bj;
    }
    __device__ __forceinline__ void learn(uint32_t, uint32_t, uint32_t, float, bool, bool, uint64_t) {}
    __device__ __forceinline__ void finish(uint32_t) {}
};

template <bool PHILOX, bool NOISE, bool UNIT, bool QLDS, bool DOUBLE>
__global__ __launch_bounds__(kBlock) void k_discrete_eval_rollout(DiscreteArgs a, EvalArgs p, int K, void *__restrict__ obs,
                                                                  float *__restrict__ reward, uint8_t *__restrict__ term,
                                                                  uint8_t *__restrict__ trunc) {
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ uint64_t s_ki[NOISE ? 256 : 1];          // numpy's ziggurat tables (kZigLdsBytes)
    __shared__ double s_wi[NOISE ? 256 : 1], s_fi[NOISE ? 256 : 1];
    if (NOISE) zig_stage(s_ki, s_wi, s_fi, threadIdx.x, kBlock);
    EvalAgent<QLDS, DOUBLE> agent{p, (float *)(lds + a.lds_bytes) + threadIdx.x, (uint32_t)a.A, (uint32_t)a.S * (uint32_t)a.A, (uint32_t)a.N};
    closed_loop_rollout<PHILOX, NOISE, UNIT>(a, K, !a.obs_i32, p.actions, obs, reward, term, trunc, lds, ZigLds{s_ki, s_wi, s_fi}, agent);
}

// ... keeping episode summaries instead of writing the [K][N] arrays
template <bool PHILOX, bool NOISE, bool UNIT, bool QLDS, bool DOUBLE>
__global__ __launch_bounds__(kBlock) void k_discrete_eval_summary(DiscreteArgs a, EvalArgs p, int K, EpisodeSummaryArgs sm) {
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ uint64_t s_ki[NOISE ? 256 : 1];
    __shared__ double s_wi[NOISE ? 256 : 1], s_fi[NOISE ? 256 : 1];
    if (NOISE) zig_stage(s_ki, s_wi, s_fi, threadIdx.x, kBlock);
    EvalAgent<QLDS, DOUBLE> agent{p, (float *)(lds + a.lds_bytes) + threadIdx.x, (uint32_t)a.A, (uint32_t)a.S * (uint32_t)a.A, (uint32_t)a.N};
    closed_loop_rollout<PHILOX, NOISE, UNIT, true>(a, K, false, nullptr, nullptr, nullptr, nullptr, nullptr, lds, ZigLds{s_ki, s_wi, s_fi}, agent, sm);
}

template <bool SUMMARY, bool PH, bool NZ, bool UNIT, bool QL, bool DOUBLE>
static constexpr auto eval_kernel() {
    if constexpr (SUMMARY) return k_discrete_eval_summary<PH, NZ, UNIT, QL, DOUBLE>;
    else return k_discrete_eval_rollout<PH, NZ, UNIT, QL, DOUBLE>;
}

// K evaluation steps
template <bool SUMMARY>
static int launch_eval_form(mdpp_env *h, const DiscreteIO &io) {
    const DiscreteArgs &a = h->dargs;
    const bool dbl = h->learn_algo == MDPP_LEARN_DOUBLE_Q;
    const size_t q_lds = (size_t)kBlock * (size_t)a.S * (size_t)a.A * sizeof(float) * (dbl ? 2u : 1u);
    int rc = MDPP_OK;
    with_bools([&](auto PH, auto NZ, auto UNIT, auto DB) {
        // the LDS form when a workgroup's 256 tables fit beside the MDP's (and the device grants it), as for the learners
        const bool qlds = !(h->opts & MDPP_OPT_NO_LEARN_LDS) && q_lds <= 160u * 1024u &&
                          dynamic_lds_ok((const void *)eval_kernel<SUMMARY, PH(), NZ(), UNIT(), true, DB()>(), (size_t)a.lds_bytes + q_lds);
        with_bools([&](auto QL) {
            char name[kNameLen];
            snprintf(name, kNameLen, "%s<PHILOX=%d,NOISE=%d,UNIT=%d,QLDS=%d,DOUBLE=%d>", SUMMARY ? "k_discrete_eval_summary" : "k_discrete_eval_rollout",
                     PH(), NZ(), UNIT(), QL(), DB());
            rc = launch_closed_loop(h, io, eval_kernel<SUMMARY, PH(), NZ(), UNIT(), QL(), DB()>(), (size_t)a.lds_bytes + (QL() ? q_lds : 0u), QL(), name,
                                    [&](int, int, int32_t *actions) { return EvalArgs{(const float *)h->d_learn_q, actions}; });
        }, qlds);
    }, a.philox != 0, a.has_p_noise || a.has_r_noise, a.unit_rewards != 0, dbl);
    return rc;
}

#if MDPP_EVAL_TU_NLEV
// ... of the per-env noise-level form
struct EvalArgsNL : EvalArgs {
    NoiseLevelArgs nl;
};

template <bool PHILOX, bool UNIT, bool QLDS, bool DOUBLE>
__global__ __launch_bounds__(kBlock) void k_discrete_eval_rollout_nlev(DiscreteArgs a, EvalArgsNL p, int K, void *__restrict__ obs,
                                                                       float *__restrict__ reward, uint8_t *__restrict__ term,
                                                                       uint8_t *__restrict__ trunc) {
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ uint64_t s_ki[256];                      // numpy's ziggurat tables (kZigLdsBytes)
    __shared__ double s_wi[256], s_fi[256];
    zig_stage(s_ki, s_wi, s_fi, threadIdx.x, kBlock);
    EvalAgent<QLDS, DOUBLE> agent{p, (float *)(lds + a.lds_bytes + p.nl.lds_bytes) + threadIdx.x, (uint32_t)a.A, (uint32_t)a.S * (uint32_t)a.A, (uint32_t)a.N};
    closed_loop_rollout<PHILOX, true, UNIT, false, true>(a, K, !a.obs_i32, p.actions, obs, reward, term, trunc, lds, ZigLds{s_ki, s_wi, s_fi}, agent,
                                                         EpisodeSummaryArgs{}, p.nl);
}

template <bool PHILOX, bool UNIT, bool QLDS, bool DOUBLE>
__global__ __launch_bounds__(kBlock) void k_discrete_eval_summary_nlev(DiscreteArgs a, EvalArgsNL p, int K, EpisodeSummaryArgs sm) {
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ uint64_t s_ki[256];
    __shared__ double s_wi[256], s_fi[256];
    zig_stage(s_ki, s_wi, s_fi, threadIdx.x, kBlock);
    EvalAgent<QLDS, DOUBLE> agent{p, (float *)(lds + a.lds_bytes + p.nl.lds_bytes) + threadIdx.x, (uint32_t)a.A, (uint32_t)a.S * (uint32_t)a.A, (uint32_t)a.N};
    closed_loop_rollout<PHILOX, true, UNIT, true, true>(a, K, false, nullptr, nullptr, nullptr, nullptr, nullptr, lds, ZigLds{s_ki, s_wi, s_fi}, agent, sm, p.nl);
}

template <bool SUMMARY, bool PH, bool UNIT, bool QL, bool DOUBLE>
static constexpr auto eval_kernel_nlev() {
    if constexpr (SUMMARY) return k_discrete_eval_summary_nlev<PH, UNIT, QL, DOUBLE>;
    else return k_discrete_eval_rollout_nlev<PH, UNIT, QL, DOUBLE>;
}

// K evaluation steps of a handle with per-env noise levels
template <bool SUMMARY>
static int launch_eval_form_nlev(mdpp_env *h, const DiscreteIO &io) {
    const DiscreteArgs &a = h->dargs;
    const bool dbl = h->learn_algo == MDPP_LEARN_DOUBLE_Q;
    const size_t q_lds = (size_t)kBlock * (size_t)a.S * (size_t)a.A * sizeof(float) * (dbl ? 2u : 1u);
    int rc = MDPP_OK;
    with_bools([&](auto PH, auto UNIT, auto DB) {
        bool qlds = false, clds = false;
        noise_levels_lds(h, q_lds, [&](bool q, size_t bytes) {
            return q ? dynamic_lds_ok((const void *)eval_kernel_nlev<SUMMARY, PH(), UNIT(), true, DB()>(), bytes)
                     : dynamic_lds_ok((const void *)eval_kernel_nlev<SUMMARY, PH(), UNIT(), false, DB()>(), bytes);
        }, qlds, clds);
        const uint32_t cdf_lds = clds ? noise_levels_cdf_lds_bytes(h) : 0u;
        with_bools([&](auto QL) {
            char name[kNameLen];
            snprintf(name, kNameLen, "%s<PHILOX=%d,NOISE=1,UNIT=%d,QLDS=%d,DOUBLE=%d,NLEV=1>", SUMMARY ? "k_discrete_eval_summary" : "k_discrete_eval_rollout",
                     PH(), UNIT(), QL(), DB());
            rc = launch_closed_loop(h, io, eval_kernel_nlev<SUMMARY, PH(), UNIT(), QL(), DB()>(), (size_t)a.lds_bytes + cdf_lds + (QL() ? q_lds : 0u),
                                    qlds || clds, name, [&](int, int, int32_t *actions) {
                return EvalArgsNL{EvalArgs{(const float *)h->d_learn_q, actions}, noise_level_args(h, cdf_lds)};
            });
        }, qlds);
    }, a.philox != 0, a.unit_rewards != 0, dbl);
    return rc;
}

#if MDPP_EVAL_TU_SUMMARY
int launch_discrete_eval_nlev_summary(mdpp_env *h, const DiscreteIO &io) { return launch_eval_form_nlev<true>(h, io); }
#else
int launch_discrete_eval_nlev(mdpp_env *h, const DiscreteIO &io) { return launch_eval_form_nlev<false>(h, io); }
#endif

#elif MDPP_EVAL_TU_SUMMARY
int launch_discrete_eval_summary(mdpp_env *h, const DiscreteIO &io) { return launch_eval_form<true>(h, io); }
#else

int launch_discrete_eval(mdpp_env *h, const DiscreteIO &io) {
    const std::string why = discrete_learn_refusal(h);
    if (!why.empty()) { h->err = "mdpp_step_n_eval: " + why; return MDPP_EUNSUPPORTED; }
    if (h->nl_on) return io.summary ? launch_discrete_eval_nlev_summary(h, io) : launch_discrete_eval_nlev(h, io);
    return io.summary ? launch_discrete_eval_summary(h, io) : launch_eval_form<false>(h, io);
}

// The observation an env shows is the newest state of its record: byte 0 of word 0, in every autoreset mode (after a same-step
// reset the new episode's first state; before the reset call of a next-step env the last state of the episode that ended)
__global__ __launch_bounds__(kBlock) void k_discrete_current_obs(const uint4 *__restrict__ state, void *__restrict__ obs, uint32_t N, int obs_i32) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    const uint32_t s = state[i].x & 0xFFu;
    if (obs_i32) ((int32_t *)obs)[i] = (int32_t)s;
    else ((int64_t *)obs)[i] = (int64_t)s;
}

int launch_discrete_current_obs(mdpp_env *h, void *obs, hipStream_t s) {
    const std::string why = discrete_learn_refusal(h);
    if (!why.empty()) { h->err = "mdpp_current_obs: " + why; return MDPP_EUNSUPPORTED; }
    const DiscreteArgs &a = h->dargs;
    hipLaunchKernelGGL(k_discrete_current_obs, dim3((a.N + kBlock - 1) / kBlock), dim3(kBlock), 0, s, (const uint4 *)a.state, obs, (uint32_t)a.N, (int)a.obs_i32);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { h->err = std::string("k_discrete_current_obs launch: ") + hipGetErrorString(e); return MDPP_EHIP; }
    return MDPP_OK;
}
#endif

} // namespace mdpp
