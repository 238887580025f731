// Greedy evaluation of the in-kernel learners' tables (mdpp_step_n_eval): K steps of "take the best action of the env's own Q,
// step" in ONE launch, the tables read and never written.  The step is closed_loop_rollout (mdpp_discrete_closed.hpp) with its
// NOISE branches; this file holds the agent, the kernels and the launcher of every form.
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
// Two kernels: k_discrete_eval_rollout, and k_discrete_eval_summary (mdpp_step_n_eval_summary) around the SUMMARY form of the
// step.  NLEV = 1 (per-env noise levels, mdpp_set_noise_levels) is the same agent around the NLEV form of the step, NOISE = 1
// always; the per-level cdfs, when staged, lie between the MDP's tables and the Q-tables in LDS.
//
// PM = 1 / 2 (one MDP per env, mdpp_learner_per_env_mdp) is the same agent around the PM form of the step; the Q-tables lie
// behind the envs' MDP slots and the shared noise cdf in LDS (closed_agent_lds_offset) -- with NLEV = 1
// (mdpp_noise_levels_per_env_mdp) behind the per-level cdfs, which take the shared cdf's place.
//
// launch_eval_form<SUMMARY, NLEV> launches one form, launch_eval_form_pm<SUMMARY, NLEV> the PM = 1 and PM = 2 kernels of one
// form on a handle with one MDP per env.  Each of the eight is instantiated in a translation unit of its own, so that they
// compile in parallel: mdpp_discrete_eval.hip holds the plain rollout form and the dispatcher,
// mdpp_discrete_eval_{summary,nlev,nlev_summary,pm,pm_summary,pm_nlev,pm_nlev_summary}.hip one explicit instantiation each;
// every other unit sees the `extern template` below.
#pragma once
#include "mdpp_discrete_closed.hpp"

namespace mdpp {

// what the kernel takes besides the handle's DiscreteArgs
struct EvalArgs {
    const float *q;             // [T S A][N] entry-major (device)
    int32_t *actions;           // [K][N] the actions taken (out; unused by the summary kernel)
};
// ... of the per-env noise-level form
struct EvalArgsNL : EvalArgs {
    NoiseLevelArgs nl;
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
    __device__ __forceinline__ void episode_end(bool) {}
    __device__ __forceinline__ void finish(uint32_t) {}
};

template <bool PHILOX, bool NOISE, bool UNIT, bool QLDS, bool DOUBLE, bool NLEV = false, int PM = 0>
__global__ __launch_bounds__(kBlock) void k_discrete_eval_rollout(DiscreteArgs a, std::conditional_t<NLEV, EvalArgsNL, EvalArgs> p, int K,
                                                                  void *__restrict__ obs,
                                                                  float *__restrict__ reward,
                                                                  uint8_t *__restrict__ term,
                                                                  uint8_t *__restrict__ trunc) {
    static_assert(!NLEV || NOISE, "per-env noise levels are levels of a NOISE step");
    extern __shared__ __align__(16) unsigned char lds[];
    const ZigLds zig = closed_loop_zig_lds<NOISE>();
    unsigned char *q_lds;                                           // the agent's LDS: behind the MDP's tables and the per-level cdfs
    if constexpr (NLEV && PM != 0) q_lds = lds + closed_agent_lds_offset<PM>(a, p.nl.lds_bytes);
    else {
        q_lds = lds + closed_agent_lds_offset<PM>(a);
        if constexpr (NLEV) q_lds += p.nl.lds_bytes;
    }
    EvalAgent<QLDS, DOUBLE> agent{p, (float *)q_lds + threadIdx.x, (uint32_t)a.A, (uint32_t)a.S * (uint32_t)a.A, (uint32_t)a.N};
    if constexpr (NLEV) closed_loop_rollout<PHILOX, NOISE, UNIT, false, NLEV, PM>(a, K, !a.obs_i32, p.actions, obs, reward, term, trunc, lds, zig, agent, EpisodeSummaryArgs{}, p.nl);
    else if constexpr (PM != 0) closed_loop_rollout<PHILOX, NOISE, UNIT, false, false, PM>(a, K, !a.obs_i32, p.actions, obs, reward, term, trunc, lds, zig, agent);
    else closed_loop_rollout<PHILOX, NOISE, UNIT>(a, K, !a.obs_i32, p.actions, obs, reward, term, trunc, lds, zig, agent);
}

// ... keeping episode summaries instead of writing the [K][N] arrays
template <bool PHILOX, bool NOISE, bool UNIT, bool QLDS, bool DOUBLE, bool NLEV = false, int PM = 0>
__global__ __launch_bounds__(kBlock) void k_discrete_eval_summary(DiscreteArgs a, std::conditional_t<NLEV, EvalArgsNL, EvalArgs> p, int K, EpisodeSummaryArgs sm) {
    static_assert(!NLEV || NOISE, "per-env noise levels are levels of a NOISE step");
    extern __shared__ __align__(16) unsigned char lds[];
    const ZigLds zig = closed_loop_zig_lds<NOISE>();
    unsigned char *q_lds;                                           // the agent's LDS: behind the MDP's tables and the per-level cdfs
    if constexpr (NLEV && PM != 0) q_lds = lds + closed_agent_lds_offset<PM>(a, p.nl.lds_bytes);
    else {
        q_lds = lds + closed_agent_lds_offset<PM>(a);
        if constexpr (NLEV) q_lds += p.nl.lds_bytes;
    }
    EvalAgent<QLDS, DOUBLE> agent{p, (float *)q_lds + threadIdx.x, (uint32_t)a.A, (uint32_t)a.S * (uint32_t)a.A, (uint32_t)a.N};
    if constexpr (NLEV) closed_loop_rollout<PHILOX, NOISE, UNIT, true, NLEV, PM>(a, K, false, nullptr, nullptr, nullptr, nullptr, nullptr, lds, zig, agent, sm, p.nl);
    else if constexpr (PM != 0) closed_loop_rollout<PHILOX, NOISE, UNIT, true, false, PM>(a, K, false, nullptr, nullptr, nullptr, nullptr, nullptr, lds, zig, agent, sm);
    else closed_loop_rollout<PHILOX, NOISE, UNIT, true>(a, K, false, nullptr, nullptr, nullptr, nullptr, nullptr, lds, zig, agent, sm);
}

template <bool SUMMARY, bool PH, bool NZ, bool UNIT, bool QL, bool DOUBLE, bool NLEV, int PM = 0>
constexpr auto eval_kernel() {
    if constexpr (SUMMARY) return k_discrete_eval_summary<PH, NZ, UNIT, QL, DOUBLE, NLEV, PM>;
    else return k_discrete_eval_rollout<PH, NZ, UNIT, QL, DOUBLE, NLEV, PM>;
}

// K evaluation steps of one form (NLEV: of a handle with per-env noise levels -- NOISE = 1 whatever its keys)
template <bool SUMMARY, bool NLEV>
int launch_eval_form(mdpp_env *h, const DiscreteIO &io) {
    const DiscreteArgs &a = h->dargs;
    const bool dbl = h->learn_algo == MDPP_LEARN_DOUBLE_Q;
    const size_t q_lds = (size_t)kBlock * (size_t)a.S * (size_t)a.A * sizeof(float) * (dbl ? 2u : 1u);
    int rc = MDPP_OK;
    with_bools([&](auto PH, auto NZ, auto UNIT, auto DB) {
        if constexpr (!NLEV || NZ()) {
            // the LDS forms when a workgroup's 256 tables (and the per-level cdfs) fit beside the MDP's (and the device grants it),
            // as for the learners
            bool qlds = false, clds = false;
            closed_agent_lds(h, q_lds, [&](bool q, size_t bytes) {
                return q ? dynamic_lds_ok((const void *)eval_kernel<SUMMARY, PH(), NZ(), UNIT(), true, DB(), NLEV>(), bytes)
                         : dynamic_lds_ok((const void *)eval_kernel<SUMMARY, PH(), NZ(), UNIT(), false, DB(), NLEV>(), bytes);
            }, qlds, clds);
            const uint32_t cdf_lds = clds ? noise_levels_cdf_lds_bytes(h) : 0u;
            with_bools([&](auto QL) {
                char name[kNameLen];
                snprintf(name, kNameLen, "%s<PHILOX=%d,NOISE=%d,UNIT=%d,QLDS=%d,DOUBLE=%d%s>", SUMMARY ? "k_discrete_eval_summary" : "k_discrete_eval_rollout",
                         PH(), NZ(), UNIT(), QL(), DB(), NLEV ? ",NLEV=1" : "");
                rc = launch_closed_loop<SUMMARY>(h, io, eval_kernel<SUMMARY, PH(), NZ(), UNIT(), QL(), DB(), NLEV>(),
                                                 (size_t)a.lds_bytes + cdf_lds + (QL() ? q_lds : 0u), qlds || clds, name, [&](int, int, int32_t *actions) {
                    const EvalArgs base{(const float *)h->d_learn_q, actions};
                    if constexpr (NLEV) return EvalArgsNL{base, noise_level_args(h, cdf_lds)};
                    else return base;
                });
            }, qlds);
        }
    }, a.philox != 0, NLEV || a.has_p_noise || a.has_r_noise, a.unit_rewards != 0, dbl);
    return rc;
}

// K evaluation steps of one form on a handle with one MDP per env (mdpp_learner_per_env_mdp): the PM = 1 and PM = 2 kernels;
// NLEV: with per-env noise levels (mdpp_noise_levels_per_env_mdp)
template <bool SUMMARY, bool NLEV>
int launch_eval_form_pm(mdpp_env *h, const DiscreteIO &io) {
    const DiscreteArgs &a = h->dargs;
    const bool dbl = h->learn_algo == MDPP_LEARN_DOUBLE_Q;
    const size_t q_lds = (size_t)kBlock * (size_t)a.S * (size_t)a.A * sizeof(float) * (dbl ? 2u : 1u);
    int rc = MDPP_OK;
    // (the queue of start states drawn ahead needs shared tables: the PM kernels do not carry it)
    if (a.fast_ok || a.shared_tables) { h->err = "mdpp_step_n_eval: one MDP per env: the handle has shared tables"; return MDPP_ESTATE; }
    with_bools([&](auto PH, auto NZ, auto UNIT, auto DB) {
        if constexpr (!NLEV || NZ()) {
            // the placement, as for the learners
            bool qlds = false, mlds = false, clds = false;
            if constexpr (NLEV)
                closed_agent_lds_pm_nlev(h, q_lds, [&](bool q, bool m, bool, size_t bytes) {
                    const void *k = nullptr;
                    with_bools([&](auto QL, auto ML) { k = (const void *)eval_kernel<SUMMARY, PH(), NZ(), UNIT(), QL(), DB(), true, ML() ? 2 : 1>(); }, q, m);
                    return dynamic_lds_ok(k, bytes);
                }, qlds, mlds, clds);
            else
                closed_agent_lds_pm(h, q_lds, [&](bool q, bool m, size_t bytes) {
                    const void *k = nullptr;
                    with_bools([&](auto QL, auto ML) { k = (const void *)eval_kernel<SUMMARY, PH(), NZ(), UNIT(), QL(), DB(), false, ML() ? 2 : 1>(); }, q, m);
                    return dynamic_lds_ok(k, bytes);
                }, qlds, mlds);
            const uint32_t cdf_lds = clds ? noise_levels_cdf_lds_bytes(h) : 0u;
            with_bools([&](auto QL, auto ML) {
                constexpr int PM = ML() ? 2 : 1;
                char name[kNameLen];
                snprintf(name, kNameLen, "%s<PHILOX=%d,NOISE=%d,UNIT=%d,QLDS=%d,DOUBLE=%d%s,PM=%d>", SUMMARY ? "k_discrete_eval_summary" : "k_discrete_eval_rollout",
                         PH(), NZ(), UNIT(), QL(), DB(), NLEV ? ",NLEV=1" : "", PM);
                const size_t agent_at = NLEV ? (size_t)closed_agent_lds_offset<PM>(a, cdf_lds) : (size_t)closed_agent_lds_offset<PM>(a);
                rc = launch_closed_loop<SUMMARY>(h, io, eval_kernel<SUMMARY, PH(), NZ(), UNIT(), QL(), DB(), NLEV, PM>(),
                                                 agent_at + (QL() ? q_lds : 0u), true, name, [&](int, int, int32_t *actions) {
                    const EvalArgs base{(const float *)h->d_learn_q, actions};
                    if constexpr (NLEV) return EvalArgsNL{base, noise_level_args(h, cdf_lds)};
                    else return base;
                });
            }, qlds, mlds);
        }
    }, a.philox != 0, NLEV || a.has_p_noise || a.has_r_noise, a.unit_rewards != 0, dbl);
    return rc;
}

// the forms built <SUMMARY, NLEV> and, with one MDP per env, <SUMMARY, NLEV>, each defined (an explicit instantiation) in the
// translation unit named
extern template int launch_eval_form<false, false>(mdpp_env *, const DiscreteIO &);     // mdpp_discrete_eval.hip
extern template int launch_eval_form<true, false>(mdpp_env *, const DiscreteIO &);      // mdpp_discrete_eval_summary.hip
extern template int launch_eval_form<false, true>(mdpp_env *, const DiscreteIO &);      // mdpp_discrete_eval_nlev.hip
extern template int launch_eval_form<true, true>(mdpp_env *, const DiscreteIO &);       // mdpp_discrete_eval_nlev_summary.hip
extern template int launch_eval_form_pm<false, false>(mdpp_env *, const DiscreteIO &);  // mdpp_discrete_eval_pm.hip
extern template int launch_eval_form_pm<true, false>(mdpp_env *, const DiscreteIO &);   // mdpp_discrete_eval_pm_summary.hip
extern template int launch_eval_form_pm<false, true>(mdpp_env *, const DiscreteIO &);   // mdpp_discrete_eval_pm_nlev.hip
extern template int launch_eval_form_pm<true, true>(mdpp_env *, const DiscreteIO &);    // mdpp_discrete_eval_pm_nlev_summary.hip

} // namespace mdpp
