// Greedy evaluation of the in-kernel learners' tables (mdpp_step_n_eval): K steps of "take the best action of the env's own Q,
// step" in ONE launch, the tables read and never written.  The step is closed_loop_rollout (mdpp_discrete_closed.hpp) with its
// NOISE branches; the LDS placement (closed_agent_lds) and the launcher (launch_closed_form) are there too, shared with the
// learners.  This file holds the agent, the two kernels around
// it, and EvalForm: what launch_closed_form needs to know of an evaluation form -- its kernel, its name, its argument block.
//
// Env i in state s takes
//   one table:  the lowest j maximising Q[s][j], scanned from j = 0 with a strict >
//   DOUBLE = 1: the lowest j maximising QA[s][j] + QB[s][j], one float32 addition per j
// -- the greedy branch of the learners' sel (mdpp_discrete_learn.hpp).  There is no exploration, no target, no update and no
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
// form on a handle with one MDP per env: each picks DOUBLE from the handle and calls launch_closed_form on that EvalForm.
// Each of the eight is instantiated in a translation unit of its own, so that they
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

// One form of the evaluation, as launch_closed_form (mdpp_discrete_closed.hpp) takes it
template <bool DOUBLE, bool SUMMARY_, bool NLEV_>
struct EvalForm {
    static constexpr bool SUMMARY = SUMMARY_, NLEV = NLEV_, LOG = false;     // (no episode log under evaluation: DESIGN.md 3.24)
    static constexpr int TABLES = DOUBLE ? 2 : 1;
    template <bool PH, bool NZ, bool UNIT, bool QL, int PM>
    static constexpr auto kernel() {
        if constexpr (SUMMARY) return k_discrete_eval_summary<PH, NZ, UNIT, QL, DOUBLE, NLEV, PM>;
        else return k_discrete_eval_rollout<PH, NZ, UNIT, QL, DOUBLE, NLEV, PM>;
    }
    static void name(char *out, int ph, int nz, int unit, int ql, int pm) {
        if (pm)
            snprintf(out, kNameLen, "%s<PHILOX=%d,NOISE=%d,UNIT=%d,QLDS=%d,DOUBLE=%d%s,PM=%d>", SUMMARY ? "k_discrete_eval_summary" : "k_discrete_eval_rollout",
                     ph, nz, unit, ql, DOUBLE, NLEV ? ",NLEV=1" : "", pm);
        else
            snprintf(out, kNameLen, "%s<PHILOX=%d,NOISE=%d,UNIT=%d,QLDS=%d,DOUBLE=%d%s>", SUMMARY ? "k_discrete_eval_summary" : "k_discrete_eval_rollout",
                     ph, nz, unit, ql, DOUBLE, NLEV ? ",NLEV=1" : "");
    }
    static std::conditional_t<NLEV, EvalArgsNL, EvalArgs> args(const mdpp_env *h, const DiscreteIO &, int, int, int32_t *actions, uint32_t cdf_lds) {
        const EvalArgs base{(const float *)h->d_learn_q, actions};
        if constexpr (NLEV) return EvalArgsNL{base, noise_level_args(h, cdf_lds)};
        else return base;
    }
};

// K evaluation steps of one form (NLEV: of a handle with per-env noise levels); DOUBLE, how many tables the learner keeps, is
// the handle's to say
template <bool SUMMARY, bool NLEV>
int launch_eval_form(mdpp_env *h, const DiscreteIO &io) {
    int rc = MDPP_OK;
    with_bools([&](auto DB) { rc = launch_closed_form<EvalForm<DB(), SUMMARY, NLEV>, false>(h, io); }, h->learn_algo == MDPP_LEARN_DOUBLE_Q);
    return rc;
}

// K evaluation steps of one form on a handle with one MDP per env (mdpp_learner_per_env_mdp): the PM = 1 and PM = 2 kernels;
// NLEV: with per-env noise levels (mdpp_noise_levels_per_env_mdp)
template <bool SUMMARY, bool NLEV>
int launch_eval_form_pm(mdpp_env *h, const DiscreteIO &io) {
    // (the queue of start states drawn ahead needs shared tables: the PM kernels do not carry it)
    if (h->dargs.fast_ok || h->dargs.shared_tables) { h->err = "mdpp_step_n_eval: one MDP per env: the handle has shared tables"; return MDPP_ESTATE; }
    int rc = MDPP_OK;
    with_bools([&](auto DB) { rc = launch_closed_form<EvalForm<DB(), SUMMARY, NLEV>, true>(h, io); }, h->learn_algo == MDPP_LEARN_DOUBLE_Q);
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
