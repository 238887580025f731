// In-kernel tabular TD learners on GRID envs: one Q-learning or SARSA agent per gridworld, its Q-table beside the env state, K
// steps of "select epsilon-greedily from the env's own Q, step, update that Q" in ONE launch (mdpp_step_n_grid_learn), greedy
// evaluation of those tables (mdpp_step_n_grid_eval) and the forms of both that keep episode summaries instead of [K][N]
// arrays.  include/mdpp.h "Grid learners" is the normative text.
//
// The step is a COPY of the G = 2 path of k_grid_step (mdpp_grid.hip: transition-noise re-draw, clip, target latch, dense /
// sparse reward, every-n mask, reward noise, scale, shift, terminal reward, truncation, the three reset modes), so that the
// open-loop kernels' code objects do not change.  The admission test is gone: the agent's vectors are one-hot or zero by
// construction.  The agent's hooks sit around it like mdpp_discrete_closed.hpp's: select before the step, learn after it and
// before any reset.
//
// The learner of env i (global id g = env_id_offset + i): alpha[i], gamma[i], E[i] = ceil(epsilon[i] 2^31) -- always [N] arrays,
// loaded once per launch -- and Q float32 [S][A], S = (g0 + 1)(g1 + 1), A = 4 or 5.  State index s = c0 (g1 + 1) + c1 (a start
// cell may be the index g, one past the grid).  Action j -> vector: j < 4: component j >> 1 is +1 (j even) or -1 (j odd);
// j == 4: the noop.  sel, target, update and sarsa's carry: mdpp_discrete_learn.hpp's, restated here on this table.
//
// Q lives in a buffer of the handle, entry-major [S A][N]: entry e = s A + j of env i at q[e N + i] (coalesced over lanes).
// QLDS = 1: the lane's table is staged once per launch at q_lds[e 256 + tid] (bank = lane: no conflict whatever entry each
// lane holds) and, unless EVAL, written back after the last step; QLDS = 0: the same indexing on the buffer.  The host
// guarantees N S A 4 < 2^32, so e N + i fits 32 bits.
//
// NOISE = 0 leaves the env's noise streams and numpy's ziggurat out of the kernel; EVAL = 1 leaves the learner's Philox words,
// the parameters and the update out; SUMMARY = 1 writes no [K][N] array and keeps the caller's five [N] episode numbers.
//
// SCHED = 1 (mdpp_set_grid_learner_schedule; include/mdpp.h "Grid learner schedules and the episode log"): E and / or alpha come
// from a table [R][M] at (row[i], min(ep[i], M - 1)) -- looked up at the launch's start and again after the update of every
// step that ends an episode, one plain global dword load per scheduled table (the tables are small and L2-resident); the lane
// keeps row[i] M and ep[i] in two registers and stores ep[i] after the last step.  LOG = 1 (mdpp_step_n_grid_learn_log): the
// summary form also writes the finished episode's return and length to row log_count[i] of the caller's episode-major
// [M][N] arrays, while there is one.  Both are forms of the learner only (EVAL = 0), LOG of the summary form only.
// The step loop is ONE text, mdpp_grid_learn_body.inc, included into three kernels: k_grid_learn_rollout (SCHED = LOG = 0: the
// symbols and the code this kernel always had), k_grid_learn_sched_rollout and k_grid_learn_log_rollout.
//
// NLEV = 1 (mdpp_set_grid_noise_levels; include/mdpp.h "Grid noise levels"): the lane steps with its OWN transition_noise and
// reward_noise, two float64 [N] arrays of the handle loaded once per launch and kept in registers, in place of GridArgs::p_noise
// and r_noise -- a lane at p == 0 draws no u, as a handle created without the key does.  Three more kernels include the body
// with NLEV = true and NOISE = true (levels exist only on handles with a noise key): k_grid_learn_nlev_rollout,
// k_grid_learn_nlev_sched_rollout and k_grid_learn_nlev_log_rollout.  The three above keep their symbols and their code.
#pragma once
#include "mdpp_internal.hpp"
#include "mdpp_rng.hpp"

namespace mdpp {

// what the kernel takes besides the handle's GridArgs
struct GridLearnArgs {
    float *q;                   // [S A][N] entry-major (device)
    const float *alpha, *gamma; // [N]
    const uint32_t *E;          // [N] ceil(epsilon 2^31): explore iff (wE >> 1) < E
    int32_t *actions;           // [K][N][2] the action vectors taken (out; unused by the summary form)
    uint64_t seed;              // key of the learner's Philox streams
    int32_t algo;               // MDPP_LEARN_Q_LEARNING / MDPP_LEARN_SARSA
    uint32_t A, SA, W;          // actions; entries per table; g1 + 1
};

// ... of the scheduled forms: the per-episode tables [R][M] (device; a NULL table: that parameter is not scheduled and the
// lane keeps its own), the envs' rows and episode counters [N]
struct GridSchedArgs {
    const uint32_t *sc_E;
    const float *sc_alpha;
    const int32_t *sc_row;
    int32_t *sc_ep;
    int32_t M;
};

// ... of the NLEV forms: every env's transition_noise and reward_noise, float64 [N] (device; both always filled)
struct GridNoiseArgs {
    const double *p_noise, *r_noise;
};

template <bool PHILOX, bool NOISE, bool QLDS, bool EVAL, bool SUMMARY>
__global__ __launch_bounds__(kBlock) void k_grid_learn_rollout(GridArgs a, GridLearnArgs p, int K, void *__restrict__ obs,
                                                               float *__restrict__ reward, uint8_t *__restrict__ term,
                                                               uint8_t *__restrict__ trunc, EpisodeSummaryArgs sm) {
    constexpr bool SCHED = false, LOG = false, NLEV = false;
    const GridSchedArgs sc{};       // (never read)
    const GridNoiseArgs nl{};       // (never read)
#include "mdpp_grid_learn_body.inc"
}

// ... with a schedule in force (SCHED = 1), full output or summary
template <bool PHILOX, bool NOISE, bool QLDS, bool SUMMARY>
__global__ __launch_bounds__(kBlock) void k_grid_learn_sched_rollout(GridArgs a, GridLearnArgs p, GridSchedArgs sc, int K, void *__restrict__ obs,
                                                                     float *__restrict__ reward, uint8_t *__restrict__ term,
                                                                     uint8_t *__restrict__ trunc, EpisodeSummaryArgs sm) {
    constexpr bool EVAL = false, SCHED = true, LOG = false, NLEV = false;
    const GridNoiseArgs nl{};       // (never read)
#include "mdpp_grid_learn_body.inc"
}

// ... keeping an episode log beside the summary (LOG = 1), with or without a schedule (SCHED = 0: sc is not read)
template <bool PHILOX, bool NOISE, bool QLDS, bool SCHED>
__global__ __launch_bounds__(kBlock) void k_grid_learn_log_rollout(GridArgs a, GridLearnArgs p, GridSchedArgs sc, int K, EpisodeSummaryArgs sm) {
    constexpr bool EVAL = false, SUMMARY = true, LOG = true, NLEV = false;
    const GridNoiseArgs nl{};       // (never read)
    void *const obs = nullptr;      // (the summary form writes no [K][N] array)
    float *const reward = nullptr;
    uint8_t *const term = nullptr, *const trunc = nullptr;
#include "mdpp_grid_learn_body.inc"
}

// ... with per-env noise levels (NLEV = 1; NOISE = 1: levels exist only on handles with a noise key): the learner or evaluation,
// full output or summary
template <bool PHILOX, bool QLDS, bool EVAL, bool SUMMARY>
__global__ __launch_bounds__(kBlock) void k_grid_learn_nlev_rollout(GridArgs a, GridLearnArgs p, GridNoiseArgs nl, int K, void *__restrict__ obs,
                                                                    float *__restrict__ reward, uint8_t *__restrict__ term,
                                                                    uint8_t *__restrict__ trunc, EpisodeSummaryArgs sm) {
    constexpr bool NOISE = true, SCHED = false, LOG = false, NLEV = true;
    const GridSchedArgs sc{};       // (never read)
#include "mdpp_grid_learn_body.inc"
}

// ... under a schedule too
template <bool PHILOX, bool QLDS, bool SUMMARY>
__global__ __launch_bounds__(kBlock) void k_grid_learn_nlev_sched_rollout(GridArgs a, GridLearnArgs p, GridSchedArgs sc, GridNoiseArgs nl, int K,
                                                                          void *__restrict__ obs, float *__restrict__ reward,
                                                                          uint8_t *__restrict__ term, uint8_t *__restrict__ trunc,
                                                                          EpisodeSummaryArgs sm) {
    constexpr bool NOISE = true, EVAL = false, SCHED = true, LOG = false, NLEV = true;
#include "mdpp_grid_learn_body.inc"
}

// ... keeping an episode log (SCHED = 0: sc is not read)
template <bool PHILOX, bool QLDS, bool SCHED>
__global__ __launch_bounds__(kBlock) void k_grid_learn_nlev_log_rollout(GridArgs a, GridLearnArgs p, GridSchedArgs sc, GridNoiseArgs nl, int K,
                                                                        EpisodeSummaryArgs sm) {
    constexpr bool NOISE = true, EVAL = false, SUMMARY = true, LOG = true, NLEV = true;
    void *const obs = nullptr;      // (the summary form writes no [K][N] array)
    float *const reward = nullptr;
    uint8_t *const term = nullptr, *const trunc = nullptr;
#include "mdpp_grid_learn_body.inc"
}

// K steps of one form of the learner or (eval; SCHED = LOG = 0 only) of greedy evaluation.  SUMMARY: io.summary's five arrays
// instead of the [K][N] ones; SCHED: the handle's schedule is in force; LOG: io.summary carries an episode log; NLEV: the
// handle's per-env noise levels are in force.  A dry run (io.name_out) writes the kernel's name and launches nothing -- the
// name is the form's: k_grid_learn_rollout<...> with ",NLEV=1" for the kernels that read the levels and then ",SCHED=1" for
// the scheduled ones, and a log launch's is that of the launch without a log.  QLDS where the device grants the workgroup's
// tables beside the static LDS of the kernel launched and MDPP_OPT_NO_GRID_QLDS does not forbid it
template <bool SUMMARY, bool SCHED = false, bool LOG = false, bool NLEV = false>
int launch_grid_learn_form(mdpp_env *h, const DiscreteIO &io, bool eval) {
    static_assert(SUMMARY || !LOG, "the episode log is kept by the summary form");
    GridArgs a = h->gargs;
    stamp_step(a, h);
    const uint32_t S = (uint32_t)(a.shape[0] + 1) * (uint32_t)(a.shape[1] + 1), A = (uint32_t)h->gl_A;
    const GridLearnArgs p{(float *)h->d_gl_q, (const float *)h->d_gl_alpha, (const float *)h->d_gl_gamma, (const uint32_t *)h->d_gl_E,
                          const_cast<int32_t *>(io.actions), h->gl_seed, h->gl_algo, A, S * A, (uint32_t)(a.shape[1] + 1)};
    const int grid = (a.N + kBlock - 1) / kBlock;
    const size_t q_bytes = (size_t)kBlock * S * A * sizeof(float);
    const bool noise = a.has_p_noise != 0 || a.has_r_noise != 0;
    const EpisodeSummaryArgs sm = SUMMARY ? *io.summary : EpisodeSummaryArgs{};
    const bool no_qlds = (a.opts & MDPP_OPT_NO_GRID_QLDS) != 0;
    if ((SCHED || LOG) && eval) { h->err = "launch_grid_learn_form: evaluation has no SCHED or LOG form"; return MDPP_EINVAL; }
    const GridSchedArgs sc = SCHED ? GridSchedArgs{h->gl_sched_eps ? (const uint32_t *)h->d_gl_sched_E : nullptr,
                                                   h->gl_sched_alpha ? (const float *)h->d_gl_sched_alpha : nullptr,
                                                   (const int32_t *)h->d_gl_sched_row, (int32_t *)h->d_gl_sched_ep, h->gl_sched_M}
                                   : GridSchedArgs{};
    const char *kernel;
    if constexpr (NLEV) {
        if (!noise || !h->d_gl_nl_p || !h->d_gl_nl_r) { h->err = "launch_grid_learn_form: noise levels on a handle without a noise key"; return MDPP_EINVAL; }
        const GridNoiseArgs nl{(const double *)h->d_gl_nl_p, (const double *)h->d_gl_nl_r};
        if constexpr (SCHED || LOG) {
            kernel = LOG ? "k_grid_learn_nlev_log_rollout" : "k_grid_learn_nlev_sched_rollout";
            with_bools([&](auto PH) {
                bool ql;
                if constexpr (LOG) ql = !no_qlds && dynamic_lds_ok((const void *)k_grid_learn_nlev_log_rollout<PH(), true, SCHED>, q_bytes);
                else ql = !no_qlds && dynamic_lds_ok((const void *)k_grid_learn_nlev_sched_rollout<PH(), true, SUMMARY>, q_bytes);
                with_bools([&](auto QL) {
                    if (io.name_out)
                        snprintf(io.name_out, kNameLen, "k_grid_learn_rollout<PHILOX=%d,NOISE=1,QLDS=%d,EVAL=0,SUMMARY=%d,NLEV=1%s>", PH(), QL(),
                                 SUMMARY ? 1 : 0, SCHED ? ",SCHED=1" : "");
                    else if constexpr (LOG)
                        hipLaunchKernelGGL((k_grid_learn_nlev_log_rollout<PH(), QL(), SCHED>), dim3(grid), dim3(kBlock), QL() ? q_bytes : 0, io.s,
                                           a, p, sc, nl, io.K, sm);
                    else
                        hipLaunchKernelGGL((k_grid_learn_nlev_sched_rollout<PH(), QL(), SUMMARY>), dim3(grid), dim3(kBlock), QL() ? q_bytes : 0, io.s,
                                           a, p, sc, nl, io.K, io.obs, io.reward, io.term, io.trunc, sm);
                }, ql);
            }, a.philox != 0);
        } else {
            kernel = "k_grid_learn_nlev_rollout";
            with_bools([&](auto PH, auto EV) {
                const bool ql = !no_qlds && dynamic_lds_ok((const void *)k_grid_learn_nlev_rollout<PH(), true, EV(), SUMMARY>, q_bytes);
                with_bools([&](auto QL) {
                    if (io.name_out)
                        snprintf(io.name_out, kNameLen, "k_grid_learn_rollout<PHILOX=%d,NOISE=1,QLDS=%d,EVAL=%d,SUMMARY=%d,NLEV=1>", PH(), QL(), EV(),
                                 SUMMARY ? 1 : 0);
                    else
                        hipLaunchKernelGGL((k_grid_learn_nlev_rollout<PH(), QL(), EV(), SUMMARY>), dim3(grid), dim3(kBlock), QL() ? q_bytes : 0, io.s,
                                           a, p, nl, io.K, io.obs, io.reward, io.term, io.trunc, sm);
                }, ql);
            }, a.philox != 0, eval);
        }
    } else if constexpr (SCHED || LOG) {
        kernel = LOG ? "k_grid_learn_log_rollout" : "k_grid_learn_sched_rollout";
        with_bools([&](auto PH, auto NZ) {
            bool ql;
            if constexpr (LOG) ql = !no_qlds && dynamic_lds_ok((const void *)k_grid_learn_log_rollout<PH(), NZ(), true, SCHED>, q_bytes);
            else ql = !no_qlds && dynamic_lds_ok((const void *)k_grid_learn_sched_rollout<PH(), NZ(), true, SUMMARY>, q_bytes);
            with_bools([&](auto QL) {
                if (io.name_out)
                    snprintf(io.name_out, kNameLen, "k_grid_learn_rollout<PHILOX=%d,NOISE=%d,QLDS=%d,EVAL=0,SUMMARY=%d%s>", PH(), NZ(), QL(),
                             SUMMARY ? 1 : 0, SCHED ? ",SCHED=1" : "");
                else if constexpr (LOG)
                    hipLaunchKernelGGL((k_grid_learn_log_rollout<PH(), NZ(), QL(), SCHED>), dim3(grid), dim3(kBlock), QL() ? q_bytes : 0, io.s,
                                       a, p, sc, io.K, sm);
                else
                    hipLaunchKernelGGL((k_grid_learn_sched_rollout<PH(), NZ(), QL(), SUMMARY>), dim3(grid), dim3(kBlock), QL() ? q_bytes : 0, io.s,
                                       a, p, sc, io.K, io.obs, io.reward, io.term, io.trunc, sm);
            }, ql);
        }, a.philox != 0, noise);
    } else {
        kernel = "k_grid_learn_rollout";
        with_bools([&](auto PH, auto NZ, auto EV) {
            const bool ql = !no_qlds && dynamic_lds_ok((const void *)k_grid_learn_rollout<PH(), NZ(), true, EV(), SUMMARY>, q_bytes);
            with_bools([&](auto QL) {
                if (io.name_out)
                    snprintf(io.name_out, kNameLen, "k_grid_learn_rollout<PHILOX=%d,NOISE=%d,QLDS=%d,EVAL=%d,SUMMARY=%d>", PH(), NZ(), QL(), EV(), SUMMARY ? 1 : 0);
                else
                    hipLaunchKernelGGL((k_grid_learn_rollout<PH(), NZ(), QL(), EV(), SUMMARY>), dim3(grid), dim3(kBlock), QL() ? q_bytes : 0, io.s,
                                       a, p, io.K, io.obs, io.reward, io.term, io.trunc, sm);
            }, ql);
        }, a.philox != 0, noise, eval);
    }
    return io.name_out ? MDPP_OK : step_done(h, io.K, kernel);
}
extern template int launch_grid_learn_form<false>(mdpp_env *, const DiscreteIO &, bool);                // mdpp_grid_learn.hip
extern template int launch_grid_learn_form<true>(mdpp_env *, const DiscreteIO &, bool);                 // mdpp_grid_summary_learn.hip
extern template int launch_grid_learn_form<false, true>(mdpp_env *, const DiscreteIO &, bool);          // mdpp_grid_sched_learn.hip
extern template int launch_grid_learn_form<true, true>(mdpp_env *, const DiscreteIO &, bool);           // mdpp_grid_summary_sched_learn.hip
extern template int launch_grid_learn_form<true, false, true>(mdpp_env *, const DiscreteIO &, bool);    // mdpp_grid_episodes_learn.hip
extern template int launch_grid_learn_form<true, true, true>(mdpp_env *, const DiscreteIO &, bool);     // mdpp_grid_episodes_sched_learn.hip
extern template int launch_grid_learn_form<false, false, false, true>(mdpp_env *, const DiscreteIO &, bool);   // mdpp_grid_levels_learn.hip
extern template int launch_grid_learn_form<true, false, false, true>(mdpp_env *, const DiscreteIO &, bool);    // mdpp_grid_summary_levels_learn.hip
extern template int launch_grid_learn_form<false, true, false, true>(mdpp_env *, const DiscreteIO &, bool);    // mdpp_grid_levels_sched_learn.hip
extern template int launch_grid_learn_form<true, true, false, true>(mdpp_env *, const DiscreteIO &, bool);     // mdpp_grid_summary_levels_sched_learn.hip
extern template int launch_grid_learn_form<true, false, true, true>(mdpp_env *, const DiscreteIO &, bool);     // mdpp_grid_episodes_levels_learn.hip
extern template int launch_grid_learn_form<true, true, true, true>(mdpp_env *, const DiscreteIO &, bool);      // mdpp_grid_episodes_levels_sched_learn.hip

} // namespace mdpp
