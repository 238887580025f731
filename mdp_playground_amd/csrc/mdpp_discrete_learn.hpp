// In-kernel tabular TD learners: one Q-learning or SARSA agent per env instance, its Q-table beside the env state, K steps of
// "select epsilon-greedily from the env's own Q, step, update that Q" in ONE launch (mdpp_step_n_learn).  The step itself is
// closed_loop_rollout (mdpp_discrete_closed.hpp) WITH its NOISE branches.  That header also has what the learners share with
// the greedy evaluation on the host: the LDS placement (closed_agent_lds) and the launcher (launch_closed_form).  This file
// holds the agent (LearnAgent), the two kernels around it, and LearnForm: what launch_closed_form needs to know of a learner
// form -- its kernel, its name, its argument block.
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
// PE, DOUBLE and NLEV are template parameters of the two kernels, k_discrete_learn_rollout and k_discrete_learn_summary
// (mdpp_step_n_learn_summary: the same agent around closed_loop_rollout's SUMMARY form -- the same steps, selections and
// updates, five per-env episode numbers instead of the [K][N] arrays).  NLEV = 1 (per-env noise levels,
// mdpp_set_noise_levels) is the PE learner around the step's NLEV form, NOISE = 1 always; the per-level cdfs, when staged, lie
// between the MDP's tables and the Q-tables in LDS.
//
// PM = 1 / 2 (one MDP per env, mdpp_learner_per_env_mdp) is the PE learner around the step's PM form (mdpp_discrete_closed.hpp:
// the lane's own tables in global memory / staged in LDS slots); the Q-tables lie behind the slots and the shared noise cdf
// in LDS (closed_agent_lds_offset).  The host picks PM and QLDS per launch (closed_agent_lds).  With NLEV = 1
// (mdpp_noise_levels_per_env_mdp) the per-level cdfs take the shared cdf's place.
//
// SCHED = 1 (per-episode schedules, mdpp_set_learner_schedule; with NLEV = 1 and / or PM != 0 under
// mdpp_learner_schedule_sweep: the agent below around that step, nothing else changes -- the schedule has no LDS placement
// and with levels the kernels are the overloads that take LearnArgsNLSched, the levels behind the schedule) is the PE learner with E and / or alpha looked up in a table
// by the env's own episode count: begin() loads the lane's row index and its counter ep and looks up entry min(ep, M - 1) of
// its row -- one plain global dword load per scheduled table (the tables are small, L2-resident and read only here and at
// episode ends; they have no LDS placement) -- into the registers the PE form keeps its parameters in.  closed_loop_rollout
// calls episode_end(terminated or truncated) after every step that is not a reset call, where the summary's `episodes`
// moves: the counter moves and both are looked up again, so the NEXT step selects and updates with them (sarsa's a' inside
// this step's target was selected before, under the old E).  finish() stores the counter.  The agent alone knows of the
// schedule: the step and the other agents (an empty episode_end) are the code they were.
//
// launch_learn_form<PE, DOUBLE, SUMMARY, NLEV, SCHED> launches one form, launch_learn_form_pm<DOUBLE, SUMMARY, NLEV, SCHED> the PM = 1 and PM = 2
// kernels of one form on a handle with one MDP per env: launch_closed_form on the form's LearnForm, without and with one MDP
// per env.  Each of the thirty-six forms built is instantiated in a translation
// unit of its own, so that they compile in parallel: mdpp_discrete_learn.hip holds the uniform rollout form and the
// dispatcher, mdpp_discrete_learn_*.hip one explicit instantiation each; every other unit sees the `extern template` below.
#pragma once
#include "mdpp_discrete_closed.hpp"

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
// ... of the per-env noise-level form: the PE parameters and the levels
struct LearnArgsNL : LearnArgsPE {
    NoiseLevelArgs nl;
};
// ... of the scheduled form: the PE parameters and the per-episode tables [R][M] (device; a NULL table: that parameter is not
// scheduled and the lane keeps its PE value), the envs' rows and episode counters [N]
struct LearnArgsSched : LearnArgsPE {
    const uint32_t *sc_E;
    const float *sc_alpha;
    const int32_t *sc_row;
    int32_t *sc_ep;
    int32_t M;
};
template <bool PE, bool NLEV, bool SCHED = false>
using LearnArgsOf = std::conditional_t<SCHED, LearnArgsSched, std::conditional_t<NLEV, LearnArgsNL, std::conditional_t<PE, LearnArgsPE, LearnArgs>>>;
// ... of the scheduled form on a handle with per-env noise levels: the schedule and the levels.  A struct of its own behind
// LearnArgsSched, which the agent reads through a reference to that base, and NOT a branch of LearnArgsOf: that alias is
// spelled out in the mangled name of every learner kernel, and LearnArgsNL and LearnArgsSched keep their layouts, so the
// kernels without one of the two keep their symbols and their code.  The kernels that take it are overloads of the two below.
struct LearnArgsNLSched : LearnArgsSched {
    NoiseLevelArgs nl;
};

template <bool QLDS, bool PE, bool DOUBLE, bool SCHED = false>
struct LearnAgent {
    static_assert(!SCHED || PE, "a schedule runs the PE learner");
    const std::conditional_t<SCHED, LearnArgsSched, std::conditional_t<PE, LearnArgsPE, LearnArgs>> &p;
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
    uint32_t sc_base;           // SCHED: row[i] M, where this lane's row starts in the tables
    int32_t sc_ep;              // SCHED: this lane's episode counter

    // SCHED: entry min(ep, M - 1) of the lane's row into the PE registers
    __device__ __forceinline__ void sched_lookup() {
        if constexpr (SCHED) {
            // (compared unsigned: a negative counter, which only mdpp_set_learner_episodes could have put there, clamps too)
            const uint32_t last = (uint32_t)(p.M - 1);
            const uint32_t at = sc_base + ((uint32_t)sc_ep < last ? (uint32_t)sc_ep : last);
            if (p.sc_E) pe_E = p.sc_E[at];                      // (wave-uniform: a table is there or not)
            if (p.sc_alpha) pe_alpha = p.sc_alpha[at];
        }
    }
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
        if constexpr (SCHED) {
            sc_base = (uint32_t)p.sc_row[i] * (uint32_t)p.M;
            sc_ep = p.sc_ep[i];
            sched_lookup();
        }
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
    // after a step that is not a reset call: the episode ended -- the schedule moves on for the next step
    __device__ __forceinline__ void episode_end(bool ended) {
        if constexpr (SCHED) {
            if (ended) {
                sc_ep += 1;
                sched_lookup();
            }
        } else (void)ended;
    }
    __device__ __forceinline__ void finish(uint32_t i) {
        if constexpr (SCHED) p.sc_ep[i] = sc_ep;
        if (QLDS)
            for (uint32_t e = 0; e < entries(); e++) qg[(size_t)e * N] = q_lds[e * kBlock];
        if (p.carry_out) p.carry[i] = have_carry ? (int32_t)carried : -1;
    }
};

// (the step is called with or without the levels, not with empty ones: one call handed a NoiseLevelArgs{} of the kernel's own
//  making reorders instructions in 34 of the forms without levels)
template <bool PHILOX, bool NOISE, bool UNIT, bool QLDS, bool PE = false, bool DOUBLE = false, bool NLEV = false, int PM = 0, bool SCHED = false>
__global__ __launch_bounds__(kBlock) void k_discrete_learn_rollout(DiscreteArgs a, LearnArgsOf<PE, NLEV, SCHED> p, int K,
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
    LearnAgent<QLDS, PE, DOUBLE, SCHED> agent{p, (float *)q_lds + threadIdx.x, (uint32_t)a.A, (uint32_t)a.S * (uint32_t)a.A, (uint32_t)a.N};
    if constexpr (NLEV) closed_loop_rollout<PHILOX, NOISE, UNIT, false, NLEV, PM>(a, K, !a.obs_i32, p.actions, obs, reward, term, trunc, lds, zig, agent, EpisodeSummaryArgs{}, p.nl);
    else if constexpr (PM != 0) closed_loop_rollout<PHILOX, NOISE, UNIT, false, false, PM>(a, K, !a.obs_i32, p.actions, obs, reward, term, trunc, lds, zig, agent);
    else closed_loop_rollout<PHILOX, NOISE, UNIT>(a, K, !a.obs_i32, p.actions, obs, reward, term, trunc, lds, zig, agent);
}

// ... keeping episode summaries instead of writing the [K][N] arrays (p.actions is unused)
template <bool PHILOX, bool NOISE, bool UNIT, bool QLDS, bool PE = false, bool DOUBLE = false, bool NLEV = false, int PM = 0, bool SCHED = false>
__global__ __launch_bounds__(kBlock) void k_discrete_learn_summary(DiscreteArgs a, LearnArgsOf<PE, NLEV, SCHED> p, int K, EpisodeSummaryArgs sm) {
    extern __shared__ __align__(16) unsigned char lds[];
    const ZigLds zig = closed_loop_zig_lds<NOISE>();
    unsigned char *q_lds;                                           // the agent's LDS: behind the MDP's tables and the per-level cdfs
    if constexpr (NLEV && PM != 0) q_lds = lds + closed_agent_lds_offset<PM>(a, p.nl.lds_bytes);
    else {
        q_lds = lds + closed_agent_lds_offset<PM>(a);
        if constexpr (NLEV) q_lds += p.nl.lds_bytes;
    }
    LearnAgent<QLDS, PE, DOUBLE, SCHED> agent{p, (float *)q_lds + threadIdx.x, (uint32_t)a.A, (uint32_t)a.S * (uint32_t)a.A, (uint32_t)a.N};
    if constexpr (NLEV) closed_loop_rollout<PHILOX, NOISE, UNIT, true, NLEV, PM>(a, K, false, nullptr, nullptr, nullptr, nullptr, nullptr, lds, zig, agent, sm, p.nl);
    else if constexpr (PM != 0) closed_loop_rollout<PHILOX, NOISE, UNIT, true, false, PM>(a, K, false, nullptr, nullptr, nullptr, nullptr, nullptr, lds, zig, agent, sm);
    else closed_loop_rollout<PHILOX, NOISE, UNIT, true>(a, K, false, nullptr, nullptr, nullptr, nullptr, nullptr, lds, zig, agent, sm);
}

// NLEV = 1 with SCHED = 1: the same two kernels taking LearnArgsNLSched (overloads: the template arguments are the same, the
// second parameter tells them apart; LearnForm::kernel picks by it).  Their bodies are the NLEV branches of the ones above
template <bool PHILOX, bool NOISE, bool UNIT, bool QLDS, bool PE, bool DOUBLE, bool NLEV, int PM, bool SCHED>
__global__ __launch_bounds__(kBlock) void k_discrete_learn_rollout(DiscreteArgs a, LearnArgsNLSched p, int K,
                                                                   void *__restrict__ obs,
                                                                   float *__restrict__ reward,
                                                                   uint8_t *__restrict__ term,
                                                                   uint8_t *__restrict__ trunc) {
    static_assert(PE && NLEV && SCHED && NOISE, "the argument block of a schedule with per-env noise levels");
    extern __shared__ __align__(16) unsigned char lds[];
    const ZigLds zig = closed_loop_zig_lds<NOISE>();
    unsigned char *q_lds;                                           // the agent's LDS: behind the MDP's tables and the per-level cdfs
    if constexpr (PM != 0) q_lds = lds + closed_agent_lds_offset<PM>(a, p.nl.lds_bytes);
    else q_lds = lds + closed_agent_lds_offset<PM>(a) + p.nl.lds_bytes;
    LearnAgent<QLDS, PE, DOUBLE, SCHED> agent{p, (float *)q_lds + threadIdx.x, (uint32_t)a.A, (uint32_t)a.S * (uint32_t)a.A, (uint32_t)a.N};
    closed_loop_rollout<PHILOX, NOISE, UNIT, false, NLEV, PM>(a, K, !a.obs_i32, p.actions, obs, reward, term, trunc, lds, zig, agent, EpisodeSummaryArgs{}, p.nl);
}
template <bool PHILOX, bool NOISE, bool UNIT, bool QLDS, bool PE, bool DOUBLE, bool NLEV, int PM, bool SCHED>
__global__ __launch_bounds__(kBlock) void k_discrete_learn_summary(DiscreteArgs a, LearnArgsNLSched p, int K, EpisodeSummaryArgs sm) {
    static_assert(PE && NLEV && SCHED && NOISE, "the argument block of a schedule with per-env noise levels");
    extern __shared__ __align__(16) unsigned char lds[];
    const ZigLds zig = closed_loop_zig_lds<NOISE>();
    unsigned char *q_lds;                                           // the agent's LDS: behind the MDP's tables and the per-level cdfs
    if constexpr (PM != 0) q_lds = lds + closed_agent_lds_offset<PM>(a, p.nl.lds_bytes);
    else q_lds = lds + closed_agent_lds_offset<PM>(a) + p.nl.lds_bytes;
    LearnAgent<QLDS, PE, DOUBLE, SCHED> agent{p, (float *)q_lds + threadIdx.x, (uint32_t)a.A, (uint32_t)a.S * (uint32_t)a.A, (uint32_t)a.N};
    closed_loop_rollout<PHILOX, NOISE, UNIT, true, NLEV, PM>(a, K, false, nullptr, nullptr, nullptr, nullptr, nullptr, lds, zig, agent, sm, p.nl);
}

// ... and keeping an episode log beside them (mdpp_step_n_learn_log: sm.log_cap != 0).  Kernels of their own, so that the
// summary kernels above stay the code they were: the same bodies around closed_loop_rollout<..., LOG = true>
template <bool PHILOX, bool NOISE, bool UNIT, bool QLDS, bool PE = false, bool DOUBLE = false, bool NLEV = false, int PM = 0, bool SCHED = false>
__global__ __launch_bounds__(kBlock) void k_discrete_learn_summary_log(DiscreteArgs a, LearnArgsOf<PE, NLEV, SCHED> p, int K, EpisodeSummaryArgs sm) {
    extern __shared__ __align__(16) unsigned char lds[];
    const ZigLds zig = closed_loop_zig_lds<NOISE>();
    unsigned char *q_lds;
    if constexpr (NLEV && PM != 0) q_lds = lds + closed_agent_lds_offset<PM>(a, p.nl.lds_bytes);
    else {
        q_lds = lds + closed_agent_lds_offset<PM>(a);
        if constexpr (NLEV) q_lds += p.nl.lds_bytes;
    }
    LearnAgent<QLDS, PE, DOUBLE, SCHED> agent{p, (float *)q_lds + threadIdx.x, (uint32_t)a.A, (uint32_t)a.S * (uint32_t)a.A, (uint32_t)a.N};
    if constexpr (NLEV) closed_loop_rollout<PHILOX, NOISE, UNIT, true, NLEV, PM, true>(a, K, false, nullptr, nullptr, nullptr, nullptr, nullptr, lds, zig, agent, sm, p.nl);
    else closed_loop_rollout<PHILOX, NOISE, UNIT, true, false, PM, true>(a, K, false, nullptr, nullptr, nullptr, nullptr, nullptr, lds, zig, agent, sm);
}
template <bool PHILOX, bool NOISE, bool UNIT, bool QLDS, bool PE, bool DOUBLE, bool NLEV, int PM, bool SCHED>
__global__ __launch_bounds__(kBlock) void k_discrete_learn_summary_log(DiscreteArgs a, LearnArgsNLSched p, int K, EpisodeSummaryArgs sm) {
    static_assert(PE && NLEV && SCHED && NOISE, "the argument block of a schedule with per-env noise levels");
    extern __shared__ __align__(16) unsigned char lds[];
    const ZigLds zig = closed_loop_zig_lds<NOISE>();
    unsigned char *q_lds;
    if constexpr (PM != 0) q_lds = lds + closed_agent_lds_offset<PM>(a, p.nl.lds_bytes);
    else q_lds = lds + closed_agent_lds_offset<PM>(a) + p.nl.lds_bytes;
    LearnAgent<QLDS, PE, DOUBLE, SCHED> agent{p, (float *)q_lds + threadIdx.x, (uint32_t)a.A, (uint32_t)a.S * (uint32_t)a.A, (uint32_t)a.N};
    closed_loop_rollout<PHILOX, NOISE, UNIT, true, NLEV, PM, true>(a, K, false, nullptr, nullptr, nullptr, nullptr, nullptr, lds, zig, agent, sm, p.nl);
}

// One form of the learner, as launch_closed_form (mdpp_discrete_closed.hpp) takes it
template <bool PE, bool DOUBLE, bool SUMMARY_, bool NLEV_, bool SCHED>
struct LearnForm {
    static constexpr bool SUMMARY = SUMMARY_, NLEV = NLEV_, LOG = SUMMARY_;
    static constexpr int TABLES = DOUBLE ? 2 : 1;
    using Args = std::conditional_t<NLEV_ && SCHED, LearnArgsNLSched, LearnArgsOf<PE, NLEV_, SCHED>>;      // the kernel's second parameter
    // the kernel: full output, or summaries
    template <bool PH, bool NZ, bool UNIT, bool QL, int PM>
    static constexpr auto kernel() {
        static_assert(!NLEV || (NZ && PE), "per-env noise levels run the PE learner around a NOISE step");
        static_assert(PM == 0 || PE, "one MDP per env runs the PE learner");
        static_assert(!SCHED || PE, "a schedule runs the PE learner");
        // (the cast picks the overload by its second parameter)
        if constexpr (SUMMARY) return static_cast<void (*)(DiscreteArgs, Args, int, EpisodeSummaryArgs)>(k_discrete_learn_summary<PH, NZ, UNIT, QL, PE, DOUBLE, NLEV, PM, SCHED>);
        else return static_cast<void (*)(DiscreteArgs, Args, int, void *, float *, uint8_t *, uint8_t *)>(k_discrete_learn_rollout<PH, NZ, UNIT, QL, PE, DOUBLE, NLEV, PM, SCHED>);
    }
    // ... the summary form's kernel that keeps an episode log too
    template <bool PH, bool NZ, bool UNIT, bool QL, int PM>
    static constexpr auto kernel_log() {
        static_assert(SUMMARY, "the episode log is kept by the summary form");
        return static_cast<void (*)(DiscreteArgs, Args, int, EpisodeSummaryArgs)>(k_discrete_learn_summary_log<PH, NZ, UNIT, QL, PE, DOUBLE, NLEV, PM, SCHED>);
    }
    static void name(char *out, int ph, int nz, int unit, int ql, int pm) {
        if (pm)
            snprintf(out, kNameLen, "%s<PHILOX=%d,NOISE=%d,UNIT=%d,QLDS=%d,PE=1%s%s,PM=%d%s>", SUMMARY ? "k_discrete_learn_summary" : "k_discrete_learn_rollout",
                     ph, nz, unit, ql, DOUBLE ? ",DOUBLE=1" : "", NLEV ? ",NLEV=1" : "", pm, SCHED ? ",SCHED=1" : "");
        else
            snprintf(out, kNameLen, "%s<PHILOX=%d,NOISE=%d,UNIT=%d,QLDS=%d%s%s%s%s>", SUMMARY ? "k_discrete_learn_summary" : "k_discrete_learn_rollout",
                     ph, nz, unit, ql, PE ? ",PE=1" : "", DOUBLE ? ",DOUBLE=1" : "", NLEV ? ",NLEV=1" : "", SCHED ? ",SCHED=1" : "");
    }
    static Args args(const mdpp_env *h, const DiscreteIO &io, int k0, int kc, int32_t *actions, uint32_t cdf_lds) {
        const LearnArgs base{(float *)h->d_learn_q, (int32_t *)h->d_learn_carry, actions, h->learn_seed, h->learn_E,
                             h->learn_alpha, h->learn_gamma, h->learn_algo, k0 > 0 ? 1 : 0, k0 + kc < io.K ? 1 : 0};
        if constexpr (PE) {
            const LearnArgsPE pe{base, (const float *)h->d_learn_alpha, (const float *)h->d_learn_gamma, (const uint32_t *)h->d_learn_E};
            if constexpr (SCHED) {
                const LearnArgsSched sc{pe, h->sched_eps ? (const uint32_t *)h->d_sched_E : nullptr, h->sched_alpha ? (const float *)h->d_sched_alpha : nullptr,
                                        (const int32_t *)h->d_sched_row, (int32_t *)h->d_sched_ep, h->sched_M};
                if constexpr (NLEV) return LearnArgsNLSched{sc, noise_level_args(h, cdf_lds)};
                else return sc;
            } else if constexpr (NLEV) return LearnArgsNL{pe, noise_level_args(h, cdf_lds)};
            else return pe;
        } else return base;
    }
};

// K learning steps of one form (NLEV: of a handle with per-env noise levels; SCHED: of a handle with a per-episode schedule
// in force)
template <bool PE, bool DOUBLE, bool SUMMARY, bool NLEV, bool SCHED = false>
int launch_learn_form(mdpp_env *h, const DiscreteIO &io) {
    return launch_closed_form<LearnForm<PE, DOUBLE, SUMMARY, NLEV, SCHED>, false>(h, io);
}

// K learning steps of one form on a handle with one MDP per env (mdpp_learner_per_env_mdp): the PE learner's PM = 1 and
// PM = 2 kernels.  NLEV: with per-env noise levels (mdpp_noise_levels_per_env_mdp); SCHED: with a per-episode schedule in
// force (mdpp_learner_schedule_sweep)
template <bool DOUBLE, bool SUMMARY, bool NLEV, bool SCHED = false>
int launch_learn_form_pm(mdpp_env *h, const DiscreteIO &io) {
    // (the queue of start states drawn ahead needs shared tables: the PM kernels do not carry it)
    if (h->dargs.fast_ok || h->dargs.shared_tables) { h->err = "mdpp_step_n_learn: one MDP per env: the handle has shared tables"; return MDPP_ESTATE; }
    return launch_closed_form<LearnForm<true, DOUBLE, SUMMARY, NLEV, SCHED>, true>(h, io);
}

// the forms built <PE, DOUBLE, SUMMARY, NLEV[, SCHED]> and, with one MDP per env, <DOUBLE, SUMMARY, NLEV[, SCHED]>, each defined (an explicit
// instantiation) in the translation unit named
extern template int launch_learn_form<false, false, false, false>(mdpp_env *, const DiscreteIO &);  // mdpp_discrete_learn.hip
extern template int launch_learn_form<true, false, false, false>(mdpp_env *, const DiscreteIO &);   // mdpp_discrete_learn_pe.hip
extern template int launch_learn_form<false, true, false, false>(mdpp_env *, const DiscreteIO &);   // mdpp_discrete_learn_double.hip
extern template int launch_learn_form<true, true, false, false>(mdpp_env *, const DiscreteIO &);    // mdpp_discrete_learn_double_pe.hip
extern template int launch_learn_form<false, false, true, false>(mdpp_env *, const DiscreteIO &);   // mdpp_discrete_learn_summary.hip
extern template int launch_learn_form<true, false, true, false>(mdpp_env *, const DiscreteIO &);    // mdpp_discrete_learn_pe_summary.hip
extern template int launch_learn_form<false, true, true, false>(mdpp_env *, const DiscreteIO &);    // mdpp_discrete_learn_double_summary.hip
extern template int launch_learn_form<true, true, true, false>(mdpp_env *, const DiscreteIO &);     // mdpp_discrete_learn_double_pe_summary.hip
extern template int launch_learn_form<true, false, false, true>(mdpp_env *, const DiscreteIO &);    // mdpp_discrete_learn_pe_nlev.hip
extern template int launch_learn_form<true, true, false, true>(mdpp_env *, const DiscreteIO &);     // mdpp_discrete_learn_double_pe_nlev.hip
extern template int launch_learn_form<true, false, true, true>(mdpp_env *, const DiscreteIO &);     // mdpp_discrete_learn_pe_nlev_summary.hip
extern template int launch_learn_form<true, true, true, true>(mdpp_env *, const DiscreteIO &);      // mdpp_discrete_learn_double_pe_nlev_summary.hip
extern template int launch_learn_form<true, false, false, false, true>(mdpp_env *, const DiscreteIO &);  // mdpp_discrete_learn_pe_sched.hip
extern template int launch_learn_form<true, false, true, false, true>(mdpp_env *, const DiscreteIO &);   // mdpp_discrete_learn_pe_sched_summary.hip
extern template int launch_learn_form<true, true, false, false, true>(mdpp_env *, const DiscreteIO &);   // mdpp_discrete_learn_double_pe_sched.hip
extern template int launch_learn_form<true, true, true, false, true>(mdpp_env *, const DiscreteIO &);    // mdpp_discrete_learn_double_pe_sched_summary.hip
extern template int launch_learn_form_pm<false, false, false>(mdpp_env *, const DiscreteIO &);      // mdpp_discrete_learn_pe_pm.hip
extern template int launch_learn_form_pm<true, false, false>(mdpp_env *, const DiscreteIO &);       // mdpp_discrete_learn_double_pe_pm.hip
extern template int launch_learn_form_pm<false, true, false>(mdpp_env *, const DiscreteIO &);       // mdpp_discrete_learn_pe_pm_summary.hip
extern template int launch_learn_form_pm<true, true, false>(mdpp_env *, const DiscreteIO &);        // mdpp_discrete_learn_double_pe_pm_summary.hip
extern template int launch_learn_form_pm<false, false, true>(mdpp_env *, const DiscreteIO &);       // mdpp_discrete_learn_pe_pm_nlev.hip
extern template int launch_learn_form_pm<true, false, true>(mdpp_env *, const DiscreteIO &);        // mdpp_discrete_learn_double_pe_pm_nlev.hip
extern template int launch_learn_form_pm<false, true, true>(mdpp_env *, const DiscreteIO &);        // mdpp_discrete_learn_pe_pm_nlev_summary.hip
extern template int launch_learn_form_pm<true, true, true>(mdpp_env *, const DiscreteIO &);         // mdpp_discrete_learn_double_pe_pm_nlev_summary.hip
extern template int launch_learn_form<true, false, false, true, true>(mdpp_env *, const DiscreteIO &);   // mdpp_discrete_learn_pe_nlev_sched.hip
extern template int launch_learn_form<true, false, true, true, true>(mdpp_env *, const DiscreteIO &);    // mdpp_discrete_learn_pe_nlev_sched_summary.hip
extern template int launch_learn_form<true, true, false, true, true>(mdpp_env *, const DiscreteIO &);    // mdpp_discrete_learn_double_pe_nlev_sched.hip
extern template int launch_learn_form<true, true, true, true, true>(mdpp_env *, const DiscreteIO &);     // mdpp_discrete_learn_double_pe_nlev_sched_summary.hip
extern template int launch_learn_form_pm<false, false, false, true>(mdpp_env *, const DiscreteIO &);     // mdpp_discrete_learn_pe_pm_sched.hip
extern template int launch_learn_form_pm<true, false, false, true>(mdpp_env *, const DiscreteIO &);      // mdpp_discrete_learn_double_pe_pm_sched.hip
extern template int launch_learn_form_pm<false, true, false, true>(mdpp_env *, const DiscreteIO &);      // mdpp_discrete_learn_pe_pm_sched_summary.hip
extern template int launch_learn_form_pm<true, true, false, true>(mdpp_env *, const DiscreteIO &);       // mdpp_discrete_learn_double_pe_pm_sched_summary.hip
extern template int launch_learn_form_pm<false, false, true, true>(mdpp_env *, const DiscreteIO &);      // mdpp_discrete_learn_pe_pm_nlev_sched.hip
extern template int launch_learn_form_pm<true, false, true, true>(mdpp_env *, const DiscreteIO &);       // mdpp_discrete_learn_double_pe_pm_nlev_sched.hip
extern template int launch_learn_form_pm<false, true, true, true>(mdpp_env *, const DiscreteIO &);       // mdpp_discrete_learn_pe_pm_nlev_sched_summary.hip
extern template int launch_learn_form_pm<true, true, true, true>(mdpp_env *, const DiscreteIO &);        // mdpp_discrete_learn_double_pe_pm_nlev_sched_summary.hip

} // namespace mdpp
