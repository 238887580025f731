// The in-kernel tabular TD learners' uniform rollout form (Q-learning and SARSA, one set of hyper-parameters: mdpp_discrete_learn.hpp
// has the agent, the kernels and the launcher of every form), the dispatcher that picks a handle's form, and what the learner
// needs besides: Q between the caller's layout and the handle's, the fill of the per-env parameter arrays.
#include "mdpp_discrete_learn.hpp"

namespace mdpp {

template int launch_learn_form<false, false, false, false>(mdpp_env *, const DiscreteIO &);

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
std::string discrete_learn_refusal(const mdpp_env *h) { return closed_loop_refusal(h, "learner", true, 0, "the MDP's tables", true); }

// K learning steps
int launch_discrete_learn(mdpp_env *h, const DiscreteIO &io) {
    const std::string why = discrete_learn_refusal(h);
    if (!why.empty()) { h->err = "mdpp_step_n_learn: " + why; return MDPP_EUNSUPPORTED; }
    const bool dbl = h->learn_algo == MDPP_LEARN_DOUBLE_Q;
    const bool pm = h->learn_pm && h->cfg.num_tables != 1;       // one MDP per env: the PM kernels
    if ((h->nl_on || pm || h->sched_on) && !h->learn_pe) {
        // per-env noise levels, one MDP per env and a per-episode schedule run the PE form: while all three parameters are uniform their arrays are
        // filled here, and again when a value has changed since (the scalar setters do not mark them while nothing is per-env).
        // The arrays themselves are mdpp_set_noise_levels' (mdpp_set_learner's with one MDP per env): a launch entry point
        // allocates nothing (it may be under a graph capture)
        const bool fresh = h->nl_fill_valid && h->nl_fill_alpha == h->learn_alpha && h->nl_fill_gamma == h->learn_gamma && h->nl_fill_E == h->learn_E;
        if (!fresh && !io.name_out) {
            if (!h->d_learn_alpha || !h->d_learn_gamma || !h->d_learn_E) { h->err = "mdpp_step_n_learn: the per-env parameter arrays are missing (mdpp_set_noise_levels / mdpp_set_learner / mdpp_set_learner_schedule allocate them)"; return MDPP_ESTATE; }
            h->learn_pe_stale = 7u;
        }
    } else {
        h->nl_fill_valid = false;
    }
    const bool pe = h->learn_pe || h->nl_on || pm || h->sched_on;
    if (pe && h->learn_pe_stale && !io.name_out) {
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
    if (h->trace_kind) return launch_discrete_trace(h, io, pe);        // eligibility traces: the trace kernels (mdpp_discrete_trace.hip)
    int rc = MDPP_OK;
    if (pm) {
        with_bools([&](auto DB, auto SM, auto NL, auto SC) { rc = launch_learn_form_pm<DB(), SM(), NL(), SC()>(h, io); }, dbl, io.summary != nullptr, h->nl_on, h->sched_on);
        return rc;
    }
    if (h->sched_on) {           // (the PE form with the tables, on a shared MDP; with levels only under mdpp_learner_schedule_sweep, which mdpp_set_learner_schedule and mdpp_set_noise_levels see to)
        with_bools([&](auto DB, auto SM, auto NL) { rc = launch_learn_form<true, DB(), SM(), NL(), true>(h, io); }, dbl, io.summary != nullptr, h->nl_on);
        return rc;
    }
    with_bools([&](auto PE, auto DB, auto SM, auto NL) {
        if constexpr (PE() || !NL()) rc = launch_learn_form<PE(), DB(), SM(), NL()>(h, io);
    }, pe, dbl, io.summary != nullptr, h->nl_on);
    return rc;
}

} // namespace mdpp
