// Eligibility traces for the in-kernel tabular learners (mdpp_discrete_trace.hpp has the agent, the kernels and the launcher of
// every form): the uniform rollout form, the dispatcher that picks a handle's form, and Z between the caller's layout and the
// handle's.
#include "mdpp_discrete_trace.hpp"

namespace mdpp {

template int launch_trace_form<false, false, false>(mdpp_env *, const DiscreteIO &);

// Z between the caller's [N][S A] and the handle's [S A][N]
template <bool TO_HANDLE>
__global__ __launch_bounds__(kBlock) void k_trace_z_transpose(float *__restrict__ handle_z, float *__restrict__ user_z, uint32_t N, uint32_t SA) {
    const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (uint64_t)N * SA) return;
    const uint32_t e = (uint32_t)(t / N), i = (uint32_t)(t - (uint64_t)e * N);
    if (TO_HANDLE) handle_z[t] = user_z[(size_t)i * SA + e];
    else user_z[(size_t)i * SA + e] = handle_z[t];
}

int launch_trace_z_copy(mdpp_env *h, float *user_z, bool to_handle, hipStream_t s) {
    const uint32_t N = (uint32_t)h->cfg.num_envs, SA = (uint32_t)h->cfg.S * (uint32_t)h->cfg.A;
    const uint64_t total = (uint64_t)N * SA;
    const uint64_t grid = (total + kBlock - 1) / kBlock;
    if (grid > 0x7FFFFFFFull) { h->err = "k_trace_z_transpose: table too large"; return MDPP_EUNSUPPORTED; }
    if (to_handle) hipLaunchKernelGGL(k_trace_z_transpose<true>, dim3((uint32_t)grid), dim3(kBlock), 0, s, (float *)h->d_trace_z, user_z, N, SA);
    else hipLaunchKernelGGL(k_trace_z_transpose<false>, dim3((uint32_t)grid), dim3(kBlock), 0, s, (float *)h->d_trace_z, user_z, N, SA);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { h->err = std::string("k_trace_z_transpose launch: ") + hipGetErrorString(e); return MDPP_EHIP; }
    return MDPP_OK;
}

// K learning steps of a handle with traces (launch_discrete_learn has made its checks and filled the per-env arrays; pe: the
// launch takes the PE form).  The setters keep such a handle to the forms built: one table, no levels, and a shared MDP or --
// under mdpp_learner_traces_per_env_mdp -- one MDP per env, the sweep schedule with the latter only
int launch_discrete_trace(mdpp_env *h, const DiscreteIO &io, bool pe) {
    const bool pm = h->learn_pm && h->cfg.num_tables != 1;       // one MDP per env: the PM kernels
    if (h->learn_algo == MDPP_LEARN_DOUBLE_Q || h->nl_on || (pm && !(h->trace_pm && pe)) || !h->d_trace_z || !h->d_trace_lambda) {
        h->err = "mdpp_step_n_learn: eligibility traces: the handle is not one the trace kernels serve";
        return MDPP_ESTATE;
    }
    int rc = MDPP_OK;
    if (pm) {
        with_bools([&](auto SM, auto SC) { rc = launch_trace_form_pm<SM(), SC()>(h, io); }, io.summary != nullptr, h->sched_on);
        return rc;
    }
    if (h->sched_on) {
        with_bools([&](auto SM) { rc = launch_trace_form<true, SM(), true>(h, io); }, io.summary != nullptr);
        return rc;
    }
    with_bools([&](auto PE, auto SM) { rc = launch_trace_form<PE(), SM(), false>(h, io); }, pe, io.summary != nullptr);
    return rc;
}

} // namespace mdpp
