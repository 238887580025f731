// Greedy evaluation's plain rollout form (mdpp_discrete_eval.hpp has the agent, the kernels and the launcher of every form), the
// dispatcher that picks a handle's form, and the observation every env shows now.
#include "mdpp_discrete_eval.hpp"

namespace mdpp {

template int launch_eval_form<false, false>(mdpp_env *, const DiscreteIO &);

int launch_discrete_eval(mdpp_env *h, const DiscreteIO &io) {
    const std::string why = discrete_learn_refusal(h);
    if (!why.empty()) { h->err = "mdpp_step_n_eval: " + why; return MDPP_EUNSUPPORTED; }
    int rc = MDPP_OK;
    if (h->learn_pm && h->cfg.num_tables != 1) {                 // one MDP per env: the PM kernels
        with_bools([&](auto SM, auto NL) { rc = launch_eval_form_pm<SM(), NL()>(h, io); }, io.summary != nullptr, h->nl_on);
        return rc;
    }
    with_bools([&](auto SM, auto NL) { rc = launch_eval_form<SM(), NL()>(h, io); }, io.summary != nullptr, h->nl_on);
    return rc;
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
} // namespace mdpp
