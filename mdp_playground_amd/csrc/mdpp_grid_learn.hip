// Grid learners (include/mdpp.h "Grid learners"; the kernel and the launcher of one output form: mdpp_grid_learn.hpp): the
// full-output instantiations of k_grid_learn_rollout, what a grid handle is refused for, the dispatcher between the two
// output forms (the summary form is built in mdpp_grid_summary_learn.hip) and their SCHED and LOG forms (built in
// mdpp_grid_sched_learn.hip, mdpp_grid_summary_sched_learn.hip, mdpp_grid_episodes_learn.hip, mdpp_grid_episodes_sched_learn.hip), the
// same six forms under per-env noise levels (built in the six mdpp_grid_*levels*_learn.hip units) and the copy of Q between
// the caller's [N][S][A] and the handle's entry-major [S A][N].
#include "mdpp_grid_learn.hpp"

namespace mdpp {

template int launch_grid_learn_form<false>(mdpp_env *, const DiscreteIO &, bool);

std::string grid_learn_refusal(const mdpp_env *h) {
    const mdpp_config &c = h->cfg;
    if (c.kind != MDPP_KIND_GRID) return "grid learners serve grid envs only";
    if (c.grid_dims != 2) return "grid learners need grid_dims == 2 (irrelevant_features: not built)";
    if (c.image) return "grid learners do not serve image observations";
    if (c.episode_stats) return "grid learners do not serve episode_stats";
    return "";
}

// (evaluation reads no table and moves no counter: it keeps its kernels whatever schedule is in force; the episode log is the
//  learner's summary form with io.summary->log_cap != 0)
int launch_grid_learn(mdpp_env *h, const DiscreteIO &io, bool eval) {
    const bool sched = h->gl_sched_on && !eval;
    if (h->gl_nl_on) {           // per-env noise levels: the same forms on the NLEV kernels
        if (io.summary && io.summary->log_cap != 0u)
            return sched ? launch_grid_learn_form<true, true, true, true>(h, io, eval) : launch_grid_learn_form<true, false, true, true>(h, io, eval);
        if (sched) return io.summary ? launch_grid_learn_form<true, true, false, true>(h, io, eval) : launch_grid_learn_form<false, true, false, true>(h, io, eval);
        return io.summary ? launch_grid_learn_form<true, false, false, true>(h, io, eval) : launch_grid_learn_form<false, false, false, true>(h, io, eval);
    }
    if (io.summary && io.summary->log_cap != 0u)
        return sched ? launch_grid_learn_form<true, true, true>(h, io, eval) : launch_grid_learn_form<true, false, true>(h, io, eval);
    if (sched) return io.summary ? launch_grid_learn_form<true, true>(h, io, eval) : launch_grid_learn_form<false, true>(h, io, eval);
    return io.summary ? launch_grid_learn_form<true>(h, io, eval) : launch_grid_learn_form<false>(h, io, eval);
}

// one thread per entry of the handle's buffer: entry e of env i at handle[e N + i] <-> user[i SA + e]  (N SA < 2^30)
__global__ __launch_bounds__(kBlock) void k_grid_q_copy(float *__restrict__ handle, float *__restrict__ user, uint32_t N, uint32_t SA,
                                                        int to_handle) {
    const uint32_t idx = blockIdx.x * kBlock + threadIdx.x;
    if (idx >= N * SA) return;
    const uint32_t e = idx / N, i = idx - e * N;
    if (to_handle) handle[idx] = user[(size_t)i * SA + e];
    else user[(size_t)i * SA + e] = handle[idx];
}

int launch_grid_q_copy(mdpp_env *h, float *user_q, bool to_handle, hipStream_t s) {
    const uint32_t N = (uint32_t)h->cfg.num_envs;
    const uint32_t SA = (uint32_t)(h->cfg.grid_shape[0] + 1) * (uint32_t)(h->cfg.grid_shape[1] + 1) * (uint32_t)h->gl_A;
    const uint32_t total = N * SA;
    hipLaunchKernelGGL(k_grid_q_copy, dim3((total + kBlock - 1) / kBlock), dim3(kBlock), 0, s, (float *)h->d_gl_q, user_q, N, SA,
                       to_handle ? 1 : 0);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { h->err = std::string("k_grid_q_copy launch: ") + hipGetErrorString(e); return MDPP_EHIP; }
    return MDPP_OK;
}

} // namespace mdpp
