// Closed-loop continuous rollouts under a linear policy per env (mdpp_set_linear_policy / mdpp_step_n_linear):
//   a = clip(W o + b, +-action_space_max),  o = the state in the env's record,
// evaluated inside the launch, around the step of mdpp_continuous_closed.hpp.  This translation unit holds the full-output
// kernels k_continuous_linear_rollout, the parameter buffer's copy kernel, the continuous mdpp_current_obs and the launcher;
// mdpp_continuous_summary_linear.hip includes it with MDPP_CLIN_TU_SUMMARY = 1 and holds k_continuous_linear_summary.
//
// The action (include/mdpp.h "Linear policies"): for r = 0 .. D-1, acc = b[r], then for c = 0 .. D-1 in that order
// acc = acc + W[r][c] * o[c], every product and every sum rounded to float32 (no FMA: -ffp-contract=off), then the clamp
// acc < -amax ? -amax : (acc > amax ? amax : acc); a NaN acc stays NaN and fails the step's admission test C1.
//
// Parameters: the handle's buffer is entry-major, entry e = r (D + 1) + c (c == D: b[r]) of env i at theta[e se + i si];
// per-env parameters (se, si) = (N, 1) -- consecutive lanes, consecutive addresses --, a shared policy (1, 0).
// PLDS = 1: every lane stages its entries once per launch at p_lds[e 256 + tid] (dynamic LDS; bank = lane, so no conflict
// whatever entry the lanes read) and reads them from there at every step.  PLDS = 0: the same indexing on the device buffer
// at every step.  The launcher takes PLDS = 1 when 256 D (D + 1) 4 bytes of dynamic LDS are granted beside the kernel's static
// LDS and MDPP_OPT_NO_LINEAR_LDS is not set.
//
// History 2 (a = clip(W o + V p + b), include/mdpp.h "Linear policies with memory"): mdpp_continuous_linear_h2.hip and
// mdpp_continuous_summary_linear_h2.hip include this file with MDPP_LINEAR_HIST = 2 and hold the HIST=2 forms of the two kernels
// and their launchers, nothing else; the act is mdpp_linear_history.hpp's.  E = D (HIST D + 1) everywhere below.
#ifndef MDPP_CLIN_TU_SUMMARY
#define MDPP_CLIN_TU_SUMMARY 0     // 1: this translation unit holds k_continuous_linear_summary (mdpp_continuous_summary_linear.hip)
#endif

#include "mdpp_continuous_closed.hpp"
#include "mdpp_linear_history.hpp"

namespace mdpp {

struct LinearParams {
    const float *theta;         // the handle's entry-major buffer
    long se, si;                // element strides of an entry and of an env
};

template <int DMAX, bool PLDS, int HIST>
struct LinearAgent {
    static constexpr int kHist = HIST;
    long N;                     // HIST = 2 (the other forms leave both unset)
    float *mem;                 // HIST = 2: the handle's memory [D][N]; from begin() on component 0 of this lane's
    const float *theta;         // PLDS = 0: entry 0 of this lane
    long se;
    const float *lds;           // PLDS = 1: entry 0 of this lane, entry e at lds[e 256]
    float *stage;
    LinearParams lp;
    int D;
    float amax;
    __device__ __forceinline__ void begin(long i) {
        theta = lp.theta + i * lp.si;
        se = lp.se;
        if constexpr (PLDS) {
            float *mine = stage + threadIdx.x;
            const int E = D * (HIST * D + 1);
            for (int e = 0; e < E; e++) mine[e * kBlock] = theta[(long)e * se];
            lds = mine;         // (this lane's column alone: no barrier)
        }
        if constexpr (HIST == 2) mem += i;
    }
    // HIST = 2: the step calls this form (first: no step taken in the env's current episode)
    __device__ __forceinline__ void act(const float (&o)[DMAX], float (&a)[DMAX], bool first) const {
        linear_act_h2<DMAX>(PLDS ? lds : theta, PLDS ? (long)kBlock : se, D, amax, o, mem, N, first, a);
    }
    // (the entries are walked with ONE running pointer, a step of `stride` elements per entry: indexed as e stride, the D (D + 1)
    //  wave-uniform offsets are hoisted out of the step loop and 156 of them at D = 12 do not fit the scalar registers)
    __device__ __forceinline__ void act(const float (&o)[DMAX], float (&a)[DMAX]) const {
        const long stride = PLDS ? (long)kBlock : se;
        const long b_off = (long)D * stride;               // row r: W[r][0 .. D-1], then b[r]
        const float *p = PLDS ? lds : theta;
#pragma unroll
        for (int r = 0; r < DMAX; r++) {
            float acc = 0.0f;
            if (r < D) {
                acc = p[b_off];
#pragma unroll
                for (int c = 0; c < DMAX; c++)
                    if (c < D) { const float w = *p; const float t = w * o[c]; acc = acc + t; p += stride; }
                p += stride;
                acc = acc < -amax ? -amax : (acc > amax ? amax : acc);
            }
            a[r] = acc;
        }
    }
    __device__ __forceinline__ void observe(float, bool) const {}
    __device__ __forceinline__ void finish(long) const {}
};

#if MDPP_CLIN_TU_SUMMARY
template <int DMAX, int OMAX, bool PHILOX, bool NOISE, bool PLDS MDPP_HIST_TPARAM>
__global__ __launch_bounds__(kBlock) void k_continuous_linear_summary(ContinuousArgs a, int K, LinearParams lp, EpisodeSummaryArgs sm MDPP_HIST_KPARAM) {
    extern __shared__ __align__(16) float s_theta[];
    LinearAgent<DMAX, PLDS, MDPP_LINEAR_HIST> agent;
    MDPP_HIST_SET_MEM(agent, a.N) agent.lp = lp; agent.D = a.D; agent.amax = a.amax32; agent.stage = s_theta;
    continuous_closed_rollout<DMAX, OMAX, PHILOX, NOISE, true>(a, K, agent, ContinuousClosedOut{}, sm);
}
#define MDPP_CLIN_KERNEL k_continuous_linear_summary
#define MDPP_CLIN_NAME "k_continuous_linear_summary"
#else
template <int DMAX, int OMAX, bool PHILOX, bool NOISE, bool PLDS MDPP_HIST_TPARAM>
__global__ __launch_bounds__(kBlock) void k_continuous_linear_rollout(ContinuousArgs a, int K, LinearParams lp, ContinuousClosedOut out MDPP_HIST_KPARAM) {
    extern __shared__ __align__(16) float s_theta[];
    LinearAgent<DMAX, PLDS, MDPP_LINEAR_HIST> agent;
    MDPP_HIST_SET_MEM(agent, a.N) agent.lp = lp; agent.D = a.D; agent.amax = a.amax32; agent.stage = s_theta;
    continuous_closed_rollout<DMAX, OMAX, PHILOX, NOISE, false>(a, K, agent, out, EpisodeSummaryArgs{});
}
#define MDPP_CLIN_KERNEL k_continuous_linear_rollout
#define MDPP_CLIN_NAME "k_continuous_linear_rollout"
#endif

// One form of this unit's kernel on (padded D, padded order): the placement, the name, the launch
template <int DMAX, int OMAX>
static void launch_linear_t(const ContinuousArgs &a, const ContinuousIO &io, const LinearParams &lp, float *mem) {
    const long grid = ((long)a.N + kBlock - 1) / kBlock;
    const bool noise = a.has_p_noise || a.has_r_noise;
    const size_t want = (size_t)kBlock * a.D * (MDPP_LINEAR_HIST * a.D + 1) * sizeof(float);
    with_bools([&](auto PH, auto NZ) {
        constexpr bool kPh = decltype(PH)::value, kNz = decltype(NZ)::value;
        const bool plds = !(a.opts & MDPP_OPT_NO_LINEAR_LDS) &&
                          dynamic_lds_ok((const void *)MDPP_CLIN_KERNEL<DMAX, OMAX, kPh, kNz, true MDPP_HIST_TARG>, want);
        with_bools([&](auto PL) {
            constexpr bool kPl = decltype(PL)::value;
            if (io.name_out) {
                snprintf(io.name_out, kNameLen, MDPP_CLIN_NAME "<D=%d,ORDER=%d,PHILOX=%d,NOISE=%d,PLDS=%d" MDPP_HIST_NAME ">", DMAX, OMAX, (int)kPh, (int)kNz, (int)kPl);
                return;
            }
            const size_t lds = kPl ? want : 0;
#if MDPP_CLIN_TU_SUMMARY
            hipLaunchKernelGGL((k_continuous_linear_summary<DMAX, OMAX, kPh, kNz, kPl MDPP_HIST_TARG>), dim3((unsigned)grid), dim3(kBlock), lds, io.s, a, io.K, lp, *io.summary MDPP_HIST_KARG);
#else
            // (ContinuousIO::actions is const for the open-loop launchers; the closed-loop launchers WRITE the actions taken there)
            hipLaunchKernelGGL((k_continuous_linear_rollout<DMAX, OMAX, kPh, kNz, kPl MDPP_HIST_TARG>), dim3((unsigned)grid), dim3(kBlock), lds, io.s, a, io.K, lp,
                               ContinuousClosedOut{const_cast<float *>(io.actions), io.obs, io.reward, io.term, io.trunc} MDPP_HIST_KARG);
#endif
        }, plds);
    }, a.philox != 0, noise);
}

// the (2,2), (4,2), (12,1) and (12,2) shapes of MDPP_C_DISPATCH (mdpp_continuous.hip); false: D > 12 or order > 2
static bool launch_linear_dispatch(const ContinuousArgs &a, const ContinuousIO &io, const LinearParams &lp, float *mem = nullptr) {
    if (a.order > 2 || a.D > 12) return false;
    if (a.D <= 2) launch_linear_t<2, 2>(a, io, lp, mem);
    else if (a.D <= 4) launch_linear_t<4, 2>(a, io, lp, mem);
    else if (a.order <= 1) launch_linear_t<12, 1>(a, io, lp, mem);
    else launch_linear_t<12, 2>(a, io, lp, mem);
    return true;
}

#if MDPP_LINEAR_HIST == 2 && MDPP_CLIN_TU_SUMMARY
bool launch_continuous_linear_summary_h2_form(const ContinuousArgs &a, const ContinuousIO &io, const LinearParams &lp, float *mem) {
    return launch_linear_dispatch(a, io, lp, mem);
}
#elif MDPP_LINEAR_HIST == 2
bool launch_continuous_linear_h2_form(const ContinuousArgs &a, const ContinuousIO &io, const LinearParams &lp, float *mem) {
    return launch_linear_dispatch(a, io, lp, mem);
}
#elif MDPP_CLIN_TU_SUMMARY
bool launch_continuous_linear_summary_form(const ContinuousArgs &a, const ContinuousIO &io, const float *theta, long se, long si) {
    return launch_linear_dispatch(a, io, LinearParams{theta, se, si});
}
#else
bool launch_continuous_linear_summary_form(const ContinuousArgs &a, const ContinuousIO &io, const float *theta, long se, long si);
bool launch_continuous_linear_h2_form(const ContinuousArgs &a, const ContinuousIO &io, const LinearParams &lp, float *mem);
bool launch_continuous_linear_summary_h2_form(const ContinuousArgs &a, const ContinuousIO &io, const LinearParams &lp, float *mem);

std::string continuous_linear_refusal(const mdpp_env *h) {
    const mdpp_config &c = h->cfg;
    if (c.kind == MDPP_KIND_DISCRETE) return "linear-policy rollouts serve continuous envs only (this handle is discrete)";
    if (c.kind == MDPP_KIND_GRID) return "linear-policy rollouts serve continuous envs only (this handle is a grid)";
    if (h->cargs.line_L) return "linear-policy rollouts do not serve reward_function move_along_a_line";
    if (c.image) return "linear-policy rollouts do not serve image observations";
    if (c.episode_stats) return "linear-policy rollouts do not serve episode_stats";
    if (c.D > 12) return "linear-policy rollouts serve state_space_dim <= 12";
    if (c.order > 2) return "linear-policy rollouts serve transition_dynamics_order <= 2";
    return "";
}

// io.K steps under the handle's linear policy; io.summary: the summary form; io.name_out: a dry run (of the summary form
// with any non-null io.summary: it is not read)
int launch_continuous_linear(mdpp_env *h, const ContinuousIO &io) {
    ContinuousArgs a = h->cargs;
    stamp_step(a, h);
    const long N = a.N;
    const float *theta = (const float *)h->d_lin_theta;
    const long se = h->lin_per_env ? N : 1, si = h->lin_per_env ? 1 : 0;
    const bool summary = io.summary != nullptr;
    const LinearParams lp{theta, se, si};
    float *mem = (float *)h->d_lin_mem;
    const bool served = h->lin_hist == 2 ? (summary ? launch_continuous_linear_summary_h2_form(a, io, lp, mem) : launch_continuous_linear_h2_form(a, io, lp, mem))
                        : summary        ? launch_continuous_linear_summary_form(a, io, theta, se, si)
                                         : launch_linear_dispatch(a, io, lp);
    if (!served) { h->err = "linear-policy rollouts serve state_space_dim <= 12 and transition_dynamics_order <= 2"; return MDPP_EUNSUPPORTED; }
    return io.name_out ? MDPP_OK : step_done(h, io.K, summary ? "k_continuous_linear_summary" : "k_continuous_linear_rollout");
}

// The parameters between the caller's layout ([D][HIST D + 1], or [N][D][HIST D + 1]) and the handle's entry-major buffer
__global__ __launch_bounds__(kBlock) void k_linear_theta_copy(float *__restrict__ handle, float *__restrict__ user, long N, int E, int per_env,
                                                              int to_handle) {
    const long t = (long)blockIdx.x * kBlock + threadIdx.x;     // per env: t = e N + i (the handle's order: its side is coalesced)
    const long total = per_env ? N * E : (long)E;
    if (t >= total) return;
    const long e = per_env ? t / N : t, i = per_env ? t % N : 0;
    float *u = user + i * E + e;
    if (to_handle) handle[t] = *u; else *u = handle[t];
}

int launch_linear_theta_copy(mdpp_env *h, float *user, bool to_handle, hipStream_t s) {
    const long N = h->cfg.num_envs;
    const int E = h->cfg.D * (h->lin_hist * h->cfg.D + 1);
    const long total = h->lin_per_env ? N * E : (long)E;
    hipLaunchKernelGGL(k_linear_theta_copy, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, (float *)h->d_lin_theta, user, N, E,
                       h->lin_per_env ? 1 : 0, to_handle ? 1 : 0);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { h->err = std::string("k_linear_theta_copy launch: ") + hipGetErrorString(e); return MDPP_EHIP; }
    return MDPP_OK;
}

// mdpp_current_obs of a continuous handle: the state in every env's record, cur [D][N], as the observation [N][D]
__global__ __launch_bounds__(kBlock) void k_continuous_current_obs(const float *__restrict__ cur, float *__restrict__ obs, long N, int D) {
    const long i = (long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    for (int d = 0; d < D; d++) obs[i * D + d] = cur[(long)d * N + i];
}

int launch_continuous_current_obs(mdpp_env *h, float *obs, hipStream_t s) {
    const long N = h->cfg.num_envs;
    hipLaunchKernelGGL(k_continuous_current_obs, dim3((unsigned)((N + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, (const float *)h->d_cur, obs, N, h->cfg.D);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { h->err = std::string("k_continuous_current_obs launch: ") + hipGetErrorString(e); return MDPP_EHIP; }
    return MDPP_OK;
}

// mdpp_linear_memory: the memory of a history = 2 policy, [D][N] in the handle, between it and the caller's [N][D]
__global__ __launch_bounds__(kBlock) void k_linear_memory_copy(float *__restrict__ mem, float *__restrict__ user, long N, int D, int to_handle) {
    const long i = (long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    for (int d = 0; d < D; d++) {
        if (to_handle) mem[(long)d * N + i] = user[i * D + d]; else user[i * D + d] = mem[(long)d * N + i];
    }
}

int launch_linear_memory_copy(mdpp_env *h, float *user, bool to_handle, hipStream_t s) {
    const long N = h->cfg.num_envs;
    hipLaunchKernelGGL(k_linear_memory_copy, dim3((unsigned)((N + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, (float *)h->d_lin_mem, user, N, h->cfg.D,
                       to_handle ? 1 : 0);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { h->err = std::string("k_linear_memory_copy launch: ") + hipGetErrorString(e); return MDPP_EHIP; }
    return MDPP_OK;
}
#endif   // !MDPP_CLIN_TU_SUMMARY

} // namespace mdpp
