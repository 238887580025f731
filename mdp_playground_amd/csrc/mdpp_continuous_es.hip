// Linear policy ES inside the launch (mdpp_step_n_linear_es; include/mdpp.h "Linear policy ES"): the 64 envs of a WAVE are one
// population, 32 antithetic pairs around one mean, around the step of mdpp_continuous_closed.hpp.  The CANDIDATE of env i is the
// handle's linear-policy buffer, as in the search (mdpp_continuous_search.hip); the means and everything else are the caller's
// arrays.  This translation unit holds the full-output kernels k_continuous_es_rollout, the launcher and mdpp_linear_es_init's
// kernel; mdpp_continuous_summary_es.hip includes it with MDPP_CES_TU_SUMMARY = 1 and holds k_continuous_es_summary.
//
// Per env (EsAgent::observe, at every step that is not a reset call): 0 <= eps < T: ret += (double)rw; at an episode's end
// acc += ret, ret = 0, eps += 1 there, and eps = 0 for a waiting member (eps == -1).  Only ret, eps and two flags are live
// across steps; acc is read-modify-written in memory at episode ends (the D = 12 step already holds 250 VGPRs).
//
// Per group, after every step: observe() sits behind the `continue` of the lanes in a reset call, so it runs under divergent
// control flow and holds no cross-lane operation.  Every live lane of a wave runs the same K iterations (N % 64 == 0: a wave is
// whole or gone), so the wave is converged at the top of the loop body and after the loop: the vote on the step just completed is
// taken at the START of act() for k >= 1 and once in finish().  `stepped`: this lane has completed a step in this launch;
// `fresh`: its last completed step was no reset call and ended an episode.
//
// A generation end (EsAgent::generation_end) is wave-uniform by construction: ranks by 64 __shfl of the sort key, the float64
// butterfly of the log, then ONE rolled loop over the E = D (D + 1) entries with two Philox generators (tick gen: the
// perturbation the candidates were made with; tick gen + 1: the next one), a float32 butterfly per entry, one running pointer
// for the candidate and one for the mean (a wave-uniform address).  No LDS, no barrier, no atomics.  Products and sums are
// rounded one by one (-ffp-contract=off).
//
// The candidate's placement is the search's: PLDS = 1, staged once per launch at p_lds[e 256 + tid], rewritten there at a
// generation end (the lane's own column) and written back by finish() when a generation moved; PLDS = 0, in the buffer itself.
//
// History 2 (include/mdpp.h "Linear policies with memory"): the *_h2.hip units include this file with MDPP_LINEAR_HIST = 2 and hold
// the HIST=2 forms of the two kernels and their launchers, nothing else; the act is mdpp_linear_history.hpp's, and everything
// below that walks the entries walks E = D (HIST D + 1) of them.
#ifndef MDPP_CES_TU_SUMMARY
#define MDPP_CES_TU_SUMMARY 0    // 1: this translation unit holds k_continuous_es_summary (mdpp_continuous_summary_es.hip)
#endif

#include "mdpp_continuous_closed.hpp"
#include "mdpp_linear_history.hpp"

namespace mdpp {

struct EsParams {
    mdpp_linear_es s;           // the caller's arrays and constants
    float *cand;                // the handle's entry-major buffer: entry e of env i at cand[e N + i]
};

template <int DMAX, bool PLDS, int HIST>
struct EsAgent {
    static constexpr int kHist = HIST;
    float *mem;                 // HIST = 2: the handle's memory [D][N]; from begin() on component 0 of this lane's
    float *cand;                // entry 0 of this lane in the handle's buffer, entry e at cand[e N]
    float *lds;                 // PLDS = 1: entry 0 of this lane, entry e at lds[e 256]
    float *stage;
    EsParams sp;
    long N, i;
    uint64_t env0;
    int D;
    float amax;
    double ret;                 // the running return of the current counted episode
    int32_t eps;                // -1: waiting for an episode boundary; 0 .. T-1: counting; T: done
    bool stepped, fresh;
    bool moved;                 // a generation ended in this launch: the staged candidate is newer than the buffer's
    __device__ __forceinline__ void begin(long lane) {
        i = lane;
        cand = sp.cand + i;
        if constexpr (HIST == 2) mem += i;
        if constexpr (PLDS) {
            float *mine = stage + threadIdx.x;
            const int E = D * (HIST * D + 1);
            for (int e = 0; e < E; e++) mine[e * kBlock] = cand[(long)e * N];
            lds = mine;         // (this lane's column alone: no barrier)
        }
        ret = sp.s.ret[i];
        eps = sp.s.eps[i];
        stepped = fresh = moved = false;
    }
    // all 64 members have eps == T: rank, log, move the mean, draw the next candidates.  The whole wave is here.
    __device__ __forceinline__ void generation_end() {
        const mdpp_linear_es &s = sp.s;
        const long g = i >> 6, G = N >> 6;
        const int m = (int)(i & 63);
        const bool plus = (m & 1) == 0;
        const double acc = s.acc[i];
        s.fitness[i] = acc;
        const double key = (acc != acc) ? -__builtin_inf() : acc;
        int lt = 0, eq = 0;
#pragma unroll 1
        for (int j = 0; j < 64; j++) {
            const double kj = __shfl(key, j);
            lt += kj < key ? 1 : 0;
            eq += kj == key ? 1 : 0;
        }
        const int r = 2 * lt + (eq - 1) - 63;           // (eq counts the lane itself)
        const int32_t gen = s.gen[g];
        double sum = acc;
#pragma unroll
        for (int k = 0; k < 6; k++) sum = sum + __shfl_xor(sum, 1 << k);
        if (m == 0 && gen < s.log_rows) s.log_mean[(long)gen * G + g] = sum * (1.0 / 64.0);
        const float sg = s.sigma[g], gn = s.gain[g], rf = (float)r;
        const uint64_t id = env0 + (uint64_t)(i & ~1L);        // the even member's id: both members of a pair read one stream
        Philox g0, g1;
        g0.init(s.seed, id, (uint64_t)(uint32_t)gen, kPhiloxLinearEsStream);
        g1.init(s.seed, id, (uint64_t)(uint32_t)(gen + 1), kPhiloxLinearEsStream);
        const long stride = PLDS ? (long)kBlock : N;
        float *c = PLDS ? lds : cand, *mu_p = s.mean + g;
        const int E = D * (HIST * D + 1);
#pragma unroll 1
        for (int e = 0; e < E; e++) {
            const float z0 = (float)g0.normal(), z1 = (float)g1.normal();
            float v = rf * (plus ? z0 : -z0);
#pragma unroll
            for (int k = 0; k < 6; k++) v = v + __shfl_xor(v, 1 << k);
            const float step = gn * v;
            const float mu = *mu_p + step;
            const float t = sg * z1;
            *c = plus ? mu + t : mu - t;
            if (m == 0) *mu_p = mu;
            c += stride; mu_p += G;
        }
        if (m == 0) s.gen[g] = gen + 1;
        s.acc[i] = 0.0;
        ret = 0.0;
        eps = fresh ? 0 : -1;
        moved = true;
    }
    // the group's vote on the step just completed; called where the wave is converged
    __device__ __forceinline__ void vote() {
        if (__all(eps == sp.s.episodes_per_member)) generation_end();
        fresh = false;
    }
    // LinearAgent::act (mdpp_continuous_linear.hip), statement for statement, on the candidate -- after the vote
    __device__ __forceinline__ void act(const float (&o)[DMAX], float (&a)[DMAX]) {
        if (stepped) vote();
        stepped = true;
        const long stride = PLDS ? (long)kBlock : N;
        const long b_off = (long)D * stride;               // row r: W[r][0 .. D-1], then b[r]
        const float *p = PLDS ? lds : cand;
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
    // HIST = 2: the step calls this form (first: no step taken in the env's current episode) -- after the vote, like act() above
    __device__ __forceinline__ void act(const float (&o)[DMAX], float (&a)[DMAX], bool first) {
        if (stepped) vote();
        stepped = true;
        linear_act_h2<DMAX>(PLDS ? lds : cand, PLDS ? (long)kBlock : N, D, amax, o, mem, N, first, a);
    }
    __device__ __forceinline__ void observe(float rw, bool end) {
        const int32_t T = sp.s.episodes_per_member;
        const bool counting = eps >= 0 && eps < T;
        if (counting) ret += (double)rw;
        fresh = end;
        if (!end) return;
        if (counting) { sp.s.acc[i] += ret; ret = 0.0; eps += 1; }
        else if (eps < 0) eps = 0;
    }
    __device__ __forceinline__ void finish(long) {
        if (stepped) vote();
        sp.s.ret[i] = ret;
        sp.s.eps[i] = eps;
        if constexpr (PLDS) {
            if (moved) {
                const int E = D * (HIST * D + 1);
                for (int e = 0; e < E; e++) cand[(long)e * N] = lds[e * kBlock];
            }
        }
    }
};

#if MDPP_CES_TU_SUMMARY
template <int DMAX, int OMAX, bool PHILOX, bool NOISE, bool PLDS MDPP_HIST_TPARAM>
__global__ __launch_bounds__(kBlock) void k_continuous_es_summary(ContinuousArgs a, int K, EsParams sp, EpisodeSummaryArgs sm MDPP_HIST_KPARAM) {
    extern __shared__ __align__(16) float s_theta[];
    EsAgent<DMAX, PLDS, MDPP_LINEAR_HIST> agent;
    MDPP_HIST_SET_MEM(agent, a.N) agent.sp = sp; agent.N = a.N; agent.env0 = (uint64_t)a.env_id_offset; agent.D = a.D; agent.amax = a.amax32; agent.stage = s_theta;
    continuous_closed_rollout<DMAX, OMAX, PHILOX, NOISE, true>(a, K, agent, ContinuousClosedOut{}, sm);
}
#define MDPP_CES_KERNEL k_continuous_es_summary
#define MDPP_CES_NAME "k_continuous_es_summary"
#else
template <int DMAX, int OMAX, bool PHILOX, bool NOISE, bool PLDS MDPP_HIST_TPARAM>
__global__ __launch_bounds__(kBlock) void k_continuous_es_rollout(ContinuousArgs a, int K, EsParams sp, ContinuousClosedOut out MDPP_HIST_KPARAM) {
    extern __shared__ __align__(16) float s_theta[];
    EsAgent<DMAX, PLDS, MDPP_LINEAR_HIST> agent;
    MDPP_HIST_SET_MEM(agent, a.N) agent.sp = sp; agent.N = a.N; agent.env0 = (uint64_t)a.env_id_offset; agent.D = a.D; agent.amax = a.amax32; agent.stage = s_theta;
    continuous_closed_rollout<DMAX, OMAX, PHILOX, NOISE, false>(a, K, agent, out, EpisodeSummaryArgs{});
}
#define MDPP_CES_KERNEL k_continuous_es_rollout
#define MDPP_CES_NAME "k_continuous_es_rollout"
#endif

// One form of this unit's kernel on (padded D, padded order): the placement, the name, the launch
template <int DMAX, int OMAX>
static void launch_es_t(const ContinuousArgs &a, const ContinuousIO &io, const EsParams &sp, float *mem) {
    const long grid = ((long)a.N + kBlock - 1) / kBlock;
    const bool noise = a.has_p_noise || a.has_r_noise;
    const size_t want = (size_t)kBlock * a.D * (MDPP_LINEAR_HIST * a.D + 1) * sizeof(float);
    with_bools([&](auto PH, auto NZ) {
        constexpr bool kPh = decltype(PH)::value, kNz = decltype(NZ)::value;
        const bool plds = !(a.opts & MDPP_OPT_NO_LINEAR_LDS) &&
                          dynamic_lds_ok((const void *)MDPP_CES_KERNEL<DMAX, OMAX, kPh, kNz, true MDPP_HIST_TARG>, want);
        with_bools([&](auto PL) {
            constexpr bool kPl = decltype(PL)::value;
            if (io.name_out) {
                snprintf(io.name_out, kNameLen, MDPP_CES_NAME "<D=%d,ORDER=%d,PHILOX=%d,NOISE=%d,PLDS=%d" MDPP_HIST_NAME ">", DMAX, OMAX, (int)kPh, (int)kNz, (int)kPl);
                return;
            }
            const size_t lds = kPl ? want : 0;
#if MDPP_CES_TU_SUMMARY
            hipLaunchKernelGGL((k_continuous_es_summary<DMAX, OMAX, kPh, kNz, kPl MDPP_HIST_TARG>), dim3((unsigned)grid), dim3(kBlock), lds, io.s, a, io.K, sp, *io.summary MDPP_HIST_KARG);
#else
            // (ContinuousIO::actions is const for the open-loop launchers; the closed-loop launchers WRITE the actions taken there)
            hipLaunchKernelGGL((k_continuous_es_rollout<DMAX, OMAX, kPh, kNz, kPl MDPP_HIST_TARG>), dim3((unsigned)grid), dim3(kBlock), lds, io.s, a, io.K, sp,
                               ContinuousClosedOut{const_cast<float *>(io.actions), io.obs, io.reward, io.term, io.trunc} MDPP_HIST_KARG);
#endif
        }, plds);
    }, a.philox != 0, noise);
}

// the (2,2), (4,2), (12,1) and (12,2) shapes of the linear kernels; false: D > 12 or order > 2
static bool launch_es_dispatch(const ContinuousArgs &a, const ContinuousIO &io, const EsParams &sp, float *mem = nullptr) {
    if (a.order > 2 || a.D > 12) return false;
    if (a.D <= 2) launch_es_t<2, 2>(a, io, sp, mem);
    else if (a.D <= 4) launch_es_t<4, 2>(a, io, sp, mem);
    else if (a.order <= 1) launch_es_t<12, 1>(a, io, sp, mem);
    else launch_es_t<12, 2>(a, io, sp, mem);
    return true;
}

#if MDPP_LINEAR_HIST == 2 && MDPP_CES_TU_SUMMARY
bool launch_continuous_es_summary_h2_form(const ContinuousArgs &a, const ContinuousIO &io, const EsParams &sp, float *mem) {
    return launch_es_dispatch(a, io, sp, mem);
}
#elif MDPP_LINEAR_HIST == 2
bool launch_continuous_es_h2_form(const ContinuousArgs &a, const ContinuousIO &io, const EsParams &sp, float *mem) {
    return launch_es_dispatch(a, io, sp, mem);
}
#elif MDPP_CES_TU_SUMMARY
bool launch_continuous_es_summary_form(const ContinuousArgs &a, const ContinuousIO &io, const EsParams &sp) {
    return launch_es_dispatch(a, io, sp);
}
#else
bool launch_continuous_es_summary_form(const ContinuousArgs &a, const ContinuousIO &io, const EsParams &sp);
bool launch_continuous_es_h2_form(const ContinuousArgs &a, const ContinuousIO &io, const EsParams &sp, float *mem);
bool launch_continuous_es_summary_h2_form(const ContinuousArgs &a, const ContinuousIO &io, const EsParams &sp, float *mem);

// io.K steps of the ES on the handle's per-env linear policy (the caller has checked that there is one and that N % 64 == 0);
// io.summary: the summary form; io.name_out: a dry run, es is not read
int launch_continuous_es(mdpp_env *h, const ContinuousIO &io, const mdpp_linear_es &es) {
    ContinuousArgs a = h->cargs;
    stamp_step(a, h);
    const EsParams sp{es, (float *)h->d_lin_theta};
    float *mem = (float *)h->d_lin_mem;
    const bool summary = io.summary != nullptr;
    const bool served = h->lin_hist == 2 ? (summary ? launch_continuous_es_summary_h2_form(a, io, sp, mem) : launch_continuous_es_h2_form(a, io, sp, mem))
                        : summary        ? launch_continuous_es_summary_form(a, io, sp)
                                         : launch_es_dispatch(a, io, sp);
    if (!served) { h->err = "linear-policy rollouts serve state_space_dim <= 12 and transition_dynamics_order <= 2"; return MDPP_EUNSUPPORTED; }
    return io.name_out ? MDPP_OK : step_done(h, io.K, summary ? "k_continuous_es_summary" : "k_continuous_es_rollout");
}

// mdpp_linear_es_init: the candidates of the current generation, mean +- sigma z with z the normals of tick gen; one lane per env
__global__ __launch_bounds__(kBlock) void k_linear_es_init(mdpp_linear_es s, float *cand, long N, int E, uint64_t env0) {
    const long i = (long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    const long g = i >> 6, G = N >> 6;
    const bool plus = (i & 1) == 0;
    const float sg = s.sigma[g];
    Philox z;
    z.init(s.seed, env0 + (uint64_t)(i & ~1L), (uint64_t)(uint32_t)s.gen[g], kPhiloxLinearEsStream);
    const float *mu_p = s.mean + g;
    float *c = cand + i;
#pragma unroll 1
    for (int e = 0; e < E; e++) {
        const float t = sg * (float)z.normal();
        const float mu = *mu_p;
        *c = plus ? mu + t : mu - t;
        c += N; mu_p += G;
    }
    s.acc[i] = 0.0; s.ret[i] = 0.0; s.eps[i] = 0;
}

int launch_linear_es_init(mdpp_env *h, const mdpp_linear_es &es, hipStream_t s) {
    const long N = h->cfg.num_envs;
    hipLaunchKernelGGL(k_linear_es_init, dim3((unsigned)((N + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, es, (float *)h->d_lin_theta, N,
                       h->cfg.D * (h->lin_hist * h->cfg.D + 1), (uint64_t)h->cfg.env_id_offset);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { h->err = std::string("k_linear_es_init launch: ") + hipGetErrorString(e); return MDPP_EHIP; }
    return MDPP_OK;
}
#endif   // !MDPP_CES_TU_SUMMARY

} // namespace mdpp
