// Linear policy search inside the launch (mdpp_step_n_linear_search; include/mdpp.h "Linear policy search"): every env runs its
// own (1+1)-ES on its own linear policy, around the step of mdpp_continuous_closed.hpp.  The CANDIDATE -- the policy the env acts
// with -- is the handle's linear-policy buffer; the incumbent and the search's seven other per-env values are the caller's arrays.
// This translation unit holds the full-output kernels k_continuous_search_rollout and the launcher;
// mdpp_continuous_summary_search.hip includes it with MDPP_CSRCH_TU_SUMMARY = 1 and holds k_continuous_search_summary.
//
// The rule, at every step that is not a reset call, after the step's float32 reward rw is final (SearchAgent::observe):
//   ret += (double)rw;  terminated or truncated: acc += ret, ret = 0, eps += 1, and at eps == T the trial ends (trial_end)
// Only `ret` is live across steps; acc / eps / trial / score / sigma / accepted are read-modify-written in memory at episode
// ends (the D = 12 step already holds 250 VGPRs).  A trial end walks the E = D (D + 1) entries with two running pointers in a
// ROLLED loop, one normal of Philox stream (seed, env, trial, 18) at a time: on an accept best[e] = cand[e] first, then
// cand[e] = best[e] + sigma z[e], a float32 product and a float32 sum, each rounded (no FMA: -ffp-contract=off).
//
// The candidate's placement is the linear kernels': PLDS = 1, staged once per launch at p_lds[e 256 + tid], rewritten there at
// a trial end (the lane's own column: no barrier) and written back to the buffer by finish() for the lanes whose trial moved;
// PLDS = 0, read at every step and rewritten at a trial end in the buffer itself.
//
// History 2 (include/mdpp.h "Linear policies with memory"): the *_h2.hip units include this file with MDPP_LINEAR_HIST = 2 and hold
// the HIST=2 forms of the two kernels and their launchers, nothing else; the act is mdpp_linear_history.hpp's, and everything
// below that walks the entries walks E = D (HIST D + 1) of them.
#ifndef MDPP_CSRCH_TU_SUMMARY
#define MDPP_CSRCH_TU_SUMMARY 0    // 1: this translation unit holds k_continuous_search_summary (mdpp_continuous_summary_search.hip)
#endif

#include "mdpp_continuous_closed.hpp"
#include "mdpp_linear_history.hpp"

namespace mdpp {

struct SearchParams {
    mdpp_linear_search s;       // the caller's arrays and constants
    float *cand;                // the handle's entry-major buffer: entry e of env i at cand[e N + i]
};

template <int DMAX, bool PLDS, int HIST>
struct SearchAgent {
    static constexpr int kHist = HIST;
    float *mem;                 // HIST = 2: the handle's memory [D][N]; from begin() on component 0 of this lane's
    float *cand;                // entry 0 of this lane in the handle's buffer, entry e at cand[e N]
    float *lds;                 // PLDS = 1: entry 0 of this lane, entry e at lds[e 256]
    float *stage;
    SearchParams sp;
    long N, i;
    uint64_t env0;
    int D;
    float amax;
    double ret;                 // the running return of the candidate's current episode
    bool moved;                 // a trial ended in this launch: the staged candidate is newer than the buffer's
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
        moved = false;
    }
    // LinearAgent::act (mdpp_continuous_linear.hip), statement for statement, on the candidate
    __device__ __forceinline__ void act(const float (&o)[DMAX], float (&a)[DMAX]) const {
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
    // HIST = 2: the step calls this form (first: no step taken in the env's current episode)
    __device__ __forceinline__ void act(const float (&o)[DMAX], float (&a)[DMAX], bool first) const {
        linear_act_h2<DMAX>(PLDS ? lds : cand, PLDS ? (long)kBlock : N, D, amax, o, mem, N, first, a);
    }
    // eps == T: accept or reject the candidate on acc, adapt sigma, draw the next candidate around the incumbent
    __device__ __forceinline__ void trial_end(double acc) {
        const mdpp_linear_search &s = sp.s;
        const bool improved = acc >= s.score[i];           // (false for a NaN acc)
        const int32_t trial = s.trial[i];
        float sg = s.sigma[i];
        if (trial > 0) {
            if (improved) { const float up = sg * s.sigma_up; sg = up < s.sigma_max ? up : s.sigma_max; }
            else sg = sg * s.sigma_down;
            s.sigma[i] = sg;
        }
        if (improved) { s.score[i] = acc; s.accepted[i] += 1; }
        s.trial[i] = trial + 1; s.acc[i] = 0.0; s.eps[i] = 0;
        Philox g;
        g.init(s.seed, env0 + (uint64_t)i, (uint64_t)(uint32_t)(trial + 1), kPhiloxLinearSearchStream);
        const long stride = PLDS ? (long)kBlock : N;
        float *c = PLDS ? lds : cand, *b = s.best + i;
        const int E = D * (HIST * D + 1);
#pragma unroll 1
        for (int e = 0; e < E; e++) {
            float inc;
            if (improved) { inc = *c; *b = inc; } else inc = *b;
            const float z = (float)g.normal();
            const float step = sg * z;
            *c = inc + step;
            c += stride; b += N;
        }
        moved = true;
    }
    __device__ __forceinline__ void observe(float rw, bool end) {
        ret += (double)rw;
        if (!end) return;
        const mdpp_linear_search &s = sp.s;
        const double acc = s.acc[i] + ret;
        const int32_t eps = s.eps[i] + 1;
        ret = 0.0;
        if (eps == s.episodes_per_trial) trial_end(acc);
        else { s.acc[i] = acc; s.eps[i] = eps; }
    }
    __device__ __forceinline__ void finish(long) {
        sp.s.ret[i] = ret;
        if constexpr (PLDS) {
            if (moved) {
                const int E = D * (HIST * D + 1);
                for (int e = 0; e < E; e++) cand[(long)e * N] = lds[e * kBlock];
            }
        }
    }
};

#if MDPP_CSRCH_TU_SUMMARY
template <int DMAX, int OMAX, bool PHILOX, bool NOISE, bool PLDS MDPP_HIST_TPARAM>
__global__ __launch_bounds__(kBlock) void k_continuous_search_summary(ContinuousArgs a, int K, SearchParams sp, EpisodeSummaryArgs sm MDPP_HIST_KPARAM) {
    extern __shared__ __align__(16) float s_theta[];
    SearchAgent<DMAX, PLDS, MDPP_LINEAR_HIST> agent;
    MDPP_HIST_SET_MEM(agent, a.N) agent.sp = sp; agent.N = a.N; agent.env0 = (uint64_t)a.env_id_offset; agent.D = a.D; agent.amax = a.amax32; agent.stage = s_theta;
    continuous_closed_rollout<DMAX, OMAX, PHILOX, NOISE, true>(a, K, agent, ContinuousClosedOut{}, sm);
}
#define MDPP_CSRCH_KERNEL k_continuous_search_summary
#define MDPP_CSRCH_NAME "k_continuous_search_summary"
#else
template <int DMAX, int OMAX, bool PHILOX, bool NOISE, bool PLDS MDPP_HIST_TPARAM>
__global__ __launch_bounds__(kBlock) void k_continuous_search_rollout(ContinuousArgs a, int K, SearchParams sp, ContinuousClosedOut out MDPP_HIST_KPARAM) {
    extern __shared__ __align__(16) float s_theta[];
    SearchAgent<DMAX, PLDS, MDPP_LINEAR_HIST> agent;
    MDPP_HIST_SET_MEM(agent, a.N) agent.sp = sp; agent.N = a.N; agent.env0 = (uint64_t)a.env_id_offset; agent.D = a.D; agent.amax = a.amax32; agent.stage = s_theta;
    continuous_closed_rollout<DMAX, OMAX, PHILOX, NOISE, false>(a, K, agent, out, EpisodeSummaryArgs{});
}
#define MDPP_CSRCH_KERNEL k_continuous_search_rollout
#define MDPP_CSRCH_NAME "k_continuous_search_rollout"
#endif

// One form of this unit's kernel on (padded D, padded order): the placement, the name, the launch
template <int DMAX, int OMAX>
static void launch_search_t(const ContinuousArgs &a, const ContinuousIO &io, const SearchParams &sp, float *mem) {
    const long grid = ((long)a.N + kBlock - 1) / kBlock;
    const bool noise = a.has_p_noise || a.has_r_noise;
    const size_t want = (size_t)kBlock * a.D * (MDPP_LINEAR_HIST * a.D + 1) * sizeof(float);
    with_bools([&](auto PH, auto NZ) {
        constexpr bool kPh = decltype(PH)::value, kNz = decltype(NZ)::value;
        const bool plds = !(a.opts & MDPP_OPT_NO_LINEAR_LDS) &&
                          dynamic_lds_ok((const void *)MDPP_CSRCH_KERNEL<DMAX, OMAX, kPh, kNz, true MDPP_HIST_TARG>, want);
        with_bools([&](auto PL) {
            constexpr bool kPl = decltype(PL)::value;
            if (io.name_out) {
                snprintf(io.name_out, kNameLen, MDPP_CSRCH_NAME "<D=%d,ORDER=%d,PHILOX=%d,NOISE=%d,PLDS=%d" MDPP_HIST_NAME ">", DMAX, OMAX, (int)kPh, (int)kNz, (int)kPl);
                return;
            }
            const size_t lds = kPl ? want : 0;
#if MDPP_CSRCH_TU_SUMMARY
            hipLaunchKernelGGL((k_continuous_search_summary<DMAX, OMAX, kPh, kNz, kPl MDPP_HIST_TARG>), dim3((unsigned)grid), dim3(kBlock), lds, io.s, a, io.K, sp, *io.summary MDPP_HIST_KARG);
#else
            // (ContinuousIO::actions is const for the open-loop launchers; the closed-loop launchers WRITE the actions taken there)
            hipLaunchKernelGGL((k_continuous_search_rollout<DMAX, OMAX, kPh, kNz, kPl MDPP_HIST_TARG>), dim3((unsigned)grid), dim3(kBlock), lds, io.s, a, io.K, sp,
                               ContinuousClosedOut{const_cast<float *>(io.actions), io.obs, io.reward, io.term, io.trunc} MDPP_HIST_KARG);
#endif
        }, plds);
    }, a.philox != 0, noise);
}

// the (2,2), (4,2), (12,1) and (12,2) shapes of the linear kernels; false: D > 12 or order > 2
static bool launch_search_dispatch(const ContinuousArgs &a, const ContinuousIO &io, const SearchParams &sp, float *mem = nullptr) {
    if (a.order > 2 || a.D > 12) return false;
    if (a.D <= 2) launch_search_t<2, 2>(a, io, sp, mem);
    else if (a.D <= 4) launch_search_t<4, 2>(a, io, sp, mem);
    else if (a.order <= 1) launch_search_t<12, 1>(a, io, sp, mem);
    else launch_search_t<12, 2>(a, io, sp, mem);
    return true;
}

#if MDPP_LINEAR_HIST == 2 && MDPP_CSRCH_TU_SUMMARY
bool launch_continuous_search_summary_h2_form(const ContinuousArgs &a, const ContinuousIO &io, const SearchParams &sp, float *mem) {
    return launch_search_dispatch(a, io, sp, mem);
}
#elif MDPP_LINEAR_HIST == 2
bool launch_continuous_search_h2_form(const ContinuousArgs &a, const ContinuousIO &io, const SearchParams &sp, float *mem) {
    return launch_search_dispatch(a, io, sp, mem);
}
#elif MDPP_CSRCH_TU_SUMMARY
bool launch_continuous_search_summary_form(const ContinuousArgs &a, const ContinuousIO &io, const SearchParams &sp) {
    return launch_search_dispatch(a, io, sp);
}
#else
bool launch_continuous_search_summary_form(const ContinuousArgs &a, const ContinuousIO &io, const SearchParams &sp);
bool launch_continuous_search_h2_form(const ContinuousArgs &a, const ContinuousIO &io, const SearchParams &sp, float *mem);
bool launch_continuous_search_summary_h2_form(const ContinuousArgs &a, const ContinuousIO &io, const SearchParams &sp, float *mem);

// io.K steps of the search on the handle's per-env linear policy (the caller has checked that there is one); io.summary: the
// summary form; io.name_out: a dry run, sr is not read
int launch_continuous_search(mdpp_env *h, const ContinuousIO &io, const mdpp_linear_search &sr) {
    ContinuousArgs a = h->cargs;
    stamp_step(a, h);
    const SearchParams sp{sr, (float *)h->d_lin_theta};
    float *mem = (float *)h->d_lin_mem;
    const bool summary = io.summary != nullptr;
    const bool served = h->lin_hist == 2 ? (summary ? launch_continuous_search_summary_h2_form(a, io, sp, mem) : launch_continuous_search_h2_form(a, io, sp, mem))
                        : summary        ? launch_continuous_search_summary_form(a, io, sp)
                                         : launch_search_dispatch(a, io, sp);
    if (!served) { h->err = "linear-policy rollouts serve state_space_dim <= 12 and transition_dynamics_order <= 2"; return MDPP_EUNSUPPORTED; }
    return io.name_out ? MDPP_OK : step_done(h, io.K, summary ? "k_continuous_search_summary" : "k_continuous_search_rollout");
}
#endif   // !MDPP_CSRCH_TU_SUMMARY

} // namespace mdpp
