// Eligibility traces for the in-kernel tabular learners: SARSA(lambda) and Watkins's Q(lambda) (include/mdpp.h "Eligibility
// traces"; mdpp_set_learner_traces).  The agent of mdpp_discrete_learn.hpp with a second table Z [S][A] per env beside Q and
// the one-step update replaced by "cut, mark, sweep":
//   q = Q[s][a];  d = y - q;  u = alpha d;                   (y: LearnAgent's target, on Q before anything is written)
//   cut    q_learning, the action came from the explore branch of sel: Z = +0 everywhere
//   mark   accumulating Z[s][a] += 1.0f;  replacing Z[s][a] = 1.0f
//   sweep  e = 0 .. S A - 1 ascending:  z = Z[e];  Q[e] = Q[e] + u z;  Z[e] = c z        (c = gamma lambda, formed in begin())
//   end    terminated or truncated (episode_end(true)): Z = +0, after the sweep
// float32, one rounding per operation (the units are built with -ffp-contract=off), denormals kept.
//
// TraceAgent holds a LearnAgent<QLDS, PE, false, SCHED> and uses its members as they are: the Philox blocks made one ahead,
// select (sel), row_best, the PE registers, the schedule's lookup, SARSA's carry, Q's staging and write-back.  The target's
// few lines are written out again in learn(): LearnAgent::learn forms the target and applies the one-step update in one
// function, and taking it apart would touch the source of every learner kernel that exists.
//
// Z lies behind Q, in LDS as in the buffers: QLDS = 1 stages entry e of this lane's Z at z_lds[e 256] (bank = lane, like Q:
// no conflict whatever entry each lane holds) and writes both tables back in finish(); QLDS = 0 is the same indexing on the
// two buffers, entry e at [e N].  launch_closed_form's placement sees TABLES = 2 and decides QLDS for both.
//
// The sweep is 2 S A LDS reads and 2 S A LDS writes per step per lane and nothing else in the step comes near it.  It runs
// over the flat table in chunks of 8 entries -- a row at A = 8 -- each written as eight independent reads of Z, eight of Q,
// then the arithmetic, then eight writes of Q and eight of Z, so that the reads of a chunk are in flight together and the
// compiler pairs reads and writes of one table into ds_read2st64_b32 / ds_write2st64_b32 (a lane's entries are 1 KiB apart:
// 4 x 64 dwords; written entry by entry the writes stay single and the launch takes 5 % longer: DESIGN.md 3.29); it is not
// unrolled for S A, which would put the whole table into registers.  The cut is folded into the sweep's read (z = cut ? +0 : Z[e], a select per entry instead of S A more LDS
// writes on most steps of most waves -- some lane of a wave nearly always explores), the marked entry written after it
// from the registers that hold q, u and c: with Z = +0 but at (s, a), the rule's sweep leaves Q[e] + u (+0) and c (+0) = +0
// everywhere else, which is what the folded loop writes, and Q[s][a] = q + u 1.0f, Z[s][a] = c 1.0f.
//
// The kind is a run-time, wave-uniform field of the argument block (one select at the mark): a template parameter would
// double the 96 kernels for nothing.  Forms: <PE, SUMMARY, SCHED>, six translation units (mdpp_discrete_trace*.hip, mdpp_discrete_summary_trace*.hip);
// with one MDP per env <PE = 1, SUMMARY, SCHED> x PM = 1 | 2, four more (mdpp_discrete_lambda_pe_pm*.hip, mdpp_discrete_summary_lambda_pe_pm*.hip:
// named apart from the six, whose list a test of the shared-MDP traces pins by the word in their names).
#pragma once
#include "mdpp_discrete_learn.hpp"

namespace mdpp {

// what a trace kernel takes besides the handle's DiscreteArgs: the learner's block and the traces'
struct TraceTail {
    float *z;                   // [S A][N] entry-major (device)
    const float *pe_lambda;     // PE: [N] (device)
    float lambda;               // ... else the uniform one
    int32_t kind;               // MDPP_TRACE_*
};
template <bool PE, bool SCHED>
struct TraceArgs {
    LearnArgsOf<PE, false, SCHED> l;
    TraceTail t;
};

template <bool QLDS, bool PE, bool SCHED>
struct TraceAgent {
    LearnAgent<QLDS, PE, false, SCHED> base;
    const TraceTail &t;
    float *z_lds;               // this lane's column of the workgroup's Z-tables: entry e at z_lds[e 256]
    float *zg;                  // this lane's Z in the buffer: entry e at zg[e N]
    float c;                    // gamma lambda
    bool accumulating, explored;

    __device__ __forceinline__ float zget(uint32_t e) const {
        if constexpr (QLDS) return z_lds[e * kBlock];
        else return zg[(size_t)e * base.N];
    }
    __device__ __forceinline__ void zput(uint32_t e, float v) {
        if constexpr (QLDS) z_lds[e * kBlock] = v;
        else zg[(size_t)e * base.N] = v;
    }
    __device__ __forceinline__ void stage(int) {}
    __device__ __forceinline__ void begin(uint32_t i, uint64_t genv, uint64_t ptick0) {
        base.begin(i, genv, ptick0);
        zg = t.z + i;
        float lambda;
        if constexpr (PE) lambda = t.pe_lambda[i];
        else lambda = t.lambda;
        c = base.gamma() * lambda;
        accumulating = t.kind == MDPP_TRACE_ACCUMULATING;       // (wave-uniform)
        explored = false;
        if (QLDS)
            for (uint32_t e = 0; e < base.SA; e++) z_lds[e * kBlock] = zg[(size_t)e * base.N];
    }
    __device__ __forceinline__ void next_block(uint64_t genv, uint64_t ptick) { base.next_block(genv, ptick); }
    // sel's explore-or-not at a tick of the current block
    __device__ __forceinline__ bool explores(uint64_t tick) const {
        const bool in_cur = (tick >> 2) == base.blk_cur;        // (wave-uniform)
        const uint32_t wE = in_cur ? philox_word_of(base.e_cur, tick) : philox_word_of(base.e_nxt, tick);
        return (wE >> 1) < base.E();
    }
    __device__ __forceinline__ uint32_t act(uint32_t cur, uint64_t ptick) {
        explored = explores(ptick);         // (read by q_learning's cut only, which carries no action: this step did select)
        return base.act(cur, ptick);
    }
    __device__ __forceinline__ void zero_traces() {
        for (uint32_t e = 0; e < base.SA; e++) zput(e, 0.0f);
    }
    __device__ __forceinline__ void learn(uint32_t cur, uint32_t action, uint32_t nxt, float rout, bool done, bool truncated_with_reset, uint64_t ptick) {
        const uint32_t A = base.A, SA = base.SA;
        // the target, as LearnAgent::learn forms it
        float y = rout;
        uint32_t a2 = 0;
        if (!done) {
            float qn;
            if (base.sarsa) {                                                       // (wave-uniform)
                a2 = base.select(nxt, ptick + 1u);
                qn = base.qget(nxt * A + a2);
            } else {
                qn = base.row_best(nxt, a2);
            }
            const float g = base.gamma() * qn;
            y = rout + g;
        }
        const uint32_t sa = cur * A + action;
        const float q = base.qget(sa);
        const float d = y - q;
        const float u = base.alpha() * d;
        const bool cut = !base.sarsa && explored;
        // mark (a cut lane's marked entry is written after the sweep)
        if (!cut) zput(sa, accumulating ? zget(sa) + 1.0f : 1.0f);
        // sweep, the cut folded into its read
        uint32_t e = 0;
        for (; e + 8u <= SA; e += 8u) {
            float z[8], w[8];
#pragma unroll
            for (int j = 0; j < 8; j++) z[j] = zget(e + j);
#pragma unroll
            for (int j = 0; j < 8; j++) w[j] = base.qget(e + j);
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const float zj = cut ? 0.0f : z[j];
                const float uz = u * zj;
                w[j] = w[j] + uz;
                z[j] = c * zj;
            }
#pragma unroll
            for (int j = 0; j < 8; j++) base.qput(e + j, w[j]);
#pragma unroll
            for (int j = 0; j < 8; j++) zput(e + j, z[j]);
        }
        for (; e < SA; e++) {
            const float ze = zget(e);
            const float zj = cut ? 0.0f : ze;
            const float uz = u * zj;
            base.qput(e, base.qget(e) + uz);
            zput(e, c * zj);
        }
        if (cut) {
            const float uz = u * 1.0f;
            base.qput(sa, q + uz);
            zput(sa, c * 1.0f);
        }
        // sarsa: the next step of this call takes a' when it starts from s'
        base.have_carry = base.sarsa && !done && !truncated_with_reset;
        base.carried = a2;
    }
    __device__ __forceinline__ void episode_end(bool ended) {
        base.episode_end(ended);
        if (ended) zero_traces();
    }
    __device__ __forceinline__ void finish(uint32_t i) {
        base.finish(i);
        if (QLDS)
            for (uint32_t e = 0; e < base.SA; e++) zg[(size_t)e * base.N] = z_lds[e * kBlock];
    }
};

template <bool QLDS, bool PE, bool SCHED>
__device__ __forceinline__ TraceAgent<QLDS, PE, SCHED> trace_agent(const DiscreteArgs &a, const TraceArgs<PE, SCHED> &p, unsigned char *lds) {
    const uint32_t SA = (uint32_t)a.S * (uint32_t)a.A;
    float *const q_lds = (float *)(lds + closed_agent_lds_offset<0>(a)) + threadIdx.x;
    return TraceAgent<QLDS, PE, SCHED>{LearnAgent<QLDS, PE, false, SCHED>{p.l, q_lds, (uint32_t)a.A, SA, (uint32_t)a.N}, p.t, q_lds + (size_t)SA * kBlock};
}

template <bool PHILOX, bool NOISE, bool UNIT, bool QLDS, bool PE = false, bool SCHED = false>
__global__ __launch_bounds__(kBlock) void k_discrete_trace_rollout(DiscreteArgs a, TraceArgs<PE, SCHED> p, int K,
                                                                   void *__restrict__ obs,
                                                                   float *__restrict__ reward,
                                                                   uint8_t *__restrict__ term,
                                                                   uint8_t *__restrict__ trunc) {
    extern __shared__ __align__(16) unsigned char lds[];
    const ZigLds zig = closed_loop_zig_lds<NOISE>();
    auto agent = trace_agent<QLDS, PE, SCHED>(a, p, lds);
    closed_loop_rollout<PHILOX, NOISE, UNIT>(a, K, !a.obs_i32, p.l.actions, obs, reward, term, trunc, lds, zig, agent);
}

// ... keeping episode summaries instead of writing the [K][N] arrays (p.l.actions is unused)
template <bool PHILOX, bool NOISE, bool UNIT, bool QLDS, bool PE = false, bool SCHED = false>
__global__ __launch_bounds__(kBlock) void k_discrete_trace_summary(DiscreteArgs a, TraceArgs<PE, SCHED> p, int K, EpisodeSummaryArgs sm) {
    extern __shared__ __align__(16) unsigned char lds[];
    const ZigLds zig = closed_loop_zig_lds<NOISE>();
    auto agent = trace_agent<QLDS, PE, SCHED>(a, p, lds);
    closed_loop_rollout<PHILOX, NOISE, UNIT, true>(a, K, false, nullptr, nullptr, nullptr, nullptr, nullptr, lds, zig, agent, sm);
}

// ... and an episode log beside them (sm.log_cap != 0)
template <bool PHILOX, bool NOISE, bool UNIT, bool QLDS, bool PE = false, bool SCHED = false>
__global__ __launch_bounds__(kBlock) void k_discrete_trace_summary_log(DiscreteArgs a, TraceArgs<PE, SCHED> p, int K, EpisodeSummaryArgs sm) {
    extern __shared__ __align__(16) unsigned char lds[];
    const ZigLds zig = closed_loop_zig_lds<NOISE>();
    auto agent = trace_agent<QLDS, PE, SCHED>(a, p, lds);
    closed_loop_rollout<PHILOX, NOISE, UNIT, true, false, 0, true>(a, K, false, nullptr, nullptr, nullptr, nullptr, nullptr, lds, zig, agent, sm);
}

// PM = 1 / 2 (one MDP per env, mdpp_learner_traces_per_env_mdp): the same agent around the step's PM form, Q and Z behind the
// envs' MDP slots and the shared noise cdf (closed_agent_lds_offset<PM>), as the traceless PM learners place Q.  Overloads
// with PM as a seventh template argument and not a defaulted parameter of the three above: a template argument is spelled
// out in a kernel's mangled name, and the shared-MDP kernels keep their symbols and their code.  PE = 1 always: a handle with
// one MDP per env runs the PE learner.
template <int PM, bool QLDS, bool PE, bool SCHED>
__device__ __forceinline__ TraceAgent<QLDS, PE, SCHED> trace_agent_pm(const DiscreteArgs &a, const TraceArgs<PE, SCHED> &p, unsigned char *lds) {
    const uint32_t SA = (uint32_t)a.S * (uint32_t)a.A;
    float *const q_lds = (float *)(lds + closed_agent_lds_offset<PM>(a)) + threadIdx.x;
    return TraceAgent<QLDS, PE, SCHED>{LearnAgent<QLDS, PE, false, SCHED>{p.l, q_lds, (uint32_t)a.A, SA, (uint32_t)a.N}, p.t, q_lds + (size_t)SA * kBlock};
}

template <bool PHILOX, bool NOISE, bool UNIT, bool QLDS, bool PE, bool SCHED, int PM>
__global__ __launch_bounds__(kBlock) void k_discrete_trace_rollout(DiscreteArgs a, TraceArgs<PE, SCHED> p, int K,
                                                                   void *__restrict__ obs,
                                                                   float *__restrict__ reward,
                                                                   uint8_t *__restrict__ term,
                                                                   uint8_t *__restrict__ trunc) {
    static_assert(PE && (PM == 1 || PM == 2), "one MDP per env runs the PE learner around the step's PM form");
    extern __shared__ __align__(16) unsigned char lds[];
    const ZigLds zig = closed_loop_zig_lds<NOISE>();
    auto agent = trace_agent_pm<PM, QLDS, PE, SCHED>(a, p, lds);
    closed_loop_rollout<PHILOX, NOISE, UNIT, false, false, PM>(a, K, !a.obs_i32, p.l.actions, obs, reward, term, trunc, lds, zig, agent);
}

template <bool PHILOX, bool NOISE, bool UNIT, bool QLDS, bool PE, bool SCHED, int PM>
__global__ __launch_bounds__(kBlock) void k_discrete_trace_summary(DiscreteArgs a, TraceArgs<PE, SCHED> p, int K, EpisodeSummaryArgs sm) {
    static_assert(PE && (PM == 1 || PM == 2), "one MDP per env runs the PE learner around the step's PM form");
    extern __shared__ __align__(16) unsigned char lds[];
    const ZigLds zig = closed_loop_zig_lds<NOISE>();
    auto agent = trace_agent_pm<PM, QLDS, PE, SCHED>(a, p, lds);
    closed_loop_rollout<PHILOX, NOISE, UNIT, true, false, PM>(a, K, false, nullptr, nullptr, nullptr, nullptr, nullptr, lds, zig, agent, sm);
}

template <bool PHILOX, bool NOISE, bool UNIT, bool QLDS, bool PE, bool SCHED, int PM>
__global__ __launch_bounds__(kBlock) void k_discrete_trace_summary_log(DiscreteArgs a, TraceArgs<PE, SCHED> p, int K, EpisodeSummaryArgs sm) {
    static_assert(PE && (PM == 1 || PM == 2), "one MDP per env runs the PE learner around the step's PM form");
    extern __shared__ __align__(16) unsigned char lds[];
    const ZigLds zig = closed_loop_zig_lds<NOISE>();
    auto agent = trace_agent_pm<PM, QLDS, PE, SCHED>(a, p, lds);
    closed_loop_rollout<PHILOX, NOISE, UNIT, true, false, PM, true>(a, K, false, nullptr, nullptr, nullptr, nullptr, nullptr, lds, zig, agent, sm);
}

// One form of the trace learner, as launch_closed_form (mdpp_discrete_closed.hpp) takes it
template <bool PE, bool SUMMARY_, bool SCHED>
struct TraceForm {
    static_assert(!SCHED || PE, "a schedule runs the PE learner");
    static constexpr bool SUMMARY = SUMMARY_, NLEV = false, LOG = SUMMARY_;
    static constexpr int TABLES = 2;        // Q and Z
    using Args = TraceArgs<PE, SCHED>;
    template <bool PH, bool NZ, bool UNIT, bool QL, int PM>
    static constexpr auto kernel() {
        static_assert(PM == 0 || PE, "one MDP per env runs the PE learner");
        // (the casts pick the overload: with PM, or the shared MDP's six arguments)
        if constexpr (PM != 0) {
            if constexpr (SUMMARY) return static_cast<void (*)(DiscreteArgs, Args, int, EpisodeSummaryArgs)>(k_discrete_trace_summary<PH, NZ, UNIT, QL, PE, SCHED, PM>);
            else return static_cast<void (*)(DiscreteArgs, Args, int, void *, float *, uint8_t *, uint8_t *)>(k_discrete_trace_rollout<PH, NZ, UNIT, QL, PE, SCHED, PM>);
        } else {
            if constexpr (SUMMARY) return static_cast<void (*)(DiscreteArgs, Args, int, EpisodeSummaryArgs)>(k_discrete_trace_summary<PH, NZ, UNIT, QL, PE, SCHED>);
            else return static_cast<void (*)(DiscreteArgs, Args, int, void *, float *, uint8_t *, uint8_t *)>(k_discrete_trace_rollout<PH, NZ, UNIT, QL, PE, SCHED>);
        }
    }
    template <bool PH, bool NZ, bool UNIT, bool QL, int PM>
    static constexpr auto kernel_log() {
        static_assert(SUMMARY, "the episode log is kept by the summary form");
        if constexpr (PM != 0) return static_cast<void (*)(DiscreteArgs, Args, int, EpisodeSummaryArgs)>(k_discrete_trace_summary_log<PH, NZ, UNIT, QL, PE, SCHED, PM>);
        else return static_cast<void (*)(DiscreteArgs, Args, int, EpisodeSummaryArgs)>(k_discrete_trace_summary_log<PH, NZ, UNIT, QL, PE, SCHED>);
    }
    static void name(char *out, int ph, int nz, int unit, int ql, int pm) {
        char pmtxt[16] = "";
        if (pm) snprintf(pmtxt, sizeof pmtxt, ",PM=%d", pm);
        snprintf(out, kNameLen, "%s<PHILOX=%d,NOISE=%d,UNIT=%d,QLDS=%d%s%s%s>", SUMMARY ? "k_discrete_trace_summary" : "k_discrete_trace_rollout",
                 ph, nz, unit, ql, PE ? ",PE=1" : "", pmtxt, SCHED ? ",SCHED=1" : "");
    }
    static Args args(const mdpp_env *h, const DiscreteIO &io, int k0, int kc, int32_t *actions, uint32_t cdf_lds) {
        const TraceTail t{(float *)h->d_trace_z, (const float *)h->d_trace_lambda, h->trace_lambda, h->trace_kind};
        return Args{LearnForm<PE, false, SUMMARY_, false, SCHED>::args(h, io, k0, kc, actions, cdf_lds), t};
    }
};

// K learning steps of one form of a handle with traces
template <bool PE, bool SUMMARY, bool SCHED>
int launch_trace_form(mdpp_env *h, const DiscreteIO &io) {
    return launch_closed_form<TraceForm<PE, SUMMARY, SCHED>, false>(h, io);
}

// K learning steps of one form of a handle with traces and one MDP per env (mdpp_learner_traces_per_env_mdp): the PE form's
// PM = 1 and PM = 2 kernels; closed_agent_lds places Q + Z (TABLES = 2) and the envs' MDP slots together.  SCHED: with a
// per-episode schedule in force (mdpp_learner_schedule_sweep)
template <bool SUMMARY, bool SCHED>
int launch_trace_form_pm(mdpp_env *h, const DiscreteIO &io) {
    // (the queue of start states drawn ahead needs shared tables: the PM kernels do not carry it)
    if (h->dargs.fast_ok || h->dargs.shared_tables) { h->err = "mdpp_step_n_learn: eligibility traces: one MDP per env: the handle has shared tables"; return MDPP_ESTATE; }
    return launch_closed_form<TraceForm<true, SUMMARY, SCHED>, true>(h, io);
}

// the forms built <PE, SUMMARY, SCHED> and, with one MDP per env, <SUMMARY, SCHED>, each defined (an explicit instantiation) in the translation unit named
extern template int launch_trace_form<false, false, false>(mdpp_env *, const DiscreteIO &);     // mdpp_discrete_trace.hip
extern template int launch_trace_form<true, false, false>(mdpp_env *, const DiscreteIO &);      // mdpp_discrete_trace_pe.hip
extern template int launch_trace_form<false, true, false>(mdpp_env *, const DiscreteIO &);      // mdpp_discrete_summary_trace.hip
extern template int launch_trace_form<true, true, false>(mdpp_env *, const DiscreteIO &);       // mdpp_discrete_summary_trace_pe.hip
extern template int launch_trace_form<true, false, true>(mdpp_env *, const DiscreteIO &);       // mdpp_discrete_trace_pe_sched.hip
extern template int launch_trace_form<true, true, true>(mdpp_env *, const DiscreteIO &);        // mdpp_discrete_summary_trace_pe_sched.hip
extern template int launch_trace_form_pm<false, false>(mdpp_env *, const DiscreteIO &);         // mdpp_discrete_lambda_pe_pm.hip
extern template int launch_trace_form_pm<true, false>(mdpp_env *, const DiscreteIO &);          // mdpp_discrete_summary_lambda_pe_pm.hip
extern template int launch_trace_form_pm<false, true>(mdpp_env *, const DiscreteIO &);          // mdpp_discrete_lambda_pe_pm_sched.hip
extern template int launch_trace_form_pm<true, true>(mdpp_env *, const DiscreteIO &);           // mdpp_discrete_summary_lambda_pe_pm_sched.hip

} // namespace mdpp
