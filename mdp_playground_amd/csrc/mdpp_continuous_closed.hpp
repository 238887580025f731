// The closed-loop step of a continuous move_to_a_point env, stated once: K steps of "an agent forms its action from the state
// the env shows, the env steps" in ONE launch.  k_continuous_linear_rollout / k_continuous_linear_summary
// (mdpp_continuous_linear.hip) are this body, continuous_closed_rollout, around their Agent; k_continuous_search_rollout /
// k_continuous_search_summary (mdpp_continuous_search.hip) around an agent that also searches.
//
// The step restates C1-C8 and R2 of k_continuous_step (mdpp_continuous.hip) with its noise branches, on the same lines of the
// reference's rl_toy_env.py, and leaves out what the closed-loop handles do not have: the line reward, the per-episode noise
// statistics, the image quirk of C4 and final_obs.  The helpers below (c_norm_rel ... c_reset_lane, CRew) are copies of that
// file's, statement for statement: k_continuous_step's translation units do not include this header, so their code is
// untouched.  Like that file this header must be compiled with -ffp-contract=off.
//
// One lane per env, 256-thread workgroups, ContinuousArgs by value.  The step counter is read through tick_now() /
// ring_head_now(), so a launch captured into a HIP graph replays on the counter of the replay.  Every index is 64-bit:
// one launch serves any K and N, there are no pieces.
//
// An Agent is a struct of force-inlined members (no virtual calls, no function pointers):
//   begin(i)              per lane, after the `i >= N` return
//   act(cur, act_out)     the action of this step from the state in the record (cur: the last observation returned for
//                         the env); also called on the reset call of a next-step-autoreset env, where it is written and ignored
//   act(cur, act_out, first)  in its place for an agent with kHist == 2 (a linear policy with memory, mdpp_linear_history.hpp);
//                         first: the env has taken no step in its current episode (the record's step count is 0)
//   kHist                 1 or 2, a static constant
//   observe(rw, end)      once per step that is not a reset call, after the step's float32 reward is final; end: the episode
//                         terminated or was truncated at this step (a same-step reset has already been made: `cur` is the
//                         new episode's first state).  What it changes acts from the next act() on
//   finish(i)             per lane, after the last step
// The agent reads no stream of the env, so the launch leaves the state, every stream, the status words and the step counter
// where mdpp_step_n fed with the same actions leaves them.
//
// NOISE = true: the handle has a transition_noise and / or a reward_noise key (at 0 too: the draws are made).  A template flag,
// so that a noise-free kernel carries no static LDS -- numpy's ziggurat tables (6 KiB) and the [D][256] doubles of a step's
// normals -- and all of a workgroup's LDS is the agent's.
//
// SUMMARY = true: the same K steps with no [K][N] output (mdpp_discrete_closed.hpp's rule, word for word).  The lane loads the
// five values of its env from sm after begin(), applies at every step that is not a reset call
//   ret += (double)reward;  len += 1;  terminated or truncated: episodes += 1, return_sum += ret, length_sum += len, ret = len = 0
// (reward: the float32 the full-output form writes) and stores them after finish().  No atomics: env i's column is this lane's.
#pragma once
#include "mdpp_internal.hpp"
#include "mdpp_rng.hpp"

namespace mdpp {

struct CRew { double v; bool is32; }; // np.float32 vs Python float, as the reference's `reward`

template <int DMAX>
__device__ __forceinline__ float c_norm_rel(const ContinuousArgs &a, const float (&rel)[DMAX], const float (&target)[DMAX]) {
    // np.linalg.norm(rel - target): float32 products, float64 accumulate, one rounding, float32 sqrt
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < DMAX; j++) {
        if (j < a.n_rel) {
            float d = rel[j] - target[j];
            float p = d * d;
            acc += (double)p;
        }
    }
    return sqrtf((float)acc);
}

// The default target (float64 zeros over every dimension, :652-654): sqrt(x.dot(x)) in float64, summed sequentially
template <int DMAX>
__device__ __forceinline__ double c_norm64(const ContinuousArgs &a, const float (&s)[DMAX]) {
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < DMAX; j++) {
        if (j < a.n_rel) {
            const double d = (double)s[j] - 0.0;
            acc += d * d;
        }
    }
    return sqrt(acc);
}

template <int DMAX>
__device__ __forceinline__ bool c_in_box(const ContinuousArgs &a, const float (&rel)[DMAX]) {
    bool any = false;
    for (int b = 0; b < a.n_boxes; b++) {
        bool in = true;
#pragma unroll
        for (int j = 0; j < DMAX; j++) {
            if (j < a.n_rel) {
                float x = rel[j];
                in = in && (x >= a.box_lo[b * a.n_rel + j]) && (x <= a.box_hi[b * a.n_rel + j]);
            }
        }
        any = any || in;
    }
    return any;
}

template <int DMAX>
__device__ __forceinline__ void c_gather_rel(const ContinuousArgs &a, const float (&s)[DMAX],
                                             float (&rel)[DMAX]) {
    // relevant_indices gather with compile-time register indices
    if (a.rel_prefix) { // relevant_indices == [0, 1, ..., n_rel-1]
#pragma unroll
        for (int j = 0; j < DMAX; j++) rel[j] = s[j];
        return;
    }
#pragma unroll
    for (int j = 0; j < DMAX; j++) {
        float v = 0.0f;
        if (j < a.n_rel) {
            const int idx = a.rel[j];
#pragma unroll
            for (int d = 0; d < DMAX; d++) v = (d == idx) ? s[d] : v;
        }
        rel[j] = v;
    }
}

template <int DMAX, int OMAX, class G>
__device__ __forceinline__ void c_reset_lane(const ContinuousArgs &a, G &sp, float (&sd)[OMAX + 1][DMAX],
                                             float (&cur)[DMAX], uint32_t &status) {
    float rel[DMAX];
    for (int tries = 0;; tries++) {
#pragma unroll
        for (int d = 0; d < DMAX; d++) {
            if (d < a.D) {
                double v = a.bounded ? a.reset_lo + a.reset_range * np_random(sp)
                                     : 0.0 + 1.0 * np_standard_normal(sp);
                cur[d] = (float)v;
            }
        }
        if (a.n_boxes == 0) break;
        c_gather_rel<DMAX>(a, cur, rel);
        if (!c_in_box<DMAX>(a, rel)) break;
        if (tries > 4096) { status |= 2u; break; }
    }
#pragma unroll
    for (int k = 0; k <= OMAX; k++)
#pragma unroll
        for (int d = 0; d < DMAX; d++) sd[k][d] = (k == 0) ? cur[d] : 0.0f;
}

// What a full-output launch writes, time-major: the actions taken [K][N][D], observations [K][N][D], rewards and flags [K][N]
struct ContinuousClosedOut {
    float *actions, *obs, *reward;
    uint8_t *term, *trunc;
};

template <int DMAX, int OMAX, bool PHILOX, bool NOISE, bool SUMMARY, class Agent>
__device__ __forceinline__ void continuous_closed_rollout(const ContinuousArgs &a, int K, Agent &agent, const ContinuousClosedOut &out,
                                                          const EpisodeSummaryArgs &sm) {
    const uint64_t ptick0 = tick_now(a);               // the step counter at this launch (through the device-side offset of a graph replay)
    const uint32_t rhead0 = ring_head_now(a, ptick0);    // ... and the head of a delay line kept in memory
    __shared__ uint64_t s_ki[NOISE ? 256 : 1];
    __shared__ double s_wi[NOISE ? 256 : 1], s_fi[NOISE ? 256 : 1];
    __shared__ double s_z[NOISE ? DMAX * kBlock : 1];        // this step's transition-noise normals, [d][lane]
    if (NOISE) { zig_stage(s_ki, s_wi, s_fi, threadIdx.x, kBlock); __syncthreads(); }
    const ZigLds zig{s_ki, s_wi, s_fi};
    const long i = (long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.N) return;
    const int D = a.D, n = a.order;
    const long N = a.N;

    float sd[OMAX + 1][DMAX], cur[DMAX], nxt[DMAX], act[DMAX], rel[DMAX];
#pragma unroll
    for (int k = 0; k <= OMAX; k++)
#pragma unroll
        for (int d = 0; d < DMAX; d++)
            sd[k][d] = (k <= n && d < D) ? a.sd[((long)k * D + d) * N + i] : 0.0f;
#pragma unroll
    for (int d = 0; d < DMAX; d++) cur[d] = (d < D) ? a.cur[(long)d * N + i] : 0.0f;
    uint2 meta = a.meta[i];
    uint32_t steps = meta.x, flags = meta.y, status = 0;
    // next-step autoreset: "episode ended, reset at the next call" travels in bit 1 of the flags word
    const bool next_step = a.autoreset == MDPP_AUTORESET_NEXT_STEP;
    bool pending = next_step && (flags & 2u) != 0;
    flags &= ~2u;

    Pcg64 env_pcg, sp_pcg;
    Philox env_phx, sp_phx;
    bool sp_loaded = false;
    const bool need_env = NOISE && (a.has_p_noise || a.has_r_noise);
    if (!PHILOX && need_env) env_pcg.load(a.env_s, a.env_inc, i);

    agent.begin(i);
    double s_ret = 0.0, s_rsum = 0.0;
    int32_t s_len = 0, s_eps = 0, s_lsum = 0;
    if constexpr (SUMMARY) {
        s_ret = sm.ret[i]; s_len = sm.len[i]; s_eps = sm.episodes[i]; s_rsum = sm.return_sum[i]; s_lsum = sm.length_sum[i];
    }

    // Per-dimension constants pinned in VECTOR registers (as k_continuous_step: left to the compiler they are re-read with
    // scalar loads at every step once the SGPR file is full)
    float tgt[DMAX], smax = a.smax32, amax = a.amax32, inertia = a.inertia32, inv_inertia = a.inv_inertia32, tpw[OMAX + 1];
    double fct[OMAX + 1], ifct[OMAX + 1], pns = a.p_noise;
#pragma unroll
    for (int j = 0; j < DMAX; j++) { tgt[j] = (j < a.n_rel) ? a.target[j] : 0.0f; asm volatile("" : "+v"(tgt[j])); }
#pragma unroll
    for (int j = 0; j <= OMAX; j++) {
        tpw[j] = a.tpow32[j]; fct[j] = a.fact[j]; ifct[j] = a.inv_fact[j];
        asm volatile("" : "+v"(tpw[j]), "+v"(fct[j]), "+v"(ifct[j]));
    }
    asm volatile("" : "+v"(smax), "+v"(amax), "+v"(inertia), "+v"(inv_inertia), "+v"(pns));
    // reset() of this lane (same-step autoreset after a finished episode; next-step: the call after it)
    auto lane_reset = [&]() __attribute__((always_inline)) {
        if (PHILOX) {
            c_reset_lane<DMAX, OMAX>(a, sp_phx, sd, cur, status);
        } else {
            if (!sp_loaded) { sp_pcg.load(a.sp_s, a.sp_inc, i); sp_loaded = true; }
            c_reset_lane<DMAX, OMAX>(a, sp_pcg, sd, cur, status);
        }
        steps = 0; flags = 0;
        if (a.rew64) {
            for (int dd = 0; dd < a.delay; dd++) a.ring64[(size_t)dd * N + i] = 0.0;
        } else {
            for (int dd = 0; dd < a.delay; dd++) a.ring[(size_t)dd * N + i] = kRingPyZero;
        }
    };
    // [env][D] row-major, 16 B per lane per store when possible
    auto put_row = [&](float *base, long o, const float (&v)[DMAX]) __attribute__((always_inline)) {
        float *op = base + o * D;
        if (DMAX % 4 == 0 && D == DMAX) {
#pragma unroll
            for (int q = 0; q < DMAX / 4; q++)
                ((float4 *)op)[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
        } else {
#pragma unroll
            for (int d = 0; d < DMAX; d++) if (d < D) op[d] = v[d];
        }
    };
    for (int k = 0; k < K; k++) {
        const uint32_t tick = rhead0 + (uint32_t)k;              // ring head (mod delay below)
        const uint64_t ptick = ptick0 + (uint64_t)k;
        const long o = (long)k * N + i;
        if (PHILOX) {
            env_phx.init(a.philox_seed, (uint64_t)(a.env_id_offset + i), ptick, MDPP_STREAM_ENV);
            sp_phx.init(a.philox_seed, (uint64_t)(a.env_id_offset + i), ptick, MDPP_STREAM_SPACE);
        }
        // ---- the agent's action, from the state in the record
        if constexpr (Agent::kHist == 2) agent.act(cur, act, steps == 0);
        else agent.act(cur, act);
        if constexpr (!SUMMARY) put_row(out.actions, o, act);
        if (pending) {               // next-step autoreset: this call is the env's reset(), :2284-2323 (the action is ignored)
            lane_reset();
            if constexpr (!SUMMARY) {
                put_row(out.obs, o, cur);
                out.reward[o] = 0.0f; out.term[o] = 0; out.trunc[o] = 0;
            }
            pending = false;
            continue;
        }
        // ---- C1 (a NaN component fails both comparisons)
        bool ok = true;
#pragma unroll
        for (int d = 0; d < DMAX; d++)
            if (d < D) ok = ok && (act[d] >= -amax) && (act[d] <= amax);
        if (ok) {
            // ---- C2: lower orders first, each using the not-yet-updated higher ones
#pragma unroll
            for (int d = 0; d < DMAX; d++) {
#pragma unroll
                for (int kk = 0; kk <= OMAX; kk++)
                    if (kk == n) sd[kk][d] = a.inertia_pow2 ? act[d] * inv_inertia : act[d] / inertia;   // (exact for 2^k)
            }
#pragma unroll
            for (int ii = 0; ii < OMAX; ii++) {
#pragma unroll
                for (int j = 0; j < OMAX; j++) {
                    if (ii < n && j < n - ii) {
#pragma unroll
                        for (int d = 0; d < DMAX; d++) {
                            float prod = sd[(ii + j + 1 <= OMAX) ? ii + j + 1 : OMAX][d] * tpw[(j + 1 <= OMAX) ? j + 1 : OMAX];
                            // 1! and 2! are powers of two: multiplying by the reciprocal is the same float64
                            const double trm = ((a.fact_pow2_mask >> (j + 1)) & 1u)
                                                   ? (double)prod * ifct[(j + 1 <= OMAX) ? j + 1 : OMAX]
                                                   : (double)prod / fct[(j + 1 <= OMAX) ? j + 1 : OMAX];
                            sd[ii][d] = (float)((double)sd[ii][d] + trm);
                        }
                    }
                }
            }
#pragma unroll
            for (int d = 0; d < DMAX; d++) nxt[d] = sd[0][d];
        } else {
            status |= MDPP_STATUS_BAD_ACTION;
#pragma unroll
            for (int d = 0; d < DMAX; d++) nxt[d] = cur[d];
        }
        // ---- C3: the D normals are drawn in a ROLLED loop into this lane's LDS column and added from there
        if constexpr (NOISE) {
            if (a.has_p_noise) {
#pragma unroll 1
                for (int d = 0; d < D; d++)
                    s_z[d * kBlock + threadIdx.x] =
                        0.0 + pns * (PHILOX ? np_standard_normal_lds(env_phx, zig) : np_standard_normal_lds(env_pcg, zig));
            }
        }
#pragma unroll
        for (int d = 0; d < DMAX; d++) {
            if (d < D) {
                double nz = 0.0;
                if constexpr (NOISE) nz = a.has_p_noise ? s_z[d * kBlock + threadIdx.x] : 0.0;
                nxt[d] = (float)((double)nxt[d] + nz);
            }
        }
        // ---- C4
        bool inside = true;
#pragma unroll
        for (int d = 0; d < DMAX; d++)
            if (d < D) inside = inside && (nxt[d] >= -smax) && (nxt[d] <= smax);
        if (!inside) {
#pragma unroll
            for (int d = 0; d < DMAX; d++) {
                float x = nxt[d];
                if (x < -smax) x = -smax;
                if (x > smax) x = smax;
                nxt[d] = x;
            }
#pragma unroll
            for (int kk = 0; kk <= OMAX; kk++)
#pragma unroll
                for (int d = 0; d < DMAX; d++) sd[kk][d] = (kk == 0) ? nxt[d] : 0.0f;
        }
        // ---- C5
        c_gather_rel<DMAX>(a, nxt, rel);
        const float dist_new = a.target64 ? 0.0f : c_norm_rel<DMAX>(a, rel, tgt);
        const double dist_new64 = a.target64 ? c_norm64<DMAX>(a, rel) : 0.0;
        const bool within = a.target64 ? (dist_new64 < a.radius) : (dist_new < a.radius32);
        if (within) flags |= 1u;
        const bool in_box = (a.n_boxes > 0) && c_in_box<DMAX>(a, rel);
        steps += 1;
        // ---- C6
        // :1858: no reward while coordinate 0 of the state this step left is NaN; the reward stays the Python float 0.0 and the
        // action penalty is not subtracted
        const bool nan_gate = cur[0] != cur[0];
        CRew r;
        if (nan_gate) {
            r.v = 0.0; r.is32 = false;
        } else if (a.make_denser && a.target64) {
            float relo[DMAX];
            c_gather_rel<DMAX>(a, cur, relo);
            r.v = -dist_new64;                            // np.float64 (:1926)
            r.v = r.v + c_norm64<DMAX>(a, relo);          // :1929
        } else if (a.make_denser) {
            float relo[DMAX];
            c_gather_rel<DMAX>(a, cur, relo);
            const float dist_old = c_norm_rel<DMAX>(a, relo, tgt);
            r.v = (double)(float)(-dist_new + dist_old);
        } else {
            r.v = within ? 1.0 : 0.0;
        }
        if (!nan_gate) {
            double acc = 0.0;
#pragma unroll
            for (int d = 0; d < DMAX; d++)
                if (d < D) { float p = act[d] * act[d]; acc += (double)p; }
            float pen = a.alw32 * sqrtf((float)acc);      // Python float * np.float32 -> np.float32
            if (a.rew64) { r.v = r.v - (double)pen; r.is32 = false; }      // np.float64 - np.float32
            else { r.v = (double)((float)r.v - pen); r.is32 = true; }
        }
        // ---- C7
        if (a.delay > 0 && a.rew64) {
            double *slot = a.ring64 + (size_t)(tick % (uint32_t)a.delay) * N + i;
            const double outv = *slot;
            *slot = r.v;
            r.v = outv;
        } else if (a.delay > 0) {
            uint32_t *slot = a.ring + (size_t)(tick % (uint32_t)a.delay) * N + i;
            uint32_t bits = *slot;
            *slot = r.is32 ? __float_as_uint((float)r.v) : kRingPyZero;       // (the Python float 0.0 of the NaN gate keeps its type)
            if (bits == kRingPyZero) { r.v = 0.0; r.is32 = false; }
            else { r.v = (double)__uint_as_float(bits); r.is32 = true; }
        }
        if (steps % (uint32_t)a.every_n != 0) { r.v = 0.0; r.is32 = false; }
        if constexpr (NOISE) {
            if (a.has_r_noise) {
                double nz = 0.0 + a.r_noise * (PHILOX ? np_standard_normal_lds(env_phx, zig) : np_standard_normal_lds(env_pcg, zig));
                if (r.is32) r.v = (double)((float)r.v + (float)nz); else r.v = r.v + nz;
            }
        }
        if (r.is32) {
            r.v = (double)((float)r.v * a.scale32);
            r.v = (double)((float)r.v + a.shift32);
        } else {
            r.v = r.v * a.scale;
            r.v = r.v + a.shift;
        }
        // ---- C8
        const bool done = in_box || (flags & 1u);
        if (done) {
            if (r.is32) r.v = (double)((float)r.v + a.term_add32); else r.v = r.v + a.term_add;
        }
#pragma unroll
        for (int d = 0; d < DMAX; d++) cur[d] = nxt[d];
        const bool truncated = (a.max_steps > 0) && (steps >= (uint32_t)a.max_steps);

        if (next_step) pending = done || truncated;
        if (a.autoreset == MDPP_AUTORESET_SAME_STEP && (done || truncated)) lane_reset();
        const float rw = (float)r.v;
        agent.observe(rw, done || truncated);
        if constexpr (SUMMARY) {
            s_ret += (double)rw; s_len += 1;
            if (done || truncated) { s_eps += 1; s_rsum += s_ret; s_lsum += s_len; s_ret = 0.0; s_len = 0; }
        } else {
            // ---- outputs
            put_row(out.obs, o, cur);
            out.reward[o] = rw;
            out.term[o] = done ? 1 : 0;
            out.trunc[o] = truncated ? 1 : 0;
        }
    }
    agent.finish(i);

#pragma unroll
    for (int k = 0; k <= OMAX; k++)
#pragma unroll
        for (int d = 0; d < DMAX; d++)
            if (k <= n && d < D) a.sd[((long)k * D + d) * N + i] = sd[k][d];
#pragma unroll
    for (int d = 0; d < DMAX; d++) if (d < D) a.cur[(long)d * N + i] = cur[d];
    a.meta[i] = make_uint2(steps, flags | (pending ? 2u : 0u));
    if (!PHILOX) {
        if (need_env) env_pcg.store(a.env_s, i);
        if (sp_loaded) sp_pcg.store(a.sp_s, i);
    }
    if constexpr (SUMMARY) {
        sm.ret[i] = s_ret; sm.len[i] = s_len; sm.episodes[i] = s_eps; sm.return_sum[i] = s_rsum; sm.length_sum[i] = s_lsum;
    }
    if (status) atomicOr(&a.status[i], status);
}

} // namespace mdpp
