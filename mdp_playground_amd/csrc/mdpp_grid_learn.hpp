// In-kernel tabular TD learners on GRID envs: one Q-learning or SARSA agent per gridworld, its Q-table beside the env state, K
// steps of "select epsilon-greedily from the env's own Q, step, update that Q" in ONE launch (mdpp_step_n_grid_learn), greedy
// evaluation of those tables (mdpp_step_n_grid_eval) and the forms of both that keep episode summaries instead of [K][N]
// arrays.  include/mdpp.h "Grid learners" is the normative text.
//
// The step is a COPY of the G = 2 path of k_grid_step (mdpp_grid.hip: transition-noise re-draw, clip, target latch, dense /
// sparse reward, every-n mask, reward noise, scale, shift, terminal reward, truncation, the three reset modes), so that the
// open-loop kernels' code objects do not change.  The admission test is gone: the agent's vectors are one-hot or zero by
// construction.  The agent's hooks sit around it like mdpp_discrete_closed.hpp's: select before the step, learn after it and
// before any reset.
//
// The learner of env i (global id g = env_id_offset + i): alpha[i], gamma[i], E[i] = ceil(epsilon[i] 2^31) -- always [N] arrays,
// loaded once per launch -- and Q float32 [S][A], S = (g0 + 1)(g1 + 1), A = 4 or 5.  State index s = c0 (g1 + 1) + c1 (a start
// cell may be the index g, one past the grid).  Action j -> vector: j < 4: component j >> 1 is +1 (j even) or -1 (j odd);
// j == 4: the noop.  sel, target, update and sarsa's carry: mdpp_discrete_learn.hpp's, restated here on this table.
//
// Q lives in a buffer of the handle, entry-major [S A][N]: entry e = s A + j of env i at q[e N + i] (coalesced over lanes).
// QLDS = 1: the lane's table is staged once per launch at q_lds[e 256 + tid] (bank = lane: no conflict whatever entry each
// lane holds) and, unless EVAL, written back after the last step; QLDS = 0: the same indexing on the buffer.  The host
// guarantees N S A 4 < 2^32, so e N + i fits 32 bits.
//
// NOISE = 0 leaves the env's noise streams and numpy's ziggurat out of the kernel; EVAL = 1 leaves the learner's Philox words,
// the parameters and the update out; SUMMARY = 1 writes no [K][N] array and keeps the caller's five [N] episode numbers.
#pragma once
#include "mdpp_internal.hpp"
#include "mdpp_rng.hpp"

namespace mdpp {

// what the kernel takes besides the handle's GridArgs
struct GridLearnArgs {
    float *q;                   // [S A][N] entry-major (device)
    const float *alpha, *gamma; // [N]
    const uint32_t *E;          // [N] ceil(epsilon 2^31): explore iff (wE >> 1) < E
    int32_t *actions;           // [K][N][2] the action vectors taken (out; unused by the summary form)
    uint64_t seed;              // key of the learner's Philox streams
    int32_t algo;               // MDPP_LEARN_Q_LEARNING / MDPP_LEARN_SARSA
    uint32_t A, SA, W;          // actions; entries per table; g1 + 1
};

template <bool PHILOX, bool NOISE, bool QLDS, bool EVAL, bool SUMMARY>
__global__ __launch_bounds__(kBlock) void k_grid_learn_rollout(GridArgs a, GridLearnArgs p, int K, void *__restrict__ obs,
                                                               float *__restrict__ reward, uint8_t *__restrict__ term,
                                                               uint8_t *__restrict__ trunc, EpisodeSummaryArgs sm) {
    const uint64_t ptick0 = tick_now(a);               // the step counter at this launch (through the device-side offset of a graph replay)
    constexpr bool ZIG = NOISE && !PHILOX;             // numpy's ziggurat tables (the Philox normal is Box-Muller)
    __shared__ uint64_t s_ki[ZIG ? 256 : 1];
    __shared__ double s_wi[ZIG ? 256 : 1], s_fi[ZIG ? 256 : 1];
    extern __shared__ __align__(16) float q_dyn[];     // QLDS: [S A][256]
    if (ZIG && a.has_r_noise) { zig_stage(s_ki, s_wi, s_fi, threadIdx.x, kBlock); __syncthreads(); }
    const ZigLds zig{s_ki, s_wi, s_fi};
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= (uint32_t)a.N) return;
    const uint32_t N = (uint32_t)a.N, A = p.A, SA = p.SA, W = p.W;
    const uint64_t genv = (uint64_t)(a.env_id_offset + (int64_t)i);     // global env id (Philox key)
    float *const q_lds = q_dyn + threadIdx.x;
    float *const qg = p.q + i;
    auto qget = [&](uint32_t e) -> float {
        if constexpr (QLDS) return q_lds[e * kBlock];
        else return qg[e * N];
    };
    auto qput = [&](uint32_t e, float v) {
        if constexpr (QLDS) q_lds[e * kBlock] = v;
        else qg[e * N] = v;
    };
    if constexpr (QLDS)
        for (uint32_t e = 0; e < SA; e++) q_lds[e * kBlock] = qg[e * N];

    // ---- the agent (mdpp_discrete_learn.hpp's LearnAgent on this table) ----
    float alpha = 0.0f, gamma = 0.0f;
    uint32_t E = 0;
    uint32_t e_cur[4] = {0, 0, 0, 0}, e_nxt[4] = {0, 0, 0, 0}, x_cur[4] = {0, 0, 0, 0}, x_nxt[4] = {0, 0, 0, 0};
    uint64_t blk_cur = 0;
    bool sarsa = false, have_carry = false;
    uint32_t carried = 0;
    if constexpr (!EVAL) {
        alpha = p.alpha[i]; gamma = p.gamma[i]; E = p.E[i];
        philox_start_block(p.seed, genv, ptick0 >> 2, kPhiloxLearnExploreStream, e_nxt);
        philox_start_block(p.seed, genv, ptick0 >> 2, kPhiloxLearnActionStream, x_nxt);
        sarsa = p.algo == MDPP_LEARN_SARSA;
    }
    // max_j Q[s][j] and the lowest j that attains it (scanned from j = 0 with a strict >)
    auto row_best = [&](uint32_t s, uint32_t &arg) -> float {
        const uint32_t e0 = s * A;
        float best = qget(e0);
        uint32_t bj = 0;
        for (uint32_t j = 1; j < A; j++) {
            const float v = qget(e0 + j);
            if (v > best) { best = v; bj = j; }
        }
        arg = bj;
        return best;
    };
    // sel(s, tick), tick in the current block of the learner's words or the first of the next
    auto select = [&](uint32_t s, uint64_t tick) -> uint32_t {
        if constexpr (!EVAL) {
            const bool in_cur = (tick >> 2) == blk_cur;     // (wave-uniform)
            const uint32_t wE = in_cur ? philox_word_of(e_cur, tick) : philox_word_of(e_nxt, tick);
            if ((wE >> 1) < E) {
                const uint32_t wA = in_cur ? philox_word_of(x_cur, tick) : philox_word_of(x_nxt, tick);
                return (uint32_t)(((uint64_t)wA * (uint64_t)A) >> 32);
            }
        }
        uint32_t j;
        (void)row_best(s, j);
        return j;
    };

    // ---- the env (k_grid_step, G = 2) ----
    const uint4 st = a.state[i];
    int cell0 = (int)(st.x & 0xFF), cell1 = (int)((st.x >> 8) & 0xFF);
    const uint32_t cell_hi = st.x & 0xFFFF0000u;        // (G = 2: zero; kept as found)
    uint32_t steps = st.y, flags = st.z, status = 0;
    // next-step autoreset: "episode ended, reset at the next call" travels in bit 1 of the flags word
    const bool next_step = a.autoreset == MDPP_AUTORESET_NEXT_STEP;
    bool pending = next_step && (flags & 2u) != 0;
    flags &= ~2u;

    Pcg64 env_pcg, sp_pcg, act_pcg;
    Philox env_phx, sp_phx, act_phx;
    Half32 act_h{0, 0}, phx_h{0, 0};
    bool sp_loaded = false;
    const bool need_env = NOISE && (a.has_p_noise || a.has_r_noise);
    if (!PHILOX) {
        if (need_env) env_pcg.load(a.env_s, a.env_inc, i);
        if (NOISE && a.has_p_noise) {
            act_pcg.load(a.act_s, a.act_inc, i);
            const uint2 hh = a.act_half[i];
            act_h = Half32{hh.x, hh.y};
        }
    }
    typedef int i32x2 __attribute__((ext_vector_type(2)));
    typedef long i64x2 __attribute__((ext_vector_type(2)));
    auto put_obs = [&](size_t o) {
        if constexpr (!SUMMARY) {
            if (a.obs_i32) *(i32x2 *)((int32_t *)obs + o * 2) = i32x2{cell0, cell1};
            else *(i64x2 *)((int64_t *)obs + o * 2) = i64x2{(long)cell0, (long)cell1};
        }
    };
    // reset() of this lane: feature_space.sample() of Box(0, grid_shape, int64), floor(uniform(0, g + 1)) per dimension -- the
    // index g, one past the grid, can come out, as in the reference
    auto lane_reset = [&]() __attribute__((always_inline)) {
        if (PHILOX) {
            cell0 = (int)floor(0.0 + ((double)(a.shape[0] + 1) - 0.0) * np_random(sp_phx));
            cell1 = (int)floor(0.0 + ((double)(a.shape[1] + 1) - 0.0) * np_random(sp_phx));
        } else {
            if (!sp_loaded) { sp_pcg.load(a.sp_s, a.sp_inc, i); sp_loaded = true; }
            cell0 = (int)floor(0.0 + ((double)(a.shape[0] + 1) - 0.0) * np_random(sp_pcg));
            cell1 = (int)floor(0.0 + ((double)(a.shape[1] + 1) - 0.0) * np_random(sp_pcg));
        }
        steps = 0; flags = 0;
    };

    double ep_ret = 0.0, ep_return_sum = 0.0;           // SUMMARY: this env's five values
    int32_t ep_len = 0, ep_count = 0, ep_length_sum = 0;
    if constexpr (SUMMARY) {
        ep_ret = sm.ret[i]; ep_len = sm.len[i];
        ep_count = sm.episodes[i]; ep_return_sum = sm.return_sum[i]; ep_length_sum = sm.length_sum[i];
    }

    for (int k = 0; k < K; k++) {
        const uint64_t tick = ptick0 + (uint64_t)k;
        const size_t o = (size_t)k * N + i;
        if constexpr (!EVAL) {
            if (k == 0 || (tick & 3u) == 0u) {          // (wave-uniform) the learner's words of the next four ticks, made ahead
#pragma unroll
                for (int w = 0; w < 4; w++) { e_cur[w] = e_nxt[w]; x_cur[w] = x_nxt[w]; }
                blk_cur = tick >> 2;
                philox_start_block(p.seed, genv, blk_cur + 1u, kPhiloxLearnExploreStream, e_nxt);
                philox_start_block(p.seed, genv, blk_cur + 1u, kPhiloxLearnActionStream, x_nxt);
            }
        }
        if (PHILOX) {
            if (NOISE) {
                env_phx.init(a.philox_seed, genv, tick, MDPP_STREAM_ENV);
                act_phx.init(a.philox_seed, genv, tick, kPhiloxActionStream);
                phx_h = Half32{0, 0};
            }
            sp_phx.init(a.philox_seed, genv, tick, MDPP_STREAM_SPACE);
        }
        const uint32_t cur = (uint32_t)cell0 * W + (uint32_t)cell1;
        const uint32_t action = have_carry ? carried : select(cur, tick);
        have_carry = false;
        // action index -> vector: (+1,0), (-1,0), (0,+1), (0,-1), (0,0)
        const int mv = (action & 1u) ? -1 : 1;
        int act0 = (action >> 1) == 0u ? mv : 0, act1 = (action >> 1) == 1u ? mv : 0;
        if constexpr (!SUMMARY) *(i32x2 *)(p.actions + o * 2) = i32x2{act0, act1};
        if (pending) {               // next-step autoreset: this call is the env's reset(); the action is ignored, nothing is learnt
            lane_reset();
            put_obs(o);
            if constexpr (!SUMMARY) { reward[o] = 0.0f; term[o] = 0; trunc[o] = 0; }
            pending = false;
            continue;
        }
        const int old0 = cell0, old1 = cell1;
        if (NOISE && a.has_p_noise) {                     // the env re-draws the move from its own action stream
            const double u = PHILOX ? np_random(env_phx) : np_random(env_pcg);
            if (u < a.p_noise) {
                for (int tries = 0;; tries++) {
                    const int ind = PHILOX ? np_integers(act_phx, phx_h, 0, 2) : np_integers(act_pcg, act_h, 0, 2);
                    const int val = PHILOX ? np_integers(act_phx, phx_h, 0, 3) : np_integers(act_pcg, act_h, 0, 3);
                    const int n0 = ind == 0 ? val - 1 : 0, n1 = ind == 1 ? val - 1 : 0;
                    if (!(n0 == act0 && n1 == act1)) { act0 = n0; act1 = n1; break; }
                    if (tries > 4096) { status |= MDPP_STATUS_INTERNAL; break; }
                }
            }
        }
        cell0 = min(max(cell0 + act0, 0), a.shape[0] - 1);
        cell1 = min(max(cell1 + act1, 0), a.shape[1] - 1);
        const bool on_target = cell0 == a.target[0] && cell1 == a.target[1];
        if (on_target) flags |= 1u;                           // reached_terminal latches
        steps += 1;
        double r = 0.0;
        if (a.make_denser)
            r += (double)((abs(old0 - a.target[0]) + abs(old1 - a.target[1])) -
                          (abs(cell0 - a.target[0]) + abs(cell1 - a.target[1])));
        else if (on_target) r += 1.0;
        if (a.every_n != 1 && steps % (uint32_t)a.every_n != 0) r = 0.0;
        if (NOISE && a.has_r_noise) {
            const double nz = 0.0 + a.r_noise * (PHILOX ? np_standard_normal_lds(env_phx, zig) : np_standard_normal_lds(env_pcg, zig));
            r += nz;
        }
        r *= a.scale;
        r += a.shift;
        const bool done = (flags & 1u) != 0;
        if (done) r += a.term_add;
        const float rout = (float)r;
        const bool truncated = (a.max_steps > 0) && (steps >= (uint32_t)a.max_steps);

        if constexpr (!EVAL) {       // target from the cell after the move, on Q as it is before this step's update
            const uint32_t nxt = (uint32_t)cell0 * W + (uint32_t)cell1;
            float y = rout;
            uint32_t a2 = 0;
            if (!done) {
                float qn;
                if (sarsa) {                                  // (wave-uniform)
                    a2 = select(nxt, tick + 1u);
                    qn = qget(nxt * A + a2);
                } else {
                    qn = row_best(nxt, a2);
                }
                const float g = gamma * qn;
                y = rout + g;
            }
            const uint32_t e = cur * A + action;
            const float q = qget(e);
            const float d = y - q;
            const float u = alpha * d;
            qput(e, q + u);
            // sarsa: the next step of this call takes a' when it starts from s' (a truncation that resets drops it)
            have_carry = sarsa && !done && !(truncated && a.autoreset != MDPP_AUTORESET_DISABLED);
            carried = a2;
        }

        if (next_step) pending = done || truncated;
        if (a.autoreset == MDPP_AUTORESET_SAME_STEP && (done || truncated)) lane_reset();
        put_obs(o);
        if constexpr (SUMMARY) {
            ep_ret += (double)rout;
            ep_len += 1;
            if (done || truncated) {
                ep_count += 1;
                ep_return_sum += ep_ret;
                ep_length_sum += ep_len;
                ep_ret = 0.0; ep_len = 0;
            }
        } else {
            reward[o] = rout;
            term[o] = done ? 1 : 0;
            trunc[o] = truncated ? 1 : 0;
        }
    }

    if constexpr (QLDS && !EVAL)
        for (uint32_t e = 0; e < SA; e++) qg[e * N] = q_lds[e * kBlock];
    if constexpr (SUMMARY) {
        sm.ret[i] = ep_ret; sm.len[i] = ep_len;
        sm.episodes[i] = ep_count; sm.return_sum[i] = ep_return_sum; sm.length_sum[i] = ep_length_sum;
    }
    a.state[i] = make_uint4((uint32_t)cell0 | ((uint32_t)cell1 << 8) | cell_hi, steps, flags | (pending ? 2u : 0u), 0u);
    if (!PHILOX) {
        if (need_env) env_pcg.store(a.env_s, i);
        if (sp_loaded) sp_pcg.store(a.sp_s, i);
        if (NOISE && a.has_p_noise) {
            act_pcg.store(a.act_s, i);
            a.act_half[i] = make_uint2(act_h.has32, act_h.u32);
        }
    }
    if (status) atomicOr(&a.status[i], status);
}

// K steps of one output form (SUMMARY: io.summary's five arrays instead of the [K][N] ones) of the learner or (eval) of greedy
// evaluation; a dry run (io.name_out) writes the kernel's name and launches nothing.  QLDS where the device grants the
// workgroup's tables beside the static LDS and MDPP_OPT_NO_GRID_QLDS does not forbid it
template <bool SUMMARY>
int launch_grid_learn_form(mdpp_env *h, const DiscreteIO &io, bool eval) {
    GridArgs a = h->gargs;
    stamp_step(a, h);
    const uint32_t S = (uint32_t)(a.shape[0] + 1) * (uint32_t)(a.shape[1] + 1), A = (uint32_t)h->gl_A;
    const GridLearnArgs p{(float *)h->d_gl_q, (const float *)h->d_gl_alpha, (const float *)h->d_gl_gamma, (const uint32_t *)h->d_gl_E,
                          const_cast<int32_t *>(io.actions), h->gl_seed, h->gl_algo, A, S * A, (uint32_t)(a.shape[1] + 1)};
    const int grid = (a.N + kBlock - 1) / kBlock;
    const size_t q_bytes = (size_t)kBlock * S * A * sizeof(float);
    const bool noise = a.has_p_noise != 0 || a.has_r_noise != 0;
    const EpisodeSummaryArgs sm = SUMMARY ? *io.summary : EpisodeSummaryArgs{};
    with_bools([&](auto PH, auto NZ, auto EV) {
        const bool ql = !(a.opts & MDPP_OPT_NO_GRID_QLDS) &&
                        dynamic_lds_ok((const void *)k_grid_learn_rollout<PH(), NZ(), true, EV(), SUMMARY>, q_bytes);
        with_bools([&](auto QL) {
            if (io.name_out)
                snprintf(io.name_out, kNameLen, "k_grid_learn_rollout<PHILOX=%d,NOISE=%d,QLDS=%d,EVAL=%d,SUMMARY=%d>", PH(), NZ(), QL(), EV(), SUMMARY ? 1 : 0);
            else
                hipLaunchKernelGGL((k_grid_learn_rollout<PH(), NZ(), QL(), EV(), SUMMARY>), dim3(grid), dim3(kBlock), QL() ? q_bytes : 0, io.s,
                                   a, p, io.K, io.obs, io.reward, io.term, io.trunc, sm);
        }, ql);
    }, a.philox != 0, noise, eval);
    return io.name_out ? MDPP_OK : step_done(h, io.K, "k_grid_learn_rollout");
}
extern template int launch_grid_learn_form<false>(mdpp_env *, const DiscreteIO &, bool);    // mdpp_grid_learn.hip
extern template int launch_grid_learn_form<true>(mdpp_env *, const DiscreteIO &, bool);     // mdpp_grid_summary_learn.hip

} // namespace mdpp
