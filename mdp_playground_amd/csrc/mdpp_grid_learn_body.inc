// The body of the grid learners' kernels (mdpp_grid_learn.hpp), included into each of them: K steps of one lane.  The kernel
// that includes it has the arguments a (GridArgs), p (GridLearnArgs), sc (GridSchedArgs), K, obs, reward, term, trunc, sm
// (EpisodeSummaryArgs), nl (GridNoiseArgs) in scope and the compile-time constants PHILOX, NOISE, QLDS, EVAL, SUMMARY, SCHED, LOG,
// NLEV.  Text included into the kernel, not a function called from it: k_grid_learn_rollout (SCHED = LOG = false) compiles to
// the code it had before the scheduled and logging kernels existed, and the three kernels with NLEV = false to the code they
// had before the per-env noise levels did (tools/compare_code_objects.py).
    static_assert(!EVAL || !(SCHED || LOG), "schedules and the episode log are forms of the learner");
    static_assert(SUMMARY || !LOG, "the episode log is kept by the summary form");
    static_assert(NOISE || !NLEV, "noise levels exist only on handles with a noise key");
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
    double lane_p = 0.0, lane_sigma = 0.0;              // NLEV: this lane's transition_noise and reward_noise (two coalesced 8-byte loads)
    if constexpr (NLEV) { lane_p = nl.p_noise[i]; lane_sigma = nl.r_noise[i]; }
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
    uint32_t sc_base = 0;           // SCHED: row[i] M, where this lane's row starts in the tables
    int32_t sc_ep = 0;              // SCHED: this lane's episode counter
    // SCHED: entry min(ep, M - 1) of the lane's row into E and alpha
    auto sched_lookup = [&]() {
        if constexpr (SCHED) {
            // (compared unsigned: a negative counter, which only mdpp_set_grid_learner_episodes could have put there, clamps too)
            const uint32_t last = (uint32_t)(sc.M - 1);
            const uint32_t at = sc_base + ((uint32_t)sc_ep < last ? (uint32_t)sc_ep : last);
            if (sc.sc_E) E = sc.sc_E[at];                       // (wave-uniform: a table is there or not)
            if (sc.sc_alpha) alpha = sc.sc_alpha[at];
        }
    };
    if constexpr (!EVAL) {
        alpha = p.alpha[i]; gamma = p.gamma[i]; E = p.E[i];
        if constexpr (SCHED) {
            sc_base = (uint32_t)sc.sc_row[i] * (uint32_t)sc.M;
            sc_ep = sc.sc_ep[i];
            sched_lookup();
        }
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
    uint32_t ep_logged = 0;                             // LOG: the episodes the log has seen this env finish
    if constexpr (SUMMARY) {
        ep_ret = sm.ret[i]; ep_len = sm.len[i];
        ep_count = sm.episodes[i]; ep_return_sum = sm.return_sum[i]; ep_length_sum = sm.length_sum[i];
        if constexpr (LOG) ep_logged = (uint32_t)sm.log_count[i];
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
        bool draw_u = NOISE && a.has_p_noise;
        if constexpr (NLEV) draw_u = draw_u && lane_p != 0.0;   // (a lane at p == 0 draws no u: the reference's `if self.transition_noise:`)
        if (draw_u) {                                     // the env re-draws the move from its own action stream
            const double u = PHILOX ? np_random(env_phx) : np_random(env_pcg);
            bool redraw;
            if constexpr (NLEV) redraw = u < lane_p;
            else redraw = u < a.p_noise;
            if (redraw) {
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
            const double z = PHILOX ? np_standard_normal_lds(env_phx, zig) : np_standard_normal_lds(env_pcg, zig);
            double nz;
            if constexpr (NLEV) nz = 0.0 + lane_sigma * z;
            else nz = 0.0 + a.r_noise * z;
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
            if constexpr (SCHED) {   // the episode ended: the schedule moves on for the next step (a carried a' keeps the old E)
                if (done || truncated) {
                    sc_ep += 1;
                    sched_lookup();
                }
            }
        }

        if (next_step) pending = done || truncated;
        if (a.autoreset == MDPP_AUTORESET_SAME_STEP && (done || truncated)) lane_reset();
        put_obs(o);
        if constexpr (SUMMARY) {
            ep_ret += (double)rout;
            ep_len += 1;
            if (done || truncated) {
                if constexpr (LOG) {        // row ep_logged of the episode-major [log_cap][N] arrays, while there is one
                    if (ep_logged < sm.log_cap) {
                        const size_t at = (size_t)ep_logged * N + i;    // (the host keeps log_cap N below 2^31)
                        sm.log_ret[at] = ep_ret;
                        sm.log_len[at] = ep_len;
                    }
                    ep_logged += 1;
                }
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
        if constexpr (LOG) sm.log_count[i] = (int32_t)ep_logged;
    }
    if constexpr (SCHED) sc.sc_ep[i] = sc_ep;
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
