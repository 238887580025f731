// The E role (state recurrence) of k_discrete_rollout_lean: included once into the kernel's body by mdpp_discrete_lean.hip --
// first, ahead of the other roles' set-up, in every unit but the numpy-noise one, which keeps it last (see there).
#if MDPP_LEAN_TU_NOISE != 2
    const uint32_t ie = i < N ? i : N - 1u;
    const uint4 st0 = a.state[ie];
    auto r_act = __builtin_amdgcn_make_buffer_rsrc((void *)actions, 0, total * 4u * (uint32_t)kEN, kPRsrc);
    const uint32_t v4 = ie * 4u * (uint32_t)kEN;
    auto load_act = [&](int k) -> Act {
        const uint32_t kk = (uint32_t)min(k, K - 1);
        if constexpr (IRR) {
            const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(r_act, v4, kk * N * 8u, MDPP_LEAN_LD_AUX);
            return make_uint2(v.x, v.y);
        } else {
            return __builtin_amdgcn_raw_buffer_load_b32(r_act, v4, kk * N * 4u, MDPP_LEAN_LD_AUX);
        }
    };
    // Actions are fetched kAhead chunks ahead of their use, columns one chunk ahead.  The buffers rotate
    // by NAME (the chunk loop is unrolled kAhead times): copying a register whose load is still in
    // flight makes the wave wait for it, which would put one HBM latency into every chunk.
    constexpr int kAh = IRR ? 2 : kAhead;      // (action pairs: half the depth, for registers)
    static_assert(kAh % 2 == 0, "the column double buffer alternates with the chunk index");
    Act act0[kChunk];            // the actions of chunk 0
    Act actq[kAh][kChunk];       // slot (m - 1) % kAhead holds the actions of chunk m
    auto first_loads = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < kChunk; u++) act0[u] = load_act(u);
#pragma unroll
        for (int q = 0; q < kAh; q++)
#pragma unroll
            for (int u = 0; u < kChunk; u++) actq[q][u] = load_act((q + 1) * kChunk + u);
    };
    first_loads();
    setup_shared();
    // The E waves' one barrier.  role is wave-uniform (kBlock is a multiple of the wave size), so every wave of the workgroup
    // executes exactly one s_barrier: this one or the other roles' below.  A barrier added to one path only hangs the workgroup.
    __syncthreads();
    if (i >= N) {                                   // ragged last block: its spare lanes leave (every wave that stays keeps
        // lane 0, which publishes the hand-off counters; no barrier follows); an E wave that leaves entirely counts as done
        if ((l & 63) == 0) __hip_atomic_fetch_add(&lds_done, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        return;
    }
#endif
    __builtin_amdgcn_s_setprio(kPrioE);   // the serial recurrence is the critical path; H is filler work
    // hist: bytes newest first, 0xFF = NaN  ->  nibbles newest first, bit 3 = is a state
    uint32_t k2, qv, cnt, steps0, last_reset = 0, badq[2] = {0u, 0u};
    bool pend = false;                              // next-step mode: the episode ended on the previous step
    {
#if MDPP_LEAN_TU_NOISE == 2
        const uint4 st0 = a.state[i];
#endif
        k2 = 0;
        for (int j = 3; j >= 0; j--) {
            const uint32_t b = (st0.x >> (8 * j)) & 0xFFu;
            k2 = (k2 << 4) | (b == 0xFFu ? 0u : ((b & 7u) | 8u));
        }
        const bool own_q = !PHILOX && !IRR && !nextmode && NZ == 0;   // word 1 of the state is this kernel's draw queue (fast_ok handles)
        const uint32_t qc = own_q ? (st0.y >> 24) & 7u : 0u;
        qv = own_q ? (st0.y & 0x00777777u) | (0x00888888u & ((1u << (4u * qc)) - 1u)) : 0u;
        steps0 = st0.z & 0x7FFFFFFFu;
        pend = nextmode && (st0.z >> 31) != 0u;
        const uint32_t ms = (uint32_t)a.max_steps;
        cnt = HASMAX ? (0x10000u - ms) + (steps0 < ms ? steps0 : ms) : 0u;
    }
    const uint32_t c0 = HASMAX ? 0x10000u - (uint32_t)a.max_steps : 0u;
#if MDPP_LEAN_TU_NOISE == 2
    auto r_act = __builtin_amdgcn_make_buffer_rsrc((void *)actions, 0, total * 4u * (uint32_t)kEN, kPRsrc);
    const uint32_t v4 = i * 4u * (uint32_t)kEN;
#endif
    uint32_t head_local = 0;
    S0Word s0c = 0;
    uint32_t sel = (k2 & 7u) | kSelPad;
    uint32_t c1 = IRR ? (a.irr_state[i] & 7u) : 0u;                 // the irrelevant part of curr_state
    const uint32_t A1 = IRR ? (uint32_t)a.A1 : 1u;

    uint32_t pnc = 0, pnc_hi = 0;                   // PN: this chunk's transition-noise nibbles (numpy streams: bytes a | b << 4)
    // NRN: the env stream by position (header).  ep = position of the next draw; (m0, m1, m2, xv) = meta[ep .. ep + 2], x[ep],
    // fetched at the end of the previous step; hh = positions H has made, as last read
    uint32_t ep = 0, hh = 0, m0 = 0, m1 = 0, m2 = 0;
    double xv = 0.0;
    auto ensure = [&](uint32_t upto) __attribute__((always_inline)) {       // positions < upto are made
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(upto > hh) != 0, 0)) {
            uint32_t spins = 0;
            hh = __hip_atomic_load(&lds_hhead[l], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
            while (__builtin_amdgcn_ballot_w64(upto > hh) != 0) {
                __hip_atomic_store(&lds_epos[l], ep, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);    // (H's window follows E)
                __builtin_amdgcn_s_sleep(1);
                hh = __hip_atomic_load(&lds_hhead[l], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (++spins > kSpinLimit) { status |= kStatusInternal; hh = upto; break; }
            }
        }
    };
    auto fetch = [&]() __attribute__((always_inline)) {
        ensure(ep + 3u);
        m0 = lds_meta[ep & (uint32_t)(kXR - 1)][l];
        m1 = lds_meta[(ep + 1u) & (uint32_t)(kXR - 1)][l];
        m2 = lds_meta[(ep + 2u) & (uint32_t)(kXR - 1)][l];
        if constexpr (NRX) xv = lds_x[ep & (uint32_t)(kXR - 1)][l];
    };
    if constexpr (NRN) fetch();
    // PN: byte s of {enc_lo, enc_hi} = s | 8 | is_terminal[s] << 7, the column byte of a re-drawn state
    uint32_t enc_lo = 0, enc_hi = 0;
    if constexpr (PN) {
        uint64_t enc = 0;
        for (uint32_t s_ = 0; s_ < 8u; s_++) enc |= (uint64_t)(s_ | 8u | ((uint32_t)((a.term_mask >> s_) & 1ULL) << 7)) << (8 * s_);
        enc_lo = (uint32_t)enc; enc_hi = (uint32_t)(enc >> 32);
    }
    auto pull = [&](int c) {
        if (!ar && !PN) return;                     // (no resets: nothing is drawn, the H lanes have left)
        if (NPN && c >= 0) {                        // this chunk's transition-noise bytes, made by the H wave from the space stream
            uint32_t spins = 0;
            while (wg_load_acq(&lds_hprod[w]) < (uint32_t)(c + 1)) {
                __builtin_amdgcn_s_sleep(1);
                if (++spins > kSpinLimit) { status |= kStatusInternal; break; }
            }
            pnc = lds_pn2[c % kHChunksNp][0][l];
            pnc_hi = lds_pn2[c % kHChunksNp][1][l];
        }
        if constexpr (NRN) return;                  // (start states come with the positions)
        if (!PHILOX && !ar) return;
        if constexpr (PHILOX) {                     // this chunk's start states, made by the H wave
            uint32_t spins = 0;
            while (wg_load_acq(&lds_hprod[w]) < (uint32_t)(c + 1)) {
                __builtin_amdgcn_s_sleep(1);
                if (++spins > kSpinLimit) { status |= kStatusInternal; break; }
            }
            s0c = lds_s0[c % kHChunks][l];
            if constexpr (PN) {
                spins = 0;
                while (wg_load_acq(&lds_pprod[w]) < (uint32_t)(c + 1)) {
                    __builtin_amdgcn_s_sleep(1);
                    if (++spins > kSpinLimit) { status |= kStatusInternal; break; }
                }
                pnc = lds_pn[c % kHChunks][l];
            }
            return;
        }
        const uint64_t rt = __hip_atomic_load(&lds_ring[l], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
        const uint32_t vals = (uint32_t)rt, tail = (uint32_t)(rt >> 32);
        const uint32_t qc = (uint32_t)__builtin_popcount(qv & 0x88888888u);
        const uint32_t avail = tail - head_local, room = kQueueCap - qc;       // (IRR: both even, entries are nibble pairs)
        const uint32_t take = avail < room ? avail : room;
        const uint32_t rot = __builtin_amdgcn_alignbit(vals, vals, (head_local & 7u) * 4u);
        const uint32_t m = (1u << (4u * take)) - 1u;
        qv |= (rot & m) << (4u * qc);
        head_local += take;
        __hip_atomic_store(&lds_head[l], head_local, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
#if MDPP_LEAN_TU_NOISE == 2
    typedef typename std::conditional<IRR, uint2, int>::type Act;      // (action, irrelevant action)
#endif
    typedef typename std::conditional<IRR, uint4, uint2>::type Col;    // their columns
    auto column = [&](Act act, uint32_t &badm, int u) -> Col {
        int action;
        if constexpr (IRR) action = (int)act.x; else action = act;
        uint32_t ua = (uint32_t)action;
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(ua >= A) != 0, 0)) {
            ua = (uint32_t)(action + ((action >> 31) & (int)A));
            const bool bad = ua >= A;
            // (next-step mode: an action the reset call ignores is not an error; decided at the step)
            if (nextmode) badm |= bad ? (1u << u) : 0u; else status |= bad ? (uint32_t)MDPP_STATUS_BAD_ACTION : 0u;
            ua = bad ? 0u : ua;
        }
        if constexpr (IRR) {
            const int action1 = (int)act.y;
            uint32_t ub = (uint32_t)action1;
            if (__builtin_expect(__builtin_amdgcn_ballot_w64(ub >= A1) != 0, 0)) {
                ub = (uint32_t)(action1 + ((action1 >> 31) & (int)A1));
                const bool bad = ub >= A1;
                if (nextmode) badm |= bad ? (1u << u) : 0u; else status |= bad ? (uint32_t)MDPP_STATUS_BAD_ACTION : 0u;
                ub = bad ? 0u : ub;
            }
            const uint2 ca = lds_col[ua], cb = lds_col1[ub];
            return make_uint4(ca.x, ca.y, cb.x, cb.y);
        } else {
            return lds_col[ua];
        }
    };
    auto stepE = [&](const Col &col, int k, uint32_t badbit) {
        uint32_t entry = __builtin_amdgcn_perm(col.y, col.x, sel);                    // D1: P[cur][a] | 8 | terminal << 7
        if constexpr (PN && PHILOX) {                                                 // D2 (:1604-1622), philox_pnoise_*
            const uint32_t nib = (pnc >> (4 * (k % kChunk))) & 0xFu, j = nib & 7u, nx = entry & 7u;
            const uint32_t ns = nib > 7u ? j + (j >= nx ? 1u : 0u) : nx;
            entry = __builtin_amdgcn_perm(enc_hi, enc_lo, ns | kSelPad);
        }
        if constexpr (NPN) {                                                          // ... on the space stream's word: min(a, n) + max(b - n, 0)
            const uint32_t by = (((k % kChunk) < 4 ? pnc : pnc_hi) >> (8 * (k & 3))) & 0xFFu, nx = entry & 7u;
            const uint32_t ns = min(by & 15u, nx) + (uint32_t)max((int)(by >> 4) - (int)nx, 0);
            entry = __builtin_amdgcn_perm(enc_hi, enc_lo, ns | kSelPad);
        }
        const uint32_t k2n = (k2 << 4) | entry;       // (bit 7 of the sum is set anyway: the nibble below was a state)
        bool need = entry > 0x7Fu;                                                    // D7: is_terminal[next]
        uint32_t rc = entry;                          // (O1 / O2 take bit 7 out)
        if (HASMAX) {
            cnt += 1;
            need = need || cnt >= 0x10000u;
            rc = __builtin_amdgcn_perm(cnt, entry, 0x0c060c00u);                       // byte 0 the entry, byte 2 truncated
        }
        need = need && ar;
        uint32_t rec_a = k2n;
        if (nextmode) {
            const bool ended = need && !pend;
            need = pend;                                         // reset now: this call is reset() (:2250-2278) ...
            rc = pend ? 0u : rc;                                 // ... which returns no flags,
            rec_a = pend ? 0u : k2n;                             // no reward (history word 0: O1 sees a reset, pays 0.0)
            status |= (badbit != 0u && !pend) ? (uint32_t)MDPP_STATUS_BAD_ACTION : 0u;
            pend = ended;
        }
        uint32_t s0v = PHILOX ? (uint32_t)(s0c >> (kEN * 4 * (k % kChunk))) & (IRR ? 0xFFu : 0xFu) : qv & (IRR ? 0xFFu : 0xFu);
        if constexpr (NRN) {
            // this step's draws on the env stream: the normal that starts at position ep, then -- if the episode ended -- one word
            uint32_t kind = (m0 >> 3) & 3u;
            if (__builtin_expect(__builtin_amdgcn_ballot_w64(kind >= 2u) != 0, 0)) {
                uint32_t guard = 0;
                while (__builtin_amdgcn_ballot_w64(kind == 2u) != 0) {          // wedge point rejected: the draw starts over two words on
                    const bool red = kind == 2u;
                    ep += red ? 2u : 0u;
                    uint32_t o0 = m0, o1 = m1, o2 = m2;
                    double ox = xv;
                    fetch();
                    if (!red) { m0 = o0; m1 = o1; m2 = o2; xv = ox; }
                    kind = (m0 >> 3) & 3u;
                    if (++guard > 64u) { status |= kStatusInternal; break; }
                }
            }
            uint32_t cntw = kind == 0u ? 1u : 2u, ssm = kind == 0u ? m1 : m2;
            // tail: its words are counted in the high byte, the start state of the word behind them is in bits 5-7
            if (kind == 3u) { cntw = m0 >> 8; ssm = m0 >> 5; }
            if constexpr (NRX) lds_rx[k % KD][l] = xv;
            s0v = (ssm & 7u) | 8u;
            ep += cntw + (need ? 1u : 0u);
            __hip_atomic_store(&lds_epos[l], ep, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // (H's window follows E)
            fetch();
        }
        if (!PHILOX && !NRN && __builtin_expect(__builtin_amdgcn_ballot_w64(need && s0v == 0u) != 0, 0)) {
            uint32_t spins = 0;
            while (__builtin_amdgcn_ballot_w64(need && (qv & 0xFu) == 0u) != 0) {
                pull(-1);                                        // (the queue only: not the chunk's noise bytes)
                __builtin_amdgcn_s_sleep(1);
                if (++spins > kSpinLimit) { status |= kStatusInternal; qv |= 8u; break; }
            }
            s0v = qv & (IRR ? 0xFFu : 0xFu);
        }
        if constexpr (IRR) {                                     // the irrelevant sub-space steps on its own table
            const uint32_t n1 = __builtin_amdgcn_perm(col.w, col.z, c1 | kSelPad);
            c1 = need ? ((s0v >> 4) & 7u) : n1;
            rc |= c1 << 8;                                       // byte 1: the irrelevant observation
            s0v &= 0xFu;
        }
        k2 = need ? s0v : k2n;
        if (!PHILOX && !NRN) qv = need ? (qv >> (4 * kEN)) : qv;
        if (HASMAX) cnt = need ? c0 : cnt;
        else last_reset = need ? (uint32_t)(k + 1) : last_reset;
        sel = (k2 & 7u) | kSelPad;
        lds_rec[0][k % KD][l] = rec_a;
        lds_rec[1][k % KD][l] = k2;
        lds_rec[2][k % KD][l] = rc;
    };

#if MDPP_LEAN_TU_NOISE == 2
    auto load_act = [&](int k) -> Act {
        const uint32_t kk = (uint32_t)min(k, K - 1);
        if constexpr (IRR) {
            const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(r_act, v4, kk * N * 8u, MDPP_LEAN_LD_AUX);
            return make_uint2(v.x, v.y);
        } else {
            return __builtin_amdgcn_raw_buffer_load_b32(r_act, v4, kk * N * 4u, MDPP_LEAN_LD_AUX);
        }
    };
    // Actions are fetched kAhead chunks ahead of their use, columns one chunk ahead.  The buffers rotate
    // by NAME (the chunk loop is unrolled kAhead times): copying a register whose load is still in
    // flight makes the wave wait for it, which would put one HBM latency into every chunk.
    constexpr int kAh = IRR ? 2 : kAhead;      // (action pairs: half the depth, for registers)
    static_assert(kAh % 2 == 0, "the column double buffer alternates with the chunk index");
    Act actq[kAh][kChunk];       // slot (m - 1) % kAhead holds the actions of chunk m
    Col colq[2][kChunk];            // slot m & 1 holds the columns of chunk m
#pragma unroll
    for (int u = 0; u < kChunk; u++) colq[0][u] = column(load_act(u), badq[0], u);
#pragma unroll
    for (int q = 0; q < kAh; q++)
#pragma unroll
        for (int u = 0; u < kChunk; u++) actq[q][u] = load_act((q + 1) * kChunk + u);

#else
    // (the chunk's actions were fetched before the set-up, above)
    Col colq[2][kChunk];            // slot m & 1 holds the columns of chunk m
#pragma unroll
    for (int u = 0; u < kChunk; u++) colq[0][u] = column(act0[u], badq[0], u);

#endif
    const int nfull = K / kChunk;   // full chunks; a ragged tail (K % kChunk steps) follows the loop
    auto wait_room = [&](int kend) {                // do not run more than kDepth steps ahead of the O wave
        if (kend > KD) {
            const uint32_t must = (uint32_t)(kend - KD);
            uint32_t spins = 0;
            for (;;) {
                const uint64_t cc = __hip_atomic_load((const uint64_t *)&lds_cons[w][0], __ATOMIC_ACQUIRE,
                                                      __HIP_MEMORY_SCOPE_WORKGROUP);
                uint32_t have = min((uint32_t)cc, (uint32_t)(cc >> 32));
                if (rows) {                         // whole-row stores: every O2 wave reads this wave's records
#pragma unroll
                    for (int j = 0; j < kBlock / 64; j++) have = min(have, wg_load_acq(&lds_cons[j][1]));
                }
                if (have >= must) break;
                __builtin_amdgcn_s_sleep(1);
                if (++spins > kSpinLimit) { status |= kStatusInternal; break; }
            }
        }
    };
    // one full chunk: slot j's actions -> next chunk's columns, (re)fill slot j, step, publish
    auto chunkE = [&](int c, int j, bool refill) {
        const int kbase = c * kChunk;
        badq[(j + 1) & 1] = 0u;
#pragma unroll
        for (int u = 0; u < kChunk; u++) colq[(j + 1) & 1][u] = column(actq[j][u], badq[(j + 1) & 1], u);
        if (refill) {
#pragma unroll
            for (int u = 0; u < kChunk; u++) actq[j][u] = load_act(kbase + (kAh + 1) * kChunk + u);
        }
        wait_room(kbase + kChunk);
        pull(c);
#pragma unroll
        for (int u = 0; u < kChunk; u++) stepE(colq[j & 1][u], kbase + u, (badq[j & 1] >> u) & 1u);
        if (NRN) __hip_atomic_store(&lds_epos[l], ep, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if ((l & 63) == 0) wg_store_rel(&lds_prod[w], (uint32_t)(kbase + kChunk));
    };
    // (single-exit loop body, no global load in an inner loop: the compiler then counts its vmcnt waits
    //  exactly, vmcnt(8 (kAhead - 1) + ...), instead of waiting for every load in flight)
    const int ngrp = nfull / kAh;
    for (int g = 0; g < ngrp; g++) {
#pragma unroll
        for (int j = 0; j < kAh; j++) chunkE(g * kAh + j, j, true);
    }
#pragma unroll
    for (int j = 0; j < kAh - 1; j++)
        if (ngrp * kAh + j < nfull) chunkE(ngrp * kAh + j, j, false);
    if (K % kChunk) {               // (no global load inside the loop above: its waits stay counted, not vmcnt(0))
        const int kbase = nfull * kChunk;
        Act ta[kChunk];
#pragma unroll
        for (int u = 0; u < kChunk; u++) ta[u] = load_act(kbase + u);
        wait_room(kbase + kChunk);
        pull(nfull);
#pragma unroll
        for (int u = 0; u < kChunk; u++)
            if (kbase + u < K) {
                uint32_t bm = 0;
                const Col cc = column(ta[u], bm, 0);
                stepE(cc, kbase + u, bm);
            }
        if ((l & 63) == 0) wg_store_rel(&lds_prod[w], (uint32_t)K);
    }

    // back to the handle's state words: hist bytes, queue nibbles + count, episode steps
    uint32_t hist = 0;
    for (int j = 3; j >= 0; j--) {
        const uint32_t nb = (k2 >> (4 * j)) & 0xFu;
        hist = (hist << 8) | ((nb & 8u) ? (nb & 7u) : 0xFFu);
    }
    const uint32_t qc = (uint32_t)__builtin_popcount(qv & 0x00888888u);
    const bool own_q = !PHILOX && !IRR && !nextmode && NZ == 0;
    if (NRN) __hip_atomic_store(&lds_epos[l], ep, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);   // (H un-draws what lies beyond)
    if (!own_q && !PHILOX && !NRN) {
        // word 1 of the state is not a queue for these handles: what sits in the register queue goes back to the H
        // lane (it un-draws everything not taken)
        __hip_atomic_store(&lds_head[l], head_local - qc, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    if (IRR) a.irr_state[i] = c1;                   // the irrelevant state has its own array
    uint32_t steps;
    if (HASMAX) steps = cnt - c0;
    else steps = last_reset ? (uint32_t)K - last_reset : steps0 + (uint32_t)K;
    uint32_t *st = (uint32_t *)&a.state[i];
    st[0] = hist; st[2] = steps | (pend ? 0x80000000u : 0u);        // word 3 (delay line) belongs to the O1 lane
    if (own_q) st[1] = (qv & 0x00777777u) | (qc << 24);   // (other handles: word 1 is older history, unused at L <= 3)
    if ((l & 63) == 0) __hip_atomic_fetch_add(&lds_done, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (status) atomicOr(&a.status[i], status);
