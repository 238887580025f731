// Per-env discrete MDPs generated on the device: one lane per env restates what mdp.build_discrete does for
// {**config, "seed": seed} (rl_toy_env.py:285-333 seed dict, :1050-1151 P, :1273-1558 rewardable sequences) on the
// same numpy PCG64 streams, draw for draw, so the tables and generator states are bit-identical to the host's.
// Covered configs only (mdp.device_coverage): no irrelevant sub-space, S <= 255, the sequence draw on Floyd's path
// of Generator.choice.  Runs once per handle: exactness and bounded scratch before speed.
#include "mdpp_internal.hpp"
#include "mdpp_rng.hpp"

namespace mdpp {

__host__ __device__ inline bool bit_test(const uint64_t *m, uint64_t v) { return (m[v >> 6] >> (v & 63u)) & 1u; }
__host__ __device__ inline void bit_set(uint64_t *m, uint64_t v) { m[v >> 6] |= 1ull << (v & 63u); }

// searchsorted(cdf, u, 'right') for the categorical Generator.choice(S, p=prob) builds: prob = 1/A on the A states
// [b, b + A) of the independent set after s's (mdp._next_set_prob) minus the states in `zero`; cdf = sequential cumsum
// divided by its last entry, as np.cumsum and `cdf /= cdf[-1]` compute it.  tot = that last entry.
__host__ __device__ inline int gen_search(int S, int b, int A, double pa, const uint64_t *zero, double tot, double u) {
    double c = 0.0;
    int cnt = 0;
    for (int j = 0; j < S; j++) {
        if (j >= b && j < b + A && !bit_test(zero, (uint64_t)j)) c += pa;
        cnt += (c / tot <= u) ? 1 : 0;
    }
    return cnt;
}
__host__ __device__ inline double gen_total(int S, int b, int A, double pa, const uint64_t *zero) {
    double c = 0.0;
    for (int j = 0; j < S; j++) {
        if (j >= b && j < b + A && !bit_test(zero, (uint64_t)j)) c += pa;
    }
    return c;
}

// Generator.choice(total, size=n, replace=False), Floyd's branch: for j = total - n ... total - 1 draw v in [0, j] and keep
// it unless already chosen (then j); then shuffle the n picks with bounded draws.  numpy's hash set only answers
// membership, so a bitset of `total` bits (`set`, cleared here) gives the same picks.
template <class G>
__host__ __device__ inline void gen_floyd(G &g, Half32 &h, uint64_t total, uint32_t n, uint64_t *set, uint64_t *out) {
    for (uint64_t w = 0; w < (total + 63u) / 64u; w++) set[w] = 0;
    for (uint64_t j = total - n; j < total; j++) {
        uint64_t v = np_bounded_u64(g, h, j);
        if (bit_test(set, v)) v = j;
        bit_set(set, v);
        out[j - (total - n)] = v;
    }
    for (uint32_t i = n - 1; i > 0 && n > 1; i--) {
        const uint64_t j = np_bounded_u64(g, h, i);
        const uint64_t t = out[i]; out[i] = out[j]; out[j] = t;
    }
}

template <class G>
__host__ __device__ inline void gen_discrete_env(const GenArgs &a, int e, uint64_t *scr) {
    const uint64_t seed = a.seeds[e];
    G env;
    pcg64_seedseq(seed, env);
    Half32 eh{0u, 0u};
    uint64_t sd[8];
    sd[0] = seed;
    for (int k = 1; k < 8; k++) sd[k] = np_bounded_u64(env, eh, 0x7FFFFFFFFFFFFFFEull);   // integers(sys.maxsize)
    if (a.sd)
        for (int k = 0; k < 8; k++) a.sd[(size_t)e * 8 + k] = sd[k];

    // ---- P from the relevant state space's generator, seeded with seed_dict["relevant_state_space"]
    G sp;
    pcg64_seedseq(sd[1], sp);
    Half32 sh{0u, 0u};
    const int S = a.S, A = a.A, d = a.diameter;
    uint8_t *P = a.P + (size_t)e * S * A;
    const double pa = 1.0 / (double)A;
    const uint64_t none[4] = {0, 0, 0, 0};
    for (int s = 0; s < S; s++) {
        uint8_t *row = P + (size_t)s * A;
        const int b = ((s / A + 1) * A) % S;          // first state of the next independent set
        if (a.maxc && d == 1) {                        // choice(S, size=A, replace=False)
            uint64_t m[4] = {0, 0, 0, 0};
            for (int j = S - A; j < S; j++) {
                uint32_t v = (uint32_t)np_bounded_u64(sp, sh, (uint64_t)j);
                if (bit_test(m, v)) v = (uint32_t)j;
                bit_set(m, v);
                row[j - (S - A)] = (uint8_t)v;
            }
            for (int i = A - 1; i > 0; i--) {
                const uint32_t j = (uint32_t)np_bounded_u64(sp, sh, (uint64_t)i);
                const uint8_t t = row[i]; row[i] = row[j]; row[j] = t;
            }
        } else if (a.maxc) {                           // choice(S, size=A, p=prob, replace=False): rounds of fresh draws
            uint64_t found[4] = {0, 0, 0, 0}, zero[4] = {0, 0, 0, 0};
            int n = 0;
            while (n < A) {
                const double tot = gen_total(S, b, A, pa, zero);
                const int want = A - n;
                for (int k = 0; k < want; k++) {
                    const int idx = gen_search(S, b, A, pa, zero, tot, np_random_f64(sp));
                    if (!bit_test(found, (uint64_t)idx)) { bit_set(found, (uint64_t)idx); row[n++] = (uint8_t)idx; }
                }
                for (int w = 0; w < 4; w++) zero[w] = found[w];
            }
        } else {                                       // A draws of choice(S, p=prob)
            const double tot = gen_total(S, b, A, pa, none);
            for (int k = 0; k < A; k++) row[k] = (uint8_t)gen_search(S, b, A, pa, none, tot, np_random_f64(sp));
        }
    }
    for (int i_s = 0; i_s < d; i_s++)                  // terminal self-loops (drawn above all the same)
        for (int s = A - a.n_term; s < A; s++)
            for (int k = 0; k < A; k++) P[(size_t)(i_s * A + s) * A + k] = (uint8_t)(i_s * A + s);
    if (a.sp_s) {
        a.sp_s[e] = make_ulonglong2(sp.s_lo, sp.s_hi);
        a.sp_inc[e] = make_ulonglong2(sp.inc_lo, sp.inc_hi);
    }

    // ---- rewardable sequences from the env generator: picks of sequence numbers, decoded
    const uint32_t nn = (uint32_t)(A - a.n_term), n_sel = a.n_sel;
    uint64_t *set = scr, *picks = scr + a.set_words;
    uint32_t *perm = (uint32_t *)(scr + a.perm_off);
    const int rounds = a.repeats ? 1 : d;
    for (int r = 0; r < rounds; r++) gen_floyd(env, eh, a.total, n_sel, set, picks + (size_t)r * n_sel);
    if (a.rews) {                                      // Generator.shuffle of the linspace values: masked rejection
        for (uint32_t k = 0; k < a.n_rews; k++) perm[k] = k;
        for (uint32_t i = a.n_rews - 1; i > 0; i--) {
            const uint32_t j = (uint32_t)np_interval(env, eh, i);
            const uint32_t t = perm[i]; perm[i] = perm[j]; perm[j] = t;
        }
    }
    uint32_t k = 0;                                    // insertion order: value k of the shuffled array
    for (int i_s = 0; i_s < d; i_s++) {
        for (uint32_t q = 0; q < n_sel; q++) {
            uint64_t num = picks[(size_t)(a.repeats ? 0 : i_s) * n_sel + q];
            uint32_t key = 0;
            uint32_t removed[16];
            int n_removed = 0;
            for (int pos = 0; pos < a.L; pos++) {
                const uint32_t which = (uint32_t)((pos + i_s) % d);
                uint32_t v;
                if (a.repeats) {
                    v = (uint32_t)(num % nn);
                    num /= nn;
                } else {                               // pools[which].pop(digit): the digit-th state not yet taken
                    const uint32_t radix = a.radix[pos], digit = (uint32_t)(num % radix);
                    num /= radix;
                    v = digit;
                    for (;;) {
                        uint32_t below = 0;
                        for (int t = 0; t < n_removed; t++)
                            below += ((removed[t] >> 8) == which && (removed[t] & 0xFFu) <= v) ? 1u : 0u;
                        if (digit + below == v) break;
                        v = digit + below;
                    }
                    removed[n_removed++] = which << 8 | v;
                }
                key = key * (uint32_t)S + v + which * (uint32_t)A;
            }
            if (a.unit) a.rbits[(size_t)e * a.rbits_stride + (key >> 3)] |= (uint8_t)(1u << (key & 7u));
            else a.rtable[(size_t)e * a.nkeys + key] = a.rews ? a.rews[perm[k]] : 1.0;
            k++;
        }
    }

    // ---- fresh streams: the env's own (reset(seed=seed_dict["env"]) of the constructor) and the image transforms'
    if (a.env_s) {
        Pcg64 g;
        pcg64_seedseq(seed, g);
        a.env_s[e] = make_ulonglong2(g.s_lo, g.s_hi);
        a.env_inc[e] = make_ulonglong2(g.inc_lo, g.inc_hi);
    }
    if (a.im_s) {
        Pcg64 g;
        pcg64_seedseq(sd[7], g);
        a.im_s[e] = make_ulonglong2(g.s_lo, g.s_hi);
        a.im_inc[e] = make_ulonglong2(g.inc_lo, g.inc_hi);
        if (a.im_half) a.im_half[e] = make_uint2(0u, 0u);
    }
}

__global__ void __launch_bounds__(64) k_generate_discrete(GenArgs a, int first, int count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    gen_discrete_env<Pcg64>(a, first + i, a.scratch + (size_t)i * a.scratch_words);
}

__global__ void __launch_bounds__(256) k_seed_streams_seedseq(const uint64_t *seeds, int N, ulonglong2 *st, ulonglong2 *inc,
                                                              uint2 *half) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    Pcg64 g;
    pcg64_seedseq(seeds[i], g);
    st[i] = make_ulonglong2(g.s_lo, g.s_hi);
    inc[i] = make_ulonglong2(g.inc_lo, g.inc_hi);
    if (half) half[i] = make_uint2(0u, 0u);
}

}  // namespace mdpp

using namespace mdpp;

hipError_t launch_generate_discrete(const GenArgs &a, int first, int count) {
    if (count <= 0) return hipSuccess;
    k_generate_discrete<<<(count + 63) / 64, 64>>>(a, first, count);
    return hipGetLastError();
}

hipError_t launch_seed_streams_seedseq(const uint64_t *seeds, int N, void *st, void *inc, void *half) {
    if (N <= 0) return hipSuccess;
    k_seed_streams_seedseq<<<(N + 255) / 256, 256>>>(seeds, N, (ulonglong2 *)st, (ulonglong2 *)inc, (uint2 *)half);
    return hipGetLastError();
}
