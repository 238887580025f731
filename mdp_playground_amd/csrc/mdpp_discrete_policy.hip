// Closed-loop fused rollout of a discrete env under a tabular policy: the launch that does s -> s' also samples
// a ~ pi(. | s), so K steps of an agent that acts on what it observes are ONE launch (mdpp_step_n_policy).  The step itself
// is closed_loop_rollout (mdpp_discrete_closed.hpp) without its NOISE branches; this file holds the agent.
//
// The policy is a table of thresholds T uint32 [S][A] (non-decreasing rows; T[s][j] = ceil(cdf_s[j] 2^31)) and a 64-bit
// seed.  Env g = env_id_offset + i at step counter t draws
//   w = word (t & 3) of block 0 of the Philox4x32-10 stream (policy seed, g, t >> 2, kPhiloxPolicyStream)   [mdpp_rng.hpp philox_start_block]
//   a = min(#{ j < A : T[s][j] <= (w >> 1) }, A - 1),      s = the state the env is in (the last observation returned for it)
// -- the rule of philox_start_m31 for start states: searchsorted(cdf_s, (w >> 1) 2^-31, 'right').
//
// The thresholds are staged in LDS behind the MDP's tables; a row of at most 8 actions is padded to 8 entries (0xFFFFFFFF:
// never <= a 31-bit draw), read as two 16-byte LDS reads and counted without a branch; longer rows are searched (the same
// count on a non-decreasing row).  The policy's words do not depend on the state: the block of the NEXT four ticks is made
// while the current one is used, so the chain a step waits for is  threshold row of s -> count -> P[s][a].
#include "mdpp_discrete_closed.hpp"

namespace mdpp {

// what the kernel takes besides the handle's DiscreteArgs
struct PolicyArgs {
    const uint32_t *thr;        // [S][A] thresholds (device)
    uint64_t seed;              // policy seed: key of the policy's Philox stream
    int32_t *actions;           // [K][N] the sampled actions (out)
};

// uint32 per threshold row in LDS
__host__ __device__ inline uint32_t policy_row_words(int A) { return A <= 8 ? 8u : (uint32_t)A; }

template <bool A8>
struct PolicyAgent {
    const PolicyArgs &p;
    // the policy's words: the block of ticks 4 b .. 4 b + 3, the next one made ahead.  (They stand BEFORE the other members
    // and are initialised by name in the kernel: with the arrays last the compiler lays the step loop out with its latch and
    // the reset-call blocks behind the body -- the same instructions, 2 % slower at one wave per SIMD)
    uint32_t w_cur[4], w_nxt[4];
    uint32_t *lds_thr;          // [S][W] the thresholds' copy
    uint32_t S, A, W;

    __device__ __forceinline__ void stage(int tid) {
        for (uint32_t k = tid; k < S * W; k += kBlock) {
            const uint32_t s = k / W, j = k - s * W;
            lds_thr[k] = j < A ? p.thr[s * A + j] : 0xFFFFFFFFu;
        }
    }
    __device__ __forceinline__ void begin(uint32_t, uint64_t genv, uint64_t ptick0) {
        philox_start_block(p.seed, genv, ptick0 >> 2, kPhiloxPolicyStream, w_nxt);
    }
    __device__ __forceinline__ void next_block(uint64_t genv, uint64_t ptick) {
#pragma unroll
        for (int q = 0; q < 4; q++) w_cur[q] = w_nxt[q];
        philox_start_block(p.seed, genv, (ptick >> 2) + 1u, kPhiloxPolicyStream, w_nxt);
    }
    // a = min(#{ j : T[cur][j] <= m }, A - 1)
    __device__ __forceinline__ uint32_t act(uint32_t cur, uint64_t ptick) const {
        const uint32_t m = philox_word_of(w_cur, ptick) >> 1;
        uint32_t cnt = 0;
        if (A8) {
            const uint4 t0 = ((const uint4 *)lds_thr)[2u * cur], t1 = ((const uint4 *)lds_thr)[2u * cur + 1u];
            cnt = (t0.x <= m) + (t0.y <= m) + (t0.z <= m) + (t0.w <= m) + (t1.x <= m) + (t1.y <= m) + (t1.z <= m) + (t1.w <= m);
        } else {
            const uint32_t *row = lds_thr + cur * W;
            for (uint32_t n = A; n > 0;) {              // first j with T[j] > m on a non-decreasing row
                const uint32_t half = n >> 1;
                const bool le = row[cnt + half] <= m;
                cnt = le ? cnt + half + 1u : cnt;
                n = le ? n - half - 1u : half;
            }
        }
        return cnt < A - 1u ? cnt : A - 1u;
    }
    __device__ __forceinline__ void learn(uint32_t, uint32_t, uint32_t, float, bool, bool, uint64_t) {}
    __device__ __forceinline__ void episode_end(bool) {}
    __device__ __forceinline__ void finish(uint32_t) {}
};

template <bool PHILOX, bool UNIT, bool OBS64, bool A8>
__global__ __launch_bounds__(kBlock) void k_discrete_policy_rollout(DiscreteArgs a, PolicyArgs p, int K,
                                                                    void *__restrict__ obs,
                                                                    float *__restrict__ reward,
                                                                    uint8_t *__restrict__ term,
                                                                    uint8_t *__restrict__ trunc) {
    extern __shared__ __align__(16) unsigned char lds[];
    PolicyAgent<A8> agent{p, {}, {}, (uint32_t *)(lds + a.lds_bytes), (uint32_t)a.S, (uint32_t)a.A, A8 ? 8u : (uint32_t)a.A};
    closed_loop_rollout<PHILOX, false, UNIT>(a, K, OBS64, p.actions, obs, reward, term, trunc, lds, ZigLds{nullptr, nullptr, nullptr}, agent);
}

// Why this handle has no closed-loop launch, or empty: the kernel serves it
std::string discrete_policy_refusal(const mdpp_env *h) {
    return closed_loop_refusal(h, "policy", false, 4ull * (uint64_t)h->cfg.S * policy_row_words(h->cfg.A), "the MDP's tables and the thresholds");
}

// K closed-loop steps from the handle's policy
int launch_discrete_policy(mdpp_env *h, const DiscreteIO &io) {
    const std::string why = discrete_policy_refusal(h);
    if (!why.empty()) { h->err = "mdpp_step_n_policy: " + why; return MDPP_EUNSUPPORTED; }
    const DiscreteArgs &a = h->dargs;
    int rc = MDPP_OK;
    with_bools([&](auto PH, auto UNIT, auto O64, auto A8) {
        char name[kNameLen];
        snprintf(name, kNameLen, "k_discrete_policy_rollout<PHILOX=%d,UNIT=%d,OBS64=%d,A8=%d>", PH(), UNIT(), O64(), A8());
        rc = launch_closed_loop<false>(h, io, k_discrete_policy_rollout<PH(), UNIT(), O64(), A8()>,
                                (size_t)a.lds_bytes + 4u * (size_t)a.S * policy_row_words(a.A), false, name, [&](int, int, int32_t *actions) {
            return PolicyArgs{(const uint32_t *)h->d_policy_thr, h->policy_seed, actions};
        });
    }, a.philox != 0, a.unit_rewards != 0, !a.obs_i32, a.A <= 8);
    return rc;
}

} // namespace mdpp
