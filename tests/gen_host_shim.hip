// Host build of the device MDP generator, for tests/test_mdp_generate_host.py only (not part of libmdpp_hip.so).
// gen_discrete_env<Pcg64> is __host__ __device__: here it runs on the CPU, one env after another, with the parameter
// checks and the GenArgs fill of mdpp_generate_discrete (gen_args_init).  No HIP API call is made.
#include "../mdp_playground_amd/csrc/mdpp_generate.hip"

#include <vector>

// Envs [0, N) of {config, seeds[i]}: P uint8 [N][S][A], rbits uint8 [N][rbits_stride] (unit) or rtable float64 [N][nkeys]
// (zeroed by the caller), seed dicts uint64 [N][8], and the PCG64 streams the generator leaves as uint64 [N][4]
// {state lo, state hi, inc lo, inc hi}: env, space, image (image may be null).  MDPP_OK or gen_args_init's code, with
// its message copied to err.
extern "C" int gen_host_discrete(const mdpp_gen_params *p, int S, int A, int L, int image, int unit, uint32_t nkeys,
                                 uint32_t rbits_stride, const uint64_t *seeds, int N, uint8_t *P, uint8_t *rbits,
                                 double *rtable, uint64_t *sd, uint64_t *env_words, uint64_t *sp_words,
                                 uint64_t *im_words, char *err, int err_len) {
    GenArgs a;
    const char *msg = nullptr;
    const int rc = gen_args_init(p, S, A, L, image != 0, unit != 0, nkeys, rbits_stride, a, &msg);
    if (rc != MDPP_OK) {
        snprintf(err, (size_t)err_len, "%s", msg);
        return rc;
    }
    std::vector<uint64_t> scratch(a.scratch_words);
    std::vector<ulonglong2> st(6 * (size_t)N);
    std::vector<uint2> half((size_t)N);
    a.rews = p->rews;
    a.seeds = seeds;
    a.P = P; a.rbits = rbits; a.rtable = rtable; a.sd = sd;
    a.env_s = &st[0]; a.env_inc = &st[(size_t)N]; a.sp_s = &st[2 * (size_t)N]; a.sp_inc = &st[3 * (size_t)N];
    if (image) { a.im_s = &st[4 * (size_t)N]; a.im_inc = &st[5 * (size_t)N]; a.im_half = half.data(); }
    for (int e = 0; e < N; e++) gen_discrete_env<Pcg64>(a, e, scratch.data());
    uint64_t *outs[3] = {env_words, sp_words, image ? im_words : nullptr};
    for (int k = 0; k < 3; k++) {
        if (!outs[k]) continue;
        for (int e = 0; e < N; e++) {
            const ulonglong2 s = st[(2 * (size_t)k) * N + e], inc = st[(2 * (size_t)k + 1) * N + e];
            outs[k][4 * (size_t)e + 0] = s.x; outs[k][4 * (size_t)e + 1] = s.y;
            outs[k][4 * (size_t)e + 2] = inc.x; outs[k][4 * (size_t)e + 3] = inc.y;
        }
    }
    return MDPP_OK;
}
