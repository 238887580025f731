// Linear policies with memory (include/mdpp.h "Linear policies with memory"): what the three agent units -- mdpp_continuous_linear.hip,
// mdpp_continuous_search.hip, mdpp_continuous_es.hip -- share for a policy of history 2,
//   a = clip(W o + V p + b, +-action_space_max),  p = the o of the env's previous act (o itself on the first step of an episode).
//
// MDPP_LINEAR_HIST is the history a translation unit is compiled for.  1 (the default): the units as they always were, every
// kernel under its own name and with its own arguments.  2: the *_h2.hip units define it and include the unit they extend;
// their kernels take one more template argument, HIST, and one more kernel argument, the memory, and their names end in
// ",HIST=2".  E = D (HIST D + 1) entries per policy, entry e = r (HIST D + 1) + c: W[r][c] for c < D, V[r][c - D] for
// D <= c < 2 D, b[r] last.
//
// The memory is the handle's float32 [D][N] buffer (component c of env i at mem[c N + i]: consecutive lanes, consecutive
// addresses).  It is not carried in registers across the step (the D = 12 step holds 250 VGPRs): the V pass reads it where it
// multiplies and act() overwrites it with o afterwards, 2 x 4 D bytes per env step.
#pragma once

#ifndef MDPP_LINEAR_HIST
#define MDPP_LINEAR_HIST 1
#endif

#if MDPP_LINEAR_HIST == 2
#define MDPP_HIST_TPARAM , int HIST
#define MDPP_HIST_TARG , 2
#define MDPP_HIST_KPARAM , float *mem     // the kernels' last argument: the handle's memory, [D][N]
#define MDPP_HIST_KARG , mem
#define MDPP_HIST_SET_MEM(agent, n) agent.mem = mem; agent.N = n;
#define MDPP_HIST_NAME ",HIST=2"
#elif MDPP_LINEAR_HIST == 1
#define MDPP_HIST_TPARAM
#define MDPP_HIST_TARG
#define MDPP_HIST_KPARAM
#define MDPP_HIST_KARG
#define MDPP_HIST_SET_MEM(agent, n)
#define MDPP_HIST_NAME ""
#else
#error "MDPP_LINEAR_HIST must be 1 or 2"
#endif

namespace mdpp {

// The act of a history = 2 policy, stated once.  p: entry 0 of this lane (entry e at p[e stride]); mem: component 0 of this
// lane's memory (component c at mem[c N]); first: the env has taken no step in its current episode, p = o.  Per row acc = b[r],
// then the W pass over o, then the V pass over p, every product and every sum rounded to float32 (-ffp-contract=off), then the
// clamp of LinearAgent::act; a NaN acc stays NaN.  Afterwards the memory becomes o -- on a reset call too.
template <int DMAX>
__device__ __forceinline__ void linear_act_h2(const float *p, long stride, int D, float amax, const float (&o)[DMAX], float *mem, long N,
                                              bool first, float (&a)[DMAX]) {
    const long b_off = 2L * D * stride;                // row r: W[r][0 .. D-1], V[r][0 .. D-1], then b[r]
#pragma unroll
    for (int r = 0; r < DMAX; r++) {
        float acc = 0.0f;
        if (r < D) {
            acc = p[b_off];
#pragma unroll
            for (int c = 0; c < DMAX; c++)
                if (c < D) { const float w = *p; const float t = w * o[c]; acc = acc + t; p += stride; }
            const float *m = mem;
#pragma unroll
            for (int c = 0; c < DMAX; c++)
                if (c < D) { const float v = *p; const float q = first ? o[c] : *m; const float t = v * q; acc = acc + t; p += stride; m += N; }
            p += stride;
            acc = acc < -amax ? -amax : (acc > amax ? amax : acc);
        }
        a[r] = acc;
    }
    float *m = mem;
#pragma unroll
    for (int c = 0; c < DMAX; c++)
        if (c < D) { *m = o[c]; m += N; }
}

} // namespace mdpp
