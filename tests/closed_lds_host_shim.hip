// Host call of the closed-loop agents' LDS placement (mdpp_discrete_closed.hpp: closed_agent_lds), for
// tests/test_closed_lds_placement_host.py only (not part of libmdpp_hip.so).  No HIP API call is made.
#include "../mdp_playground_amd/csrc/mdpp_discrete_closed.hpp"

// The placement of a handle filled by hand with what the rule reads, under a device that grants up to `budget` bytes.
// asked: the calls of granted in order, {q, slots, cdfs, bytes} each (at most 8 rows are written); *n_asked: how many were
// made.  Returns the subset chosen: bit 2 Q, bit 1 the slots, bit 0 the cdfs.
extern "C" int closed_lds_host(int pm, uint64_t q_lds, uint32_t lds_bytes, uint32_t lds_noise, int rew_in_lds, int philox,
                               int has_p_noise, uint32_t opts, int nl_on, int nl_levels, int S, uint64_t budget,
                               uint64_t *asked, int *n_asked) {
    mdpp_env h{};
    h.dargs.lds_bytes = lds_bytes; h.dargs.lds_noise = lds_noise;
    h.dargs.rew_in_lds = (uint32_t)rew_in_lds; h.dargs.philox = philox; h.dargs.has_p_noise = has_p_noise;
    h.opts = opts;
    h.nl_on = nl_on != 0; h.nl_levels = nl_levels; h.cfg.S = S;
    int n = 0;
    const mdpp::ClosedLdsPlacement at = mdpp::closed_agent_lds(&h, (size_t)q_lds, pm != 0, [&](bool q, bool m, bool c, size_t bytes) {
        if (n < 8) { asked[4 * n] = q; asked[4 * n + 1] = m; asked[4 * n + 2] = c; asked[4 * n + 3] = bytes; }
        n += 1;
        return bytes <= budget;
    });
    *n_asked = n;
    return (at.q ? 4 : 0) | (at.slots ? 2 : 0) | (at.cdfs ? 1 : 0);
}
