// Grid learners with per-env noise levels (mdpp_set_grid_noise_levels; include/mdpp.h "Grid noise levels"): the instantiations of
// k_grid_learn_nlev_sched_rollout (a per-episode schedule in force too) that keep episode summaries instead of the [K][N] arrays.
// The kernel and the launcher: mdpp_grid_learn.hpp.
#include "mdpp_grid_learn.hpp"

namespace mdpp {

template int launch_grid_learn_form<true, true, false, true>(mdpp_env *, const DiscreteIO &, bool);

} // namespace mdpp
