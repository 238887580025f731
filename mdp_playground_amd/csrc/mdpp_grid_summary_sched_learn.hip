// Grid learners under a per-episode schedule (mdpp_set_grid_learner_schedule): the instantiations of
// k_grid_learn_sched_rollout that keep episode summaries instead of the [K][N] arrays.  The kernel and the launcher:
// mdpp_grid_learn.hpp.
#include "mdpp_grid_learn.hpp"

namespace mdpp {

template int launch_grid_learn_form<true, true>(mdpp_env *, const DiscreteIO &, bool);

} // namespace mdpp
