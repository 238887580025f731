// Grid learners keeping an episode log (mdpp_step_n_grid_learn_log) under a per-episode schedule: the SCHED = 1
// instantiations of k_grid_learn_log_rollout.  The kernel and the launcher: mdpp_grid_learn.hpp.
#include "mdpp_grid_learn.hpp"

namespace mdpp {

template int launch_grid_learn_form<true, true, true>(mdpp_env *, const DiscreteIO &, bool);

} // namespace mdpp
