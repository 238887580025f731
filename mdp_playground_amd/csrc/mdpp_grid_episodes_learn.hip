// Grid learners keeping an episode log (mdpp_step_n_grid_learn_log) without a schedule: the SCHED = 0 instantiations of
// k_grid_learn_log_rollout.  The kernel and the launcher: mdpp_grid_learn.hpp.
#include "mdpp_grid_learn.hpp"

namespace mdpp {

template int launch_grid_learn_form<true, false, true>(mdpp_env *, const DiscreteIO &, bool);

} // namespace mdpp
