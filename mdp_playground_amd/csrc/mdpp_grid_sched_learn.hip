// Grid learners under a per-episode schedule (mdpp_set_grid_learner_schedule): the full-output instantiations of
// k_grid_learn_sched_rollout; a unit of its own so that the forms compile side by side and the unscheduled units keep the
// code they had.  The kernel and the launcher: mdpp_grid_learn.hpp.
#include "mdpp_grid_learn.hpp"

namespace mdpp {

template int launch_grid_learn_form<false, true>(mdpp_env *, const DiscreteIO &, bool);

} // namespace mdpp
