// Grid learners: the instantiations of k_grid_learn_rollout that keep episode summaries instead of the [K][N] arrays
// (mdpp_step_n_grid_learn_summary / mdpp_step_n_grid_eval_summary); a unit of its own so that the two output forms compile
// side by side.  The kernel and the launcher: mdpp_grid_learn.hpp.
#include "mdpp_grid_learn.hpp"

namespace mdpp {

template int launch_grid_learn_form<true>(mdpp_env *, const DiscreteIO &, bool);

} // namespace mdpp
