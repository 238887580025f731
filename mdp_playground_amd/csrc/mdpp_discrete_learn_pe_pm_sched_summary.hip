// The learner form <DOUBLE = 0, SUMMARY = 1, NLEV = 0, SCHED = 1> on one MDP per env (mdpp_discrete_learn.hpp: launch_learn_form_pm, the
// PM = 1 and PM = 2 kernels): Q-learning and SARSA with a per-episode epsilon / alpha schedule, keeping episode summaries -- in a
// translation unit of its own so that the forms compile in parallel.
#include "mdpp_discrete_learn.hpp"

template int mdpp::launch_learn_form_pm<false, true, false, true>(mdpp_env *, const mdpp::DiscreteIO &);
