// The learner form <PE = 1, DOUBLE = 1, SUMMARY = 1, NLEV = 1, SCHED = 1> (mdpp_discrete_learn.hpp): double Q-learning with a per-episode epsilon / alpha
// schedule on a handle with per-env noise levels, keeping episode summaries -- in a translation unit of its own so that the forms compile in parallel.
#include "mdpp_discrete_learn.hpp"

template int mdpp::launch_learn_form<true, true, true, true, true>(mdpp_env *, const mdpp::DiscreteIO &);
