// The learner form <PE = 1, DOUBLE = 0, SUMMARY = 0, NLEV = 1, SCHED = 1> (mdpp_discrete_learn.hpp): Q-learning and SARSA with a per-episode epsilon / alpha
// schedule on a handle with per-env noise levels -- in a translation unit of its own so that the forms compile in parallel.
#include "mdpp_discrete_learn.hpp"

template int mdpp::launch_learn_form<true, false, false, true, true>(mdpp_env *, const mdpp::DiscreteIO &);
