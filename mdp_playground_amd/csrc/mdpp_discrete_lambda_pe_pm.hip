// The trace-learner form <PE = 1, SUMMARY = 0, SCHED = 0> on one MDP per env, PM = 1 and PM = 2 (mdpp_discrete_trace.hpp): Q(lambda) and
// SARSA(lambda) with every env on its own MDP -- in a translation unit of its own so that the forms compile in parallel.
#include "mdpp_discrete_trace.hpp"

template int mdpp::launch_trace_form_pm<false, false>(mdpp_env *, const mdpp::DiscreteIO &);
