// The trace-learner form <PE = 1, SUMMARY = 0, SCHED = 0> (mdpp_discrete_trace.hpp): Q(lambda) and SARSA(lambda) with per-env hyper-parameters --
// in a translation unit of its own so that the forms compile in parallel.
#include "mdpp_discrete_trace.hpp"

template int mdpp::launch_trace_form<true, false, false>(mdpp_env *, const mdpp::DiscreteIO &);
