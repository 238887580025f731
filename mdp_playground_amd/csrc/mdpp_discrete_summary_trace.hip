// The trace-learner form <PE = 0, SUMMARY = 1, SCHED = 0> (mdpp_discrete_trace.hpp): Q(lambda) and SARSA(lambda) keeping episode summaries --
// in a translation unit of its own so that the forms compile in parallel.
#include "mdpp_discrete_trace.hpp"

template int mdpp::launch_trace_form<false, true, false>(mdpp_env *, const mdpp::DiscreteIO &);
