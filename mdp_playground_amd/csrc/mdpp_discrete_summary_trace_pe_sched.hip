// The trace-learner form <PE = 1, SUMMARY = 1, SCHED = 1> (mdpp_discrete_trace.hpp): Q(lambda) and SARSA(lambda) with a per-episode epsilon / alpha schedule, keeping episode summaries --
// in a translation unit of its own so that the forms compile in parallel.
#include "mdpp_discrete_trace.hpp"

template int mdpp::launch_trace_form<true, true, true>(mdpp_env *, const mdpp::DiscreteIO &);
