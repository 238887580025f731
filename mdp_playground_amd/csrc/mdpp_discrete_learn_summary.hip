// The learner form <PE = 0, DOUBLE = 0, SUMMARY = 1, NLEV = 0> (mdpp_discrete_learn.hpp): Q-learning and SARSA, keeping episode summaries --
// in a translation unit of its own so that the forms compile in parallel.
#include "mdpp_discrete_learn.hpp"

template int mdpp::launch_learn_form<false, false, true, false>(mdpp_env *, const mdpp::DiscreteIO &);
