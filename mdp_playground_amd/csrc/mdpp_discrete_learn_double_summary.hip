// The learner form <PE = 0, DOUBLE = 1, SUMMARY = 1, NLEV = 0> (mdpp_discrete_learn.hpp): double Q-learning, keeping episode summaries --
// in a translation unit of its own so that the forms compile in parallel.
#include "mdpp_discrete_learn.hpp"

template int mdpp::launch_learn_form<false, true, true, false>(mdpp_env *, const mdpp::DiscreteIO &);
