// The learner form <PE = 0, DOUBLE = 1, SUMMARY = 0, NLEV = 0> (mdpp_discrete_learn.hpp): double Q-learning --
// in a translation unit of its own so that the forms compile in parallel.
#include "mdpp_discrete_learn.hpp"

template int mdpp::launch_learn_form<false, true, false, false>(mdpp_env *, const mdpp::DiscreteIO &);
