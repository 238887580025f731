// The learner form <PE = 1, DOUBLE = 0, SUMMARY = 0, NLEV = 0> (mdpp_discrete_learn.hpp): Q-learning and SARSA with per-env hyper-parameters --
// in a translation unit of its own so that the forms compile in parallel.
#include "mdpp_discrete_learn.hpp"

template int mdpp::launch_learn_form<true, false, false, false>(mdpp_env *, const mdpp::DiscreteIO &);
