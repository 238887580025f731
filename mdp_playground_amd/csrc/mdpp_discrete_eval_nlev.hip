// The evaluation form <SUMMARY = 0, NLEV = 1> (mdpp_discrete_eval.hpp): greedy evaluation on a handle with per-env noise levels --
// in a translation unit of its own so that the forms compile in parallel.
#include "mdpp_discrete_eval.hpp"

template int mdpp::launch_eval_form<false, true>(mdpp_env *, const mdpp::DiscreteIO &);
