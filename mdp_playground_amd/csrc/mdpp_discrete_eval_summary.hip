// The evaluation form <SUMMARY = 1, NLEV = 0> (mdpp_discrete_eval.hpp): greedy evaluation keeping episode summaries --
// in a translation unit of its own so that the forms compile in parallel.
#include "mdpp_discrete_eval.hpp"

template int mdpp::launch_eval_form<true, false>(mdpp_env *, const mdpp::DiscreteIO &);
