// The evaluation form <SUMMARY = 1> on one MDP per env (mdpp_discrete_eval.hpp: launch_eval_form_pm, the PM = 1 and PM = 2
// kernels): greedy evaluation keeping episode summaries -- in a translation unit of its own so that the forms compile in
// parallel.
#include "mdpp_discrete_eval.hpp"

template int mdpp::launch_eval_form_pm<true, false>(mdpp_env *, const mdpp::DiscreteIO &);
