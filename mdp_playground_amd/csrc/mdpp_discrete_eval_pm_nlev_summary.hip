// The evaluation form <SUMMARY = 1, NLEV = 1> on one MDP per env (mdpp_discrete_eval.hpp: launch_eval_form_pm, the PM = 1 and
// PM = 2 kernels): greedy evaluation on a handle with per-env noise levels, keeping episode summaries -- in a translation unit
// of its own so that the forms compile in parallel.
#include "mdpp_discrete_eval.hpp"

template int mdpp::launch_eval_form_pm<true, true>(mdpp_env *, const mdpp::DiscreteIO &);
