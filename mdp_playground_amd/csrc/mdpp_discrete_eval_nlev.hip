// The per-env noise-level (NLEV = 1; mdpp_set_noise_levels) instantiations of k_discrete_eval_rollout_nlev (see mdpp_discrete_eval.hip): greedy evaluation,
// in a translation unit of its own so that the forms compile in parallel.
#define MDPP_EVAL_TU_NLEV 1
#include "mdpp_discrete_eval.hip"
