// The per-env noise-level (NLEV = 1; mdpp_set_noise_levels) instantiations of k_discrete_eval_summary_nlev (see mdpp_discrete_eval.hip): greedy evaluation keeping episode summaries,
// in a translation unit of its own so that the forms compile in parallel.
#define MDPP_EVAL_TU_NLEV 1
#define MDPP_EVAL_TU_SUMMARY 1
#include "mdpp_discrete_eval.hip"
