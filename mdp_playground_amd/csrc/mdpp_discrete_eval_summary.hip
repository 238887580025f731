// The instantiations of k_discrete_eval_summary (see mdpp_discrete_eval.hip): greedy evaluation that keeps episode summaries
// instead of writing [K][N] arrays, in a translation unit of its own so that the two forms compile in parallel.
#define MDPP_EVAL_TU_SUMMARY 1
#include "mdpp_discrete_eval.hip"
