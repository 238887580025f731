// The double Q-learning (DOUBLE = 1) instantiations of k_discrete_learn_summary (see mdpp_discrete_learn.hip): the learner that keeps episode
// summaries instead of writing [K][N] arrays, in a translation unit of its own so that the learner's forms compile in parallel.
#define MDPP_LEARN_TU_SUMMARY 1
#define MDPP_LEARN_TU_DOUBLE 1
#include "mdpp_discrete_learn.hip"
