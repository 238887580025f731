// The per-env hyper-parameter (PE = 1) instantiations of k_discrete_learn_rollout (see mdpp_discrete_learn.hip), in
// their own translation unit so that the learner's forms compile in parallel.
#define MDPP_LEARN_TU_PE 1
#include "mdpp_discrete_learn.hip"
