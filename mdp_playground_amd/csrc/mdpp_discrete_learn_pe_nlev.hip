// The per-env noise-level (NLEV = 1; mdpp_set_noise_levels) instantiations of k_discrete_learn_rollout_nlev (see mdpp_discrete_learn.hip): Q-learning and SARSA with per-env hyper-parameters (PE = 1),
// in a translation unit of its own so that the forms compile in parallel.
#define MDPP_LEARN_TU_NLEV 1
#define MDPP_LEARN_TU_PE 1
#include "mdpp_discrete_learn.hip"
