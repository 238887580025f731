// k_continuous_es_rollout<..., HIST=2>: the antithetic ES per 64 linear policies with memory, E = D (2 D + 1) entries
// (include/mdpp.h "Linear policies with memory") -- mdpp_continuous_es.hip's agent and launcher with the act of
// mdpp_linear_history.hpp.
#define MDPP_LINEAR_HIST 2
#include "mdpp_continuous_es.hip"
