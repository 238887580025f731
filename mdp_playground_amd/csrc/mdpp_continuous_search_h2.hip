// k_continuous_search_rollout<..., HIST=2>: the (1+1)-ES per env on a linear policy with memory, E = D (2 D + 1) entries
// (include/mdpp.h "Linear policies with memory") -- mdpp_continuous_search.hip's agent and launcher with the act of
// mdpp_linear_history.hpp.
#define MDPP_LINEAR_HIST 2
#include "mdpp_continuous_search.hip"
