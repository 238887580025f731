// k_continuous_linear_rollout<..., HIST=2>: the linear-policy rollout under a policy with memory, a = clip(W o + V p + b)
// (include/mdpp.h "Linear policies with memory") -- mdpp_continuous_linear.hip's agent and launcher with the act of
// mdpp_linear_history.hpp.
#define MDPP_LINEAR_HIST 2
#include "mdpp_continuous_linear.hip"
