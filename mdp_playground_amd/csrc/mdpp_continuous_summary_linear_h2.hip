// k_continuous_linear_summary<..., HIST=2>: the summary form of the linear-policy rollout under a policy with memory
// (include/mdpp.h "Linear policies with memory").
#define MDPP_LINEAR_HIST 2
#define MDPP_CLIN_TU_SUMMARY 1
#include "mdpp_continuous_linear.hip"
