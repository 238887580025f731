// k_continuous_linear_summary: the linear-policy rollout that keeps per-env episode summaries and writes no [K][N] array
// (mdpp_step_n_linear_summary) -- mdpp_continuous_linear.hip's agent and launcher around the SUMMARY form of the step.
#define MDPP_CLIN_TU_SUMMARY 1
#include "mdpp_continuous_linear.hip"
