// k_continuous_search_summary: the linear policy search that keeps per-env episode summaries and writes no [K][N] array
// (mdpp_step_n_linear_search_summary) -- mdpp_continuous_search.hip's agent and launcher around the SUMMARY form of the step.
#define MDPP_CSRCH_TU_SUMMARY 1
#include "mdpp_continuous_search.hip"
