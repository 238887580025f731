// k_continuous_es_summary: the linear policy ES that keeps per-env episode summaries and writes no [K][N] array
// (mdpp_step_n_linear_es_summary) -- mdpp_continuous_es.hip's agent and launcher around the SUMMARY form of the step.
#define MDPP_CES_TU_SUMMARY 1
#include "mdpp_continuous_es.hip"
