// k_continuous_es_summary<..., HIST=2>: the summary form of the antithetic ES per 64 linear policies with memory
// (include/mdpp.h "Linear policies with memory").
#define MDPP_LINEAR_HIST 2
#define MDPP_CES_TU_SUMMARY 1
#include "mdpp_continuous_es.hip"
