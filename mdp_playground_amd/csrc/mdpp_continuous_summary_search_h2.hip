// k_continuous_search_summary<..., HIST=2>: the summary form of the (1+1)-ES per env on a linear policy with memory
// (include/mdpp.h "Linear policies with memory").
#define MDPP_LINEAR_HIST 2
#define MDPP_CSRCH_TU_SUMMARY 1
#include "mdpp_continuous_search.hip"
