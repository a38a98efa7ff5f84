#define DNS_BWD_NN 32
#define DNS_BWD_NL 1
#define DNS_TF_STEM
#include "track_fused.inc"
