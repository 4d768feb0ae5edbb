// attention_fast_f16.hip -- translation unit of attention_fast.hip for the fp16 precision mode: the 64-queries-per-wave kernel with the element
// type f16_t (f16 MFMA shape, a tile redone when a row sum reaches 2^15; no reference-free build), behind launch_attention_wide_f16().
#define F5_F16_TU 1
#include "attention_fast.hip"
