// gemm_w4_f16.hip -- translation unit of gemm_w4.hip for the fp16 precision mode: the one-wave-per-SIMD kernel with the element type f16_t
// (the _f16 MFMA mnemonic in every instantiation, saturating fp16 stores), behind launch_gemm_w4_f16().  Split off for build time only.
#define F5_F16_TU 1
#include "gemm_w4.hip"
