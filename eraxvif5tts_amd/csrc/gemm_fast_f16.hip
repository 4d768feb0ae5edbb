// gemm_fast_f16.hip -- translation unit of gemm_fast.hip for the fp16 precision mode: the same kernels with the element type f16_t
// (v_mfma_f32_16x16x32_f16, saturating fp16 stores), behind launch_gemm_fast_f16().  Split off for build time only.
#define F5_F16_TU 1
#include "gemm_fast.hip"
