// gemm_fast_lnf_f16.hip -- the LayerNorm-fold instantiations of gemm_fast.hip for the fp16 precision mode (the operands are fp16 in both
// modes; here the 16-bit outputs are too), behind launch_gemm_fast_lnf_f16().  Split off for build time only.
#define F5_LNF_TU 1
#define F5_F16_TU 1
#include "gemm_fast.hip"
