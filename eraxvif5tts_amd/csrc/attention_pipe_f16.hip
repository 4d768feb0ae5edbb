// attention_pipe_f16.hip -- translation unit of attention_pipe.hip for the fp16 precision mode: the pipelined kernel with the element type
// f16_t (f16 MFMA shape, deferral threshold 2^14), behind launch_attention_pipe_f16 / launch_attention_pipe_segs_f16.  Split off for build time.
#define F5_F16_TU 1
#include "attention_pipe.hip"
