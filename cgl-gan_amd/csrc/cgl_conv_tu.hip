// Second translation unit of libcglgan_hip: the conv GAN path of model/lsgan.py (implicit-GEMM
// convolutions, BatchNorm2d, losses, Adam) and the evaluation kernels.  Compiled separately from
// the MLP step (cgl_runtime.hip) so that either side rebuilds alone; shared helpers live in
// cgl_common.h.  cgl_conv.hip takes the MFMA kernels from cgl_conv_mma.h and instantiates them for
// fp32 here; cgl_conv_bf16.hip holds their bf16 instances.  BatchNorm2d and the elementwise passes are
// cgl_conv_bn.h (kernels and launch helpers, included by cgl_conv.hip) and cgl_conv_bn.hip (entry points).
#include "cgl_internal.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "cgl_conv.hip"
#include "cgl_conv_bn.hip"
#include "cgl_eval.hip"
