// Third translation unit of the conv path: the bf16-operand instances (cgl_conv_set_mma_dtype) of the four MFMA
// kernel families of cgl_conv_mma.h, compiled apart from cgl_conv_tu.hip so that they build in parallel with the
// fp32 ones instead of doubling that unit's compile time, and rebuild only when the header changes.  The launcher
// templates state the routes; instantiating them for bf16 instantiates exactly the kernels the fp32 side has.
#include "cgl_conv_mma.h"

template int cgl_conv_fwd_launch<CGL_DTYPE_BF16>(int, int, bool, bool, bool, int, int, hipStream_t,
                                                 const CglConvLaunch&);
template int cgl_conv_fwd_halo_launch<CGL_DTYPE_BF16>(bool, int, int, hipStream_t, const CglConvLaunch&);
template int cgl_conv_wgrad_launch<CGL_DTYPE_BF16>(int, int, bool, bool, int, hipStream_t, const CglConvLaunch&);
template int cgl_conv_wgrad_lds_launch<CGL_DTYPE_BF16>(int, int, bool, int, hipStream_t, const CglConvLaunch&);
