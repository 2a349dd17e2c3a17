// Third translation unit of the conv path: the bf16-operand instantiations of the four MFMA kernel families of
// cgl_conv.hip (cgl_conv_set_mma_dtype), compiled apart from cgl_conv_tu.hip so that they build in parallel with
// the fp32 ones instead of doubling that unit's compile time.  Only the combinations the fp32 dispatchers
// (launch_conv_mma, conv_bwd_weight_impl) can form are instantiated; they call the launchers below with the
// template arguments, grid and LDS size of the fp32 launch they replace.
#include "cgl_internal.h"

#define CGL_CONV_MMA_KERNELS_ONLY
#include "cgl_conv.hip"

#define CGL_BF CGL_DTYPE_BF16

int cgl_conv_fwd_bf16(int tm, int tn, bool fast, bool bnin, bool ldsm, int wg, int lds, hipStream_t s,
                      const CglConvLaunch& L) {
#define CGL_FWD(TM, TN, FAST, BNIN, LDSM) \
  hipLaunchKernelGGL((cgl_conv_fwd<TM, TN, FAST, BNIN, LDSM, CGL_BF>), dim3(wg), dim3(256), lds, s, L)
  if (ldsm) {
    if (tm != 2 || tn != 2 || !fast || bnin) return CGL_E_ARG;
    CGL_FWD(2, 2, true, false, true);
  } else if (bnin) {
    if (!fast) return CGL_E_ARG;
    if (tm == 2 && tn == 2) CGL_FWD(2, 2, true, true, false);
    else if (tm == 2 && tn == 1) CGL_FWD(2, 1, true, true, false);
    else if (tm == 1 && tn == 1) CGL_FWD(1, 1, true, true, false);
    else return CGL_E_ARG;
  } else if (tm == 2 && tn == 2) {
    if (fast) CGL_FWD(2, 2, true, false, false);
    else CGL_FWD(2, 2, false, false, false);
  } else if (tm == 2 && tn == 1) {
    if (fast) CGL_FWD(2, 1, true, false, false);
    else CGL_FWD(2, 1, false, false, false);
  } else if (tm == 1 && tn == 1) {
    if (fast) CGL_FWD(1, 1, true, false, false);
    else CGL_FWD(1, 1, false, false, false);
  } else {
    return CGL_E_ARG;
  }
#undef CGL_FWD
  return (int)hipGetLastError();
}

int cgl_conv_fwd_halo_bf16(bool bnin, int grid, int lds, hipStream_t s, const CglConvLaunch& L) {
  if (bnin) hipLaunchKernelGGL((cgl_conv_fwd_halo<true, CGL_BF>), dim3(grid), dim3(256), lds, s, L);
  else hipLaunchKernelGGL((cgl_conv_fwd_halo<false, CGL_BF>), dim3(grid), dim3(256), lds, s, L);
  return (int)hipGetLastError();
}

int cgl_conv_wgrad_bf16(int tm, int tn, bool row, bool bnin, int wg, hipStream_t s, const CglConvLaunch& L) {
#define CGL_WG(TM, TN)                                                                                      \
  do {                                                                                                      \
    if (row && bnin) hipLaunchKernelGGL((cgl_conv_wgrad<TM, TN, true, true, CGL_BF>), dim3(wg), dim3(256), 0, s, L);    \
    else if (row) hipLaunchKernelGGL((cgl_conv_wgrad<TM, TN, true, false, CGL_BF>), dim3(wg), dim3(256), 0, s, L);      \
    else if (bnin) hipLaunchKernelGGL((cgl_conv_wgrad<TM, TN, false, true, CGL_BF>), dim3(wg), dim3(256), 0, s, L);     \
    else hipLaunchKernelGGL((cgl_conv_wgrad<TM, TN, false, false, CGL_BF>), dim3(wg), dim3(256), 0, s, L);              \
  } while (0)
  // (the fp32 dispatch's order: 2 x 2, then TN = 2, then TM = 2)
  if (tm == 2 && tn == 2) CGL_WG(2, 2);
  else if (tn == 2) CGL_WG(1, 2);
  else if (tm == 2) CGL_WG(2, 1);
  else CGL_WG(1, 1);
#undef CGL_WG
  return (int)hipGetLastError();
}

int cgl_conv_wgrad_lds_bf16(int wm, int ks, bool bnin, int wgl, hipStream_t s, const CglConvLaunch& L) {
  if ((wm != 1 && wm != 2) || (ks != 1 && ks != 2) || (bnin && ks != 1)) return CGL_E_ARG;
  if (bnin) {
    if (wm == 2) hipLaunchKernelGGL((cgl_conv_wgrad_lds<2, 2, 1, true, CGL_BF>), dim3(wgl), dim3(256), 0, s, L);
    else hipLaunchKernelGGL((cgl_conv_wgrad_lds<1, 4, 1, true, CGL_BF>), dim3(wgl), dim3(256), 0, s, L);
  } else if (ks == 2) {
    if (wm == 2) hipLaunchKernelGGL((cgl_conv_wgrad_lds<2, 2, 2, false, CGL_BF>), dim3(wgl), dim3(512), 0, s, L);
    else hipLaunchKernelGGL((cgl_conv_wgrad_lds<1, 4, 2, false, CGL_BF>), dim3(wgl), dim3(512), 0, s, L);
  } else {
    if (wm == 2) hipLaunchKernelGGL((cgl_conv_wgrad_lds<2, 2, 1, false, CGL_BF>), dim3(wgl), dim3(256), 0, s, L);
    else hipLaunchKernelGGL((cgl_conv_wgrad_lds<1, 4, 1, false, CGL_BF>), dim3(wgl), dim3(256), 0, s, L);
  }
  return (int)hipGetLastError();
}
