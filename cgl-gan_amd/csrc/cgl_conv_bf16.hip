// Third translation unit of the conv path: the bf16-operand instantiations of the four MFMA kernel families of
// cgl_conv.hip (cgl_conv_set_mma_dtype), compiled apart from cgl_conv_tu.hip so that they build in parallel with
// the fp32 ones instead of doubling that unit's compile time.  Only the combinations the fp32 dispatchers
// (launch_conv_mma, conv_bwd_weight_impl) can form are instantiated; they call the launchers below with the
// template arguments, grid and LDS size of the fp32 launch they replace.  Each launch stores its launch record
// (cgl_conv_last_launches) as the fp32 ones do, with CGL_LF_BF16.
#include "cgl_internal.h"

#define CGL_CONV_MMA_KERNELS_ONLY
#include "cgl_conv.hip"

#define CGL_BF CGL_DTYPE_BF16

int cgl_conv_fwd_bf16(int tm, int tn, bool fast, bool bnin, bool ldsm, int wg, int lds, hipStream_t s,
                      const CglConvLaunch& L) {
#define CGL_FWD(TM, TN, FAST, BNIN, LDSM)                                                                        \
  CGL_LAUNCH_L(CGL_REC(CGL_K_CONV_FWD, TM, TN,                                                                   \
                       CGL_LF_BF16 | (FAST ? CGL_LF_FAST : 0) | (BNIN ? CGL_LF_BNIN : 0) | (LDSM ? CGL_LF_LDSM : 0)), \
               &L, 0, (cgl_conv_fwd<TM, TN, FAST, BNIN, LDSM, CGL_BF>), dim3(wg), dim3(256), lds, s, L)
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
  if (bnin)
    CGL_LAUNCH_L(CGL_REC(CGL_K_CONV_FWD_HALO, 0, 0, CGL_LF_BF16 | CGL_LF_HALO | CGL_LF_BNIN), &L, 0,
                 (cgl_conv_fwd_halo<true, CGL_BF>), dim3(grid), dim3(256), lds, s, L);
  else
    CGL_LAUNCH_L(CGL_REC(CGL_K_CONV_FWD_HALO, 0, 0, CGL_LF_BF16 | CGL_LF_HALO), &L, 0,
                 (cgl_conv_fwd_halo<false, CGL_BF>), dim3(grid), dim3(256), lds, s, L);
  return (int)hipGetLastError();
}

int cgl_conv_wgrad_bf16(int tm, int tn, bool row, bool bnin, int wg, hipStream_t s, const CglConvLaunch& L) {
#define CGL_WGK(TM, TN, ROW, BNIN)                                                                              \
  CGL_LAUNCH_L(CGL_REC(CGL_K_CONV_WGRAD, TM, TN, CGL_LF_BF16 | (ROW ? CGL_LF_ROW : 0) | (BNIN ? CGL_LF_BNIN : 0)), \
               &L, L.p[0].splits, (cgl_conv_wgrad<TM, TN, ROW, BNIN, CGL_BF>), dim3(wg), dim3(256), 0, s, L)
#define CGL_WG(TM, TN)                              \
  do {                                              \
    if (row && bnin) CGL_WGK(TM, TN, true, true);   \
    else if (row) CGL_WGK(TM, TN, true, false);     \
    else if (bnin) CGL_WGK(TM, TN, false, true);    \
    else CGL_WGK(TM, TN, false, false);             \
  } while (0)
  // (the fp32 dispatch's order: 2 x 2, then TN = 2, then TM = 2)
  if (tm == 2 && tn == 2) CGL_WG(2, 2);
  else if (tn == 2) CGL_WG(1, 2);
  else if (tm == 2) CGL_WG(2, 1);
  else CGL_WG(1, 1);
#undef CGL_WG
#undef CGL_WGK
  return (int)hipGetLastError();
}

int cgl_conv_wgrad_lds_bf16(int wm, int ks, bool bnin, int wgl, hipStream_t s, const CglConvLaunch& L) {
  if ((wm != 1 && wm != 2) || (ks != 1 && ks != 2) || (bnin && ks != 1)) return CGL_E_ARG;
#define CGL_LDS(WM_, WN_, KS_, BNIN, THREADS) CGL_LAUNCH_WLDS(WM_, WN_, KS_, BNIN, CGL_BF, wgl, THREADS, s, L)
  if (bnin) {
    if (wm == 2) CGL_LDS(2, 2, 1, true, 256);
    else CGL_LDS(1, 4, 1, true, 256);
  } else if (ks == 2) {
    if (wm == 2) CGL_LDS(2, 2, 2, false, 512);
    else CGL_LDS(1, 4, 2, false, 512);
  } else {
    if (wm == 2) CGL_LDS(2, 2, 1, false, 256);
    else CGL_LDS(1, 4, 1, false, 256);
  }
#undef CGL_LDS
  return (int)hipGetLastError();
}
