// The MFMA side of the conv path (cgl_conv.hip describes the design), shared by the two translation units that
// compile it: the launch descriptors, the device helpers, the four MFMA kernel families (cgl_conv_fwd,
// cgl_conv_fwd_halo, cgl_conv_wgrad, cgl_conv_wgrad_lds; operand type DT at compile time), the launch record's
// helpers and macros, and one launcher template per family that states its route table once for both operand
// types.  cgl_conv_tu.hip (through cgl_conv.hip) instantiates the launchers -- and with them the kernels -- for
// fp32, cgl_conv_bf16.hip for bf16.
#pragma once
#include "cgl_internal.h"

#define CGL_CONV_MAXP 4
#define CGL_AS4 __attribute__((address_space(4)))

struct CglConvProb {
  int M, N, K, Kp;           // enumerated output pixels, output channels, K = taps * Cin, packed row length
  int OH, OW;                // enumerated output grid per image
  int osy, osx, ooy, oox;    // stored output position (oy * osy + ooy, ox * osx + oox)
  int YH, YW, ldy;           // stored output dims and channel count (pixel stride)
  int isy, isx;              // input step per enumerated output pixel
  int IH, IW, ish;           // virtual input bounds; stored input is read at (iy >> ish, ix >> ish)
  int XH, XW, Cin;           // stored input dims / channels
  int Ty, Tx;                // tap grid, t = ty * Tx + tx
  int dy[4], dx[4];          // tap offsets
  int ym[4], xm[4];          // kernel rows / columns combined into each tap (bitmask of kh / kw)
  int wg_begin, tiles_m, tiles_n, splits;
  const float* X;
  const float* Wp;           // packed weights [N][Kp]
  float* Y;                  // output (fwd), or the output gradient dY (wgrad, read only)
  float* part;               // wgrad partials [splits][N][Kp]
  int st_gr, st_off;         // BatchNorm statistics in the epilogue: rows per forward call (group),
                             // first 32-row chunk of this problem within a group's chunks
};

struct CglConvLaunch {
  CglConvProb p[CGL_CONV_MAXP];
  int np, WM, WN, WK;        // waves per workgroup: WM x WN output blocks x WK k-splits
  const float* bias;         // [N] or null
  int act;                   // CGL_EPI_ACT_*
  float slope;
  const float* drop;         // Dropout2d scale per (image, channel) [img][ldy], or null
  int wbias;                 // weight gradient: im2col column K is the constant 1 (bias gradient)
  double* st_part;           // per-(32-row chunk, channel) BatchNorm2d partials of the stored output:
  int st_cpg;                // 32-row chunks per group (all problems)
  int st_mode;               //   0 {sum, M2} (forward statistics), 1 {sum g, sum g (x - mean)} with
  float st_slope;            //   g = the stored dY (* leaky'(post)) (backward statistics)
  const float* st_x;         // mode 1: the BatchNorm input x, the post-activation (or null) and the
  const float* st_post;      // saved per-call mean [groups][N], all at the stored tensor's positions
  const float* st_mean;
  // forward statistics of a call whose first group (the D step's real call) holds a short batch: only its
  // first *st_nv images are real (DataLoader's short final batch, capgan.py:282,326-331); the padding
  // images' rows are left out of the partials (single-problem launches only; null: every row counts)
  const int* st_nv;
  int ilv;                   // forward: the np problems share X and their tile grid -- tiles interleaved
                             // problem-minor (tile t of every problem back to back on one XCD)
  // forward with the input's BatchNorm2d folded into the operand load (the producer's bn2d finalize wrote
  // scale / shift per (group, channel): in_coef = [2][in_groups][Cin]): x -> fmaf(x, scale, shift), then
  // LeakyReLU when in_act -- cgl_eltwise's arithmetic, so the operand equals the applied activation
  const float* in_coef;
  int in_groups, in_gimg;    // BatchNorm groups (forward calls) and input images per group
  int in_act;
  float in_slope;
  int in_g0;                 // weight gradient (one call's rows): the input's BatchNorm group
  // backward statistics without the post-activation tensor: LeakyReLU'(post) from the sign of the forward's
  // fmaf(x, scale, shift), scale = st_psc[c], shift = st_psc[st_psc_ld + c] (cgl_bn2d_bwd's post_coef)
  const float* st_psc;
  int st_psc_ld;
};

typedef const CGL_AS4 CglConvLaunch* CglKL;
typedef const CGL_AS4 CglConvProb* CglKP;

// The launch descriptor is the kernel's first (by-value) argument: read it through the kernarg
// segment pointer so that uniform-indexed fields become scalar loads (a dynamically indexed
// by-value struct would otherwise be copied to scratch).
__device__ __forceinline__ CglKL cgl_conv_args() { return (CglKL)__builtin_amdgcn_kernarg_segment_ptr(); }

__device__ __forceinline__ int cgl_conv_prob(CglKL L, int bid) {
  int pi = 0;
  for (int q = 1; q < L->np; ++q)
    if (bid >= L->p[q].wg_begin) pi = q;
  return pi;
}

__device__ __forceinline__ void cgl_conv_pix(CglKP P, int m, int& img, int& oy, int& ox) {
  const int hw = P->OH * P->OW;
  img = m / hw;
  const int r = m - img * hw;
  oy = r / P->OW;
  ox = r - oy * P->OW;
}

// q = a / d, r = a % d for 0 <= a < 2^31, d >= 1 (inv = 1.0 / d): the double product is within
// one of the quotient, fixed by one branch-free correction step (no integer division sequence)
__device__ __forceinline__ void cgl_divmod(int a, int d, double inv, int& q, int& r) {
  q = (int)((double)a * inv);
  r = a - q * d;
  const bool hi = r >= d, lo = r < 0;
  q += hi ? 1 : (lo ? -1 : 0);
  r += hi ? -d : (lo ? d : 0);
}

__device__ __forceinline__ int cgl_xcd_tile(int local, int nwg) {
  if (nwg < 16) return local;
  const int xcd = local & 7, pos = local >> 3, q = nwg >> 3, r = nwg & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + pos;
}

// ------------------------------------------------------------------------------------------
// Forward / input-gradient convolution: C[m][n] = sum_k A[m][k] Wp[n][k] with the implicit A of
// the tap table.  One wave owns TM x TN 32x32 accumulators; WM x WN waves per workgroup.
// FAST: Cin % 16 == 0, so a 16-k chunk lies inside one tap (uniform tap, 2 x 16-byte loads per
// lane and block).  Otherwise each k is decoded per element (tiny-K layers: Cin = 1).
// The folded BatchNorm's activation slope: LeakyReLU(w) = max(w, w * slope) -- bitwise cgl_eltwise's
// (w > 0 ? w : w * slope) for 0 < slope <= 1 (the entry points require it: at slope 0 the select turns
// w = -inf into -inf * 0 = NaN where the max form gives -inf), two VALU ops instead of three;
// act none = slope 1 (max(w, w) = w), so the staging loops carry no activation branch.
__device__ __forceinline__ float cgl_bnin_slope(CglKL L) {
  return L->in_act == CGL_EPI_ACT_LEAKY ? L->in_slope : 1.f;
}

#ifndef CGL_HALO_SB
#define CGL_HALO_SB 8   // the halo window's staging loads in flight per thread (1: one load, then its store)
#endif
// DT (compile time, CGL_DTYPE_F32 / CGL_DTYPE_BF16; cgl_conv_set_mma_dtype): with bf16 the finished fragment of
// a 16-k chunk -- after the masks and the folded BatchNorm -- is rounded to bf16 (RNE) and one
// v_mfma_f32_32x32x16_bf16 replaces the chunk's eight f32 MFMAs (cgl_mfma16); loads, LDS staging (fp32),
// accumulators and the epilogue are the fp32 kernel's.
template <int DT, int TM, int TN>
__device__ __forceinline__ void cgl_conv_mm16(f32x16 (&acc)[TM][TN], const float (&A)[TM][8], const float (&B)[TN][8]) {
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) cgl_mfma16<DT>(acc[i][j], A[i], B[j]);
}

template <int TM, int TN, bool FAST, bool BNIN = false, bool HALO = false, bool LDSM = false, int DT = CGL_DTYPE_F32>
__device__ __forceinline__ void cgl_conv_fwd_body(CglKL L, CglKP P, int local, float* s_red, bool direct = false) {
  constexpr int S = 3;
  static_assert(DT == CGL_DTYPE_F32 || DT == CGL_DTYPE_BF16, "fp32 or bf16 MFMA operands");
  static_assert(!LDSM || (TM == 2 && TN == 2 && FAST && !BNIN && !HALO), "the LDS main loop: 2x2 blocks, FAST");
  static_assert(!BNIN || FAST, "the folded BatchNorm input needs the FAST (uniform-tap chunk) path");
  static_assert(!HALO || (TM == 2 && TN == 2 && FAST), "the halo path is the 2x2-block FAST path");
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, li = lane & 31, lh = lane >> 5;
  const int WN = L->WN, WM = L->WM, WK = L->WK;
  // HALO: the workgroup's waves each own the same tile of a different problem (the caller picks P per wave)
  const int wsel = HALO ? 0 : wave;
  const int wk = wsel % WK, wmn = wsel / WK;
  const int wm = wmn / WN, wn = wmn - wm * WN;
  const int tiles_n = P->tiles_n;
  const int tile = direct ? local : cgl_xcd_tile(local, P->tiles_m * tiles_n);
  const int tn = tile % tiles_n, tm = tile / tiles_n;
  const int M = P->M, N = P->N, K = P->K, Kp = P->Kp, Cin = P->Cin;
  const int IH = P->IH, IW = P->IW, ish = P->ish, XW = P->XW, Tx = P->Tx;
  const int m0 = tm * 32 * TM * WM + wm * 32 * TM;
  const int n0 = (tn * WN + wn) * 32 * TN;
  const float* __restrict__ X = P->X;

  int ay[TM], ax[TM];
  long aoff[TM];
  int cgo[TM];                 // BNIN: this row's BatchNorm group offset into the coefficient table
  float* s_coef = s_red;       // BNIN: [2][in_groups][Cin] scale / shift staged in LDS ahead of s_red
  const int coef_n = BNIN ? 2 * L->in_groups * Cin : 0;
  const float bn_sl = BNIN ? cgl_bnin_slope(L) : 0.f;
  if constexpr (BNIN && !HALO) {
    for (int q = tid; q < coef_n; q += 256) s_coef[q] = gld(L->in_coef + q);
    s_red += (coef_n + 63) & ~63;
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    int img, oy, ox;
    cgl_conv_pix(P, min(m0 + 32 * i + li, M - 1), img, oy, ox);
    ay[i] = oy * P->isy;
    ax[i] = ox * P->isx;
    aoff[i] = (long)img * P->XH * XW * Cin;
    cgo[i] = BNIN ? min(img / L->in_gimg, L->in_groups - 1) * Cin : 0;
  }
  const float* brow[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) brow[j] = P->Wp + (long)min(n0 + 32 * j + li, N - 1) * Kp;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  auto load = [&](int c, float (&A)[TM][8], float (&B)[TN][8], int& okm) {
    const int k0 = c * 16;
    okm = 0;
    if (FAST) {
      // the chunk lies inside one tap (Cin % 16 == 0), or the problem has a single tap and
      // Cin % 4 == 0: then the K tail is masked per float4 (bits 4 / 5 of okm)
      const int t = k0 / Cin;
      const int ci = k0 - t * Cin + 8 * lh;
      const int ty = t / Tx, tx = t - ty * Tx;
      const int dyv = P->dy[ty], dxv = P->dx[tx];
      okm = (ci < Cin ? 16 : 0) | (ci + 4 < Cin ? 32 : 0);
      const int c0 = min(ci, Cin - 4), c1 = min(ci + 4, Cin - 4);
      if (BNIN) okm |= (c0 << 8) | (c1 << 20);   // the channels of the two float4, for the folded BatchNorm
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int iy = ay[i] + dyv, ix = ax[i] + dxv;
        const bool ok = (unsigned)iy < (unsigned)IH && (unsigned)ix < (unsigned)IW;
        okm |= ok ? (1 << i) : 0;
        const int cy = min(max(iy, 0), IH - 1) >> ish, cx = min(max(ix, 0), IW - 1) >> ish;
        gcfp p = (gcfp)(X + aoff[i] + ((long)cy * XW + cx) * Cin);
        const f32x4 u = *(gcf4p)(p + c0), w = *(gcf4p)(p + c1);
        A[i][0] = u[0]; A[i][1] = u[1]; A[i][2] = u[2]; A[i][3] = u[3];
        A[i][4] = w[0]; A[i][5] = w[1]; A[i][6] = w[2]; A[i][7] = w[3];
      }
    } else {
#pragma unroll
      for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int k = k0 + 8 * lh + q;
          const int kk = min(k, K - 1);
          const int t = kk / Cin, ci = kk - t * Cin;
          const int ty = t / Tx, tx = t - ty * Tx;
          const int iy = ay[i] + P->dy[ty], ix = ax[i] + P->dx[tx];
          const bool ok = k < K && (unsigned)iy < (unsigned)IH && (unsigned)ix < (unsigned)IW;
          okm |= ok ? (1 << (i * 8 + q)) : 0;
          const int cy = min(max(iy, 0), IH - 1) >> ish, cx = min(max(ix, 0), IW - 1) >> ish;
          A[i][q] = ((gcfp)X)[aoff[i] + ((long)cy * XW + cx) * Cin + ci];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      gcfp p = (gcfp)(brow[j] + k0 + 8 * lh);
      const f32x4 u = *(gcf4p)p, w = *(gcf4p)(p + 4);
      B[j][0] = u[0]; B[j][1] = u[1]; B[j][2] = u[2]; B[j][3] = u[3];
      B[j][4] = w[0]; B[j][5] = w[1]; B[j][6] = w[2]; B[j][7] = w[3];
    }
  };
  auto compute = [&](float (&A)[TM][8], float (&B)[TN][8], int okm) {
    if constexpr (BNIN) {
      // BatchNorm2d (+ LeakyReLU) of the loaded input, from the staged scale / shift (before the mask:
      // padded taps and out-of-range channels stay zero, as in the applied activation)
      const int c0 = (okm >> 8) & 0xfff, c1 = (okm >> 20) & 0xfff;
      const int shb = coef_n >> 1;
      const float sl = bn_sl;
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const f32x4 s0 = *(const f32x4*)(s_coef + cgo[i] + c0), s1 = *(const f32x4*)(s_coef + cgo[i] + c1);
        const f32x4 h0 = *(const f32x4*)(s_coef + shb + cgo[i] + c0), h1 = *(const f32x4*)(s_coef + shb + cgo[i] + c1);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          float v = fmaf(A[i][q], q < 4 ? s0[q] : s1[q - 4], q < 4 ? h0[q] : h1[q - 4]);
          v = fmaxf(v, v * sl);
          A[i][q] = v;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      if (FAST) {
        const bool ok0 = ((okm >> i) & 1) && (okm & 16), ok1 = ((okm >> i) & 1) && (okm & 32);
#pragma unroll
        for (int q = 0; q < 8; ++q) A[i][q] = (q < 4 ? ok0 : ok1) ? A[i][q] : 0.f;
      } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) A[i][q] = ((okm >> (i * 8 + q)) & 1) ? A[i][q] : 0.f;
      }
    }
    if constexpr (DT != CGL_DTYPE_F32) {
      cgl_conv_mm16<DT>(acc, A, B);
      return;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[i][q], B[j][q], acc[i][j], 0, 0, 0);
  };

  // S register sets in rotation (S - 1 chunks of loads in flight); Kp % 16 == 0, no K tail.
  // This wave's k-split: chunks [cb, ce).
  const int nch = Kp >> 4;
  const int cb = (wk * nch) / WK, ce = ((wk + 1) * nch) / WK;
  if constexpr (LDSM) {
    // LDS-staged operand panels (2 x 2 waves of 64 x 64, WK = 1; the input gradients of the upsampling convs):
    // per 16-k chunk the workgroup's 256 threads fetch the A panel [128 rows][16 k] (two 16-byte im2col loads
    // each) and the B panel [128 columns][16 k] (two 16-byte weight loads each) into LDS, where each element is
    // read by the 2 waves sharing its row (column) block instead of loaded by each.  Rows padded to 20 floats:
    // the 16 lanes of a 16-byte read phase cover the 64 banks once.  The next chunk's loads are in flight while
    // this one is multiplied (two register sets, two LDS buffers, one barrier per chunk).  Fragment values and
    // MFMA order are the direct path's (lane half lh holds k 8 lh .. 8 lh + 7 of the chunk), so the results are
    // bitwise equal to it.
    constexpr int RS = 20;
    float* const la = s_red;                  // [2][128][RS]
    float* const lb = s_red + 2 * 128 * RS;   // [2][128][RS]
    const int tid2 = threadIdx.x;
    const int sr = tid2 >> 2, sq = tid2 & 3;  // staging: rows sr and sr + 64, float4 sq of the chunk
    const int mt = tm * 32 * TM * WM, nt = tn * 32 * TN * WN;
    int say[2], sax[2];
    long saoff[2];
    const float* sbrow[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      int img, oy, ox;
      cgl_conv_pix(P, min(mt + sr + 64 * h, M - 1), img, oy, ox);
      say[h] = oy * P->isy;
      sax[h] = ox * P->isx;
      saoff[h] = (long)img * P->XH * XW * Cin;
      sbrow[h] = P->Wp + (long)min(nt + sr + 64 * h, N - 1) * Kp;
    }
    auto gload = [&](int c, f32x4 (&ra)[2], f32x4 (&rb)[2], int& okm) {
      const int k0 = c * 16, t = k0 / Cin, ci = k0 - t * Cin + 4 * sq;
      const int ty = t / Tx, tx = t - ty * Tx;
      const int dyv = P->dy[ty], dxv = P->dx[tx];
      okm = 0;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int iy = say[h] + dyv, ix = sax[h] + dxv;
        const bool ok = (unsigned)iy < (unsigned)IH && (unsigned)ix < (unsigned)IW;
        okm |= ok ? (1 << h) : 0;
        const int cy = min(max(iy, 0), IH - 1) >> ish, cx = min(max(ix, 0), IW - 1) >> ish;
        ra[h] = *(gcf4p)(X + saoff[h] + ((long)cy * XW + cx) * Cin + ci);
        rb[h] = *(gcf4p)(sbrow[h] + k0 + 4 * sq);
      }
    };
    auto stage = [&](int buf, const f32x4 (&ra)[2], const f32x4 (&rb)[2], int okm) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        *(f32x4*)&la[(buf * 128 + sr + 64 * h) * RS + 4 * sq] = ((okm >> h) & 1) ? ra[h] : f32x4{0.f, 0.f, 0.f, 0.f};
        *(f32x4*)&lb[(buf * 128 + sr + 64 * h) * RS + 4 * sq] = rb[h];
      }
    };
    const int ra0 = wm * 32 * TM + li, rb0 = wn * 32 * TN + li;
    auto mmc = [&](int buf) {
      float A[TM][8], B[TN][8];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const float* w = &la[(buf * 128 + ra0 + 32 * i) * RS + 8 * lh];
        const f32x4 u = *(const f32x4*)w, v = *(const f32x4*)(w + 4);
        A[i][0] = u[0]; A[i][1] = u[1]; A[i][2] = u[2]; A[i][3] = u[3];
        A[i][4] = v[0]; A[i][5] = v[1]; A[i][6] = v[2]; A[i][7] = v[3];
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const float* w = &lb[(buf * 128 + rb0 + 32 * j) * RS + 8 * lh];
        const f32x4 u = *(const f32x4*)w, v = *(const f32x4*)(w + 4);
        B[j][0] = u[0]; B[j][1] = u[1]; B[j][2] = u[2]; B[j][3] = u[3];
        B[j][4] = v[0]; B[j][5] = v[1]; B[j][6] = v[2]; B[j][7] = v[3];
      }
      __builtin_amdgcn_sched_barrier(0);   // all 8 LDS reads ahead of the 32 MFMAs
      if constexpr (DT != CGL_DTYPE_F32) {
        cgl_conv_mm16<DT>(acc, A, B);
        return;
      }
#pragma unroll
      for (int q = 0; q < 8; ++q)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[i][q], B[j][q], acc[i][j], 0, 0, 0);
    };
    f32x4 r0a[2], r0b[2], r1a[2], r1b[2];
    int ok0, ok1;
    gload(0, r0a, r0b, ok0);
    gload(min(1, nch - 1), r1a, r1b, ok1);
    stage(0, r0a, r0b, ok0);
    __syncthreads();
    int c = 0;
    for (; c + 2 <= nch; c += 2) {
      gload(min(c + 2, nch - 1), r0a, r0b, ok0);
      mmc(0);
      stage(1, r1a, r1b, ok1);
      __syncthreads();
      gload(min(c + 3, nch - 1), r1a, r1b, ok1);
      mmc(1);
      stage(0, r0a, r0b, ok0);
      __syncthreads();
    }
    if (c < nch) mmc(0);
  } else if constexpr (HALO) {
    // LDS-staged input window (the phase-form upsampling conv: 4 output parities x 2x2 taps, all reading one
    // low-res window).  The workgroup's tile is 64 enumerated rows = R = 64 / OW whole low-res rows of one
    // image; its window (rows y0 - 1 .. y0 + R, columns -1 .. OW, every channel, zeros outside the image) is
    // loaded once -- with the folded BatchNorm applied here, once per element -- and the 4 waves (one per
    // parity) read their A fragments of every tap from it.  The chunk order and MFMA sequence are the
    // direct path's, so the results are bitwise equal.
    const int OWp = P->OW, hwp = P->OH * OWp;
    const int img = m0 / hwp, y0 = (m0 - img * hwp) / OWp;
    const int WC = OWp + 2, WR = 64 / OWp + 2, CS = Cin + 4;   // pixel stride padded (LDS banks)
    const int c4 = Cin >> 2;
    const float* __restrict__ Xi = X + (long)img * P->XH * XW * Cin;
    const int g = BNIN ? min(img / L->in_gimg, L->in_groups - 1) : 0;
    // BNIN: when the staging stride keeps each thread on one channel quad, its scale / shift are loaded once
    const bool qfix = (256 % c4) == 0;
    // the activation flag and slope in registers: read through the kernarg pointer inside the loop, the slope's
    // scalar load sat under the LeakyReLU condition and became a branch per value
    const float in_sl = BNIN ? cgl_bnin_slope(L) : 0.f;
    f32x4 sc0 = {0.f, 0.f, 0.f, 0.f}, sh0 = sc0;
    if (BNIN && qfix) {
      sc0 = *(gcf4p)(L->in_coef + g * Cin + 4 * (tid % c4));
      sh0 = *(gcf4p)(L->in_coef + (L->in_groups + g) * Cin + 4 * (tid % c4));
    }
    // SB staging loads in flight per thread (a load-then-store loop kept ~2 in flight: ~7 serial round trips for
    // a 57 KB window), then the transform and the LDS stores
    constexpr int SB = CGL_HALO_SB;
    const int tot = WR * WC * c4;
    for (int e0 = tid; e0 < tot; e0 += 256 * SB) {
      f32x4 v[SB];
      int okm = 0;
#pragma unroll
      for (int u = 0; u < SB; ++u) {
        const int e = e0 + 256 * u;
        const int q = e % c4, pix = e / c4;
        const int wr = pix / WC, wc = pix - wr * WC;
        const int iy = y0 - 1 + wr, ix = wc - 1;
        v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (e < tot && (unsigned)iy < (unsigned)IH && (unsigned)ix < (unsigned)IW) {
          v[u] = *(gcf4p)(Xi + ((long)iy * XW + ix) * Cin + 4 * q);
          okm |= 1 << u;
        }
      }
#pragma unroll
      for (int u = 0; u < SB; ++u) {
        const int e = e0 + 256 * u;
        if (e >= tot) break;
        const int q = e % c4, pix = e / c4;
        if constexpr (BNIN) {
          if ((okm >> u) & 1) {
            const f32x4 sc = qfix ? sc0 : *(gcf4p)(L->in_coef + g * Cin + 4 * q);
            const f32x4 sh = qfix ? sh0 : *(gcf4p)(L->in_coef + (L->in_groups + g) * Cin + 4 * q);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
              float w = fmaf(v[u][t], sc[t], sh[t]);
              w = fmaxf(w, w * in_sl);
              v[u][t] = w;
            }
          }
        }
        *(f32x4*)(s_red + pix * CS + 4 * q) = v[u];
      }
    }
    __syncthreads();
    // this lane's window pixel (tap offset 0) per row block
    int wpix[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int rr = 32 * i + li;                   // row within the tile
      wpix[i] = (rr / OWp + 1) * WC + (rr % OWp) + 1;
    }
    auto lda = [&](int c, float (&A)[TM][8]) {
      const int k0 = c * 16, t = k0 / Cin, ci = k0 - t * Cin + 8 * lh;
      const int ty = t / Tx, tx = t - ty * Tx;
      const int toff = P->dy[ty] * WC + P->dx[tx];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const float* w = s_red + (wpix[i] + toff) * CS + ci;
        const f32x4 u = *(const f32x4*)w, v = *(const f32x4*)(w + 4);
        A[i][0] = u[0]; A[i][1] = u[1]; A[i][2] = u[2]; A[i][3] = u[3];
        A[i][4] = v[0]; A[i][5] = v[1]; A[i][6] = v[2]; A[i][7] = v[3];
      }
    };
    auto ldb = [&](int c, float (&B)[TN][8]) {
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        gcfp p = (gcfp)(brow[j] + c * 16 + 8 * lh);
        const f32x4 u = *(gcf4p)p, w = *(gcf4p)(p + 4);
        B[j][0] = u[0]; B[j][1] = u[1]; B[j][2] = u[2]; B[j][3] = u[3];
        B[j][4] = w[0]; B[j][5] = w[1]; B[j][6] = w[2]; B[j][7] = w[3];
      }
    };
    auto mm = [&](float (&A)[TM][8], float (&B)[TN][8]) {
      if constexpr (DT != CGL_DTYPE_F32) {
        cgl_conv_mm16<DT>(acc, A, B);
        return;
      }
#pragma unroll
      for (int q = 0; q < 8; ++q)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[i][q], B[j][q], acc[i][j], 0, 0, 0);
    };
    // B (weights, global) S - 1 chunks ahead in a rotation of S register sets, A (LDS) one chunk ahead
    float xb[S][TN][8], xa[2][TM][8];
#pragma unroll
    for (int s2 = 0; s2 < S; ++s2) ldb(min(s2, nch - 1), xb[s2]);
    lda(0, xa[0]);
    int c = 0;
    for (; c + S <= nch; c += S) {
#pragma unroll
      for (int s2 = 0; s2 < S; ++s2) {
        lda(min(c + s2 + 1, nch - 1), xa[(s2 + 1) & 1]);
        mm(xa[s2 & 1], xb[s2]);
        ldb(min(c + s2 + S, nch - 1), xb[s2]);
      }
      if (S & 1) {   // keep the A double buffer's parity aligned with s2 = 0 at the next iteration
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int q = 0; q < 8; ++q) xa[0][i][q] = xa[1][i][q];
      }
    }
#pragma unroll
    for (int s2 = 0; s2 < S - 1; ++s2)
      if (c + s2 < nch) {
        lda(min(c + s2 + 1, nch - 1), xa[(s2 + 1) & 1]);
        mm(xa[s2 & 1], xb[s2]);
      }
  } else if (cb < ce) {
    float xa[S][TM][8], xb[S][TN][8];
    int okm[S];
#pragma unroll
    for (int s = 0; s < S; ++s) load(min(cb + s, ce - 1), xa[s], xb[s], okm[s]);
    int c = cb;
    for (; c + S <= ce; c += S) {
#pragma unroll
      for (int s = 0; s < S; ++s) {
        compute(xa[s], xb[s], okm[s]);
        load(min(c + s + S, ce - 1), xa[s], xb[s], okm[s]);
      }
    }
#pragma unroll
    for (int s = 0; s < S - 1; ++s)
      if (c + s < ce) compute(xa[s], xb[s], okm[s]);
  }
  // k-split reduction through LDS in a fixed order (wk = 1, 2, 3 added to wk = 0): deterministic
  if (WK > 1) {
    constexpr int NB = TM * TN;
    if (wk > 0) {
      float* dst = s_red + ((wmn * (WK - 1) + (wk - 1)) * NB * 16) * 64;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) dst[((i * TN + j) * 16 + r) * 64 + lane] = acc[i][j][r];
    }
    __syncthreads();
    if (wk > 0) return;
    for (int q = 1; q < WK; ++q) {
      const float* src = s_red + ((wmn * (WK - 1) + (q - 1)) * NB * 16) * 64;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[i][j][r] += src[((i * TN + j) * 16 + r) * 64 + lane];
    }
  }

  // epilogue: bias, activation, Dropout2d scale, NHWC store at the mapped position.  The activation
  // is a uniform branch around the element loops; the output pixel of each row is decoded once per
  // 32-row block and stepped from row to row (no per-element divisions); the Dropout2d multipliers of
  // a block are all loaded before its stores (a load after a store may alias it, which would
  // serialise one global round trip per element).
  const int ldy = P->ldy, YH = P->YH, YW = P->YW, OW = P->OW, hw = P->OH * P->OW;
  const double inv_hw = 1.0 / hw, inv_ow = 1.0 / OW;
  const int osy = P->osy, osx = P->osx, ooy = P->ooy, oox = P->oox;
  const float* __restrict__ bias = L->bias;
  const float* __restrict__ drop = L->drop;
  const int act = L->act;
  const float sl = L->slope;
  float* __restrict__ Y = P->Y;
  float bj[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = min(n0 + 32 * j + li, N - 1);
    bj[j] = bias ? gld(bias + col) : 0.f;
  }
#define CGL_EPI_LOOP(EXPR)                                  \
  _Pragma("unroll") for (int i = 0; i < TM; ++i)            \
  _Pragma("unroll") for (int j = 0; j < TN; ++j)            \
  _Pragma("unroll") for (int r = 0; r < 16; ++r) {          \
    float v = acc[i][j][r] + bj[j];                         \
    EXPR;                                                   \
    acc[i][j][r] = v;                                       \
  }
  if (act == CGL_EPI_ACT_LEAKY) { CGL_EPI_LOOP(v = v > 0.f ? v : v * sl) }
  else if (act == CGL_EPI_ACT_TANH) { CGL_EPI_LOOP(v = cgl_tanh(v)) }
  else if (act == CGL_EPI_ACT_SIGMOID) { CGL_EPI_LOOP(v = 1.f / (1.f + expf(-v))) }
  else { CGL_EPI_LOOP((void)0) }
#undef CGL_EPI_LOOP
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int rowb = m0 + 32 * i;               // wave-uniform first row of the block
    if (rowb >= M) break;
    const int row0 = rowb + 4 * lh;
    int pix[16];
    auto decode = [&](int r, int& img) {
      const int row = row0 + (r & 3) + 8 * (r >> 2);
      int rem, oy, ox;
      cgl_divmod(row, hw, inv_hw, img, rem);
      cgl_divmod(rem, OW, inv_ow, oy, ox);
      pix[r] = (img * YH + oy * osy + ooy) * YW + ox * osx + oox;
      return row;
    };
    if (drop) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int img;
        const int row = decode(r, img);
        const long dro = (long)(row < M ? img : 0) * ldy;
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j][r] *= gld(drop + dro + min(n0 + 32 * j + li, N - 1));
      }
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int img;
        decode(r, img);
      }
    }
    // BatchNorm2d statistics of the stored values (the next op's BatchNorm, cgl_bn2d_fwd_stats): per
    // 32-row chunk and channel {sum, M2 about the chunk mean} in double, the two lane halves
    // combined by one xor-32 exchange (fixed order); the chunks of a forward call are contiguous
    int imb, remb, oyb, oxb;
    cgl_divmod(rowb, hw, inv_hw, imb, remb);
    cgl_divmod(remb, OW, inv_ow, oyb, oxb);
    const int pixb = __builtin_amdgcn_readfirstlane((imb * YH + oyb * osy + ooy) * YW + oxb * osx + oox);
    if (L->st_part && L->st_mode == 1) {
      // backward statistics (cgl_bn2d_bwd_stats): x and post loaded at the stored positions through
      // buffer resources of the same base (every row of a statistics launch is valid)
      const int g = rowb / P->st_gr;
      const long chunk = (long)g * L->st_cpg + P->st_off + (rowb - g * P->st_gr) / 32;
      const auto rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(L->st_x) + (long)pixb * ldy, (short)0,
                                                        0x7fffffff, 0x00020000);
      const float* pp = L->st_post ? L->st_post : L->st_x;
      const auto rp = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(pp) + (long)pixb * ldy, (short)0,
                                                        0x7fffffff, 0x00020000);
      const float psl = L->st_slope;
      const bool psc = L->st_psc != nullptr;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int col = n0 + 32 * j + li;
        const int colc = min(col, N - 1);
        const float mu = gld(L->st_mean + (long)g * N + colc);
        const float sc = psc ? gld(L->st_psc + colc) : 0.f, sh = psc ? gld(L->st_psc + L->st_psc_ld + colc) : 0.f;
        float xv[16], pv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int off = ((pix[r] - pixb) * ldy + colc) * 4;
          xv[r] = __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(rx, off, 0, 0));
          if (!psc) pv[r] = __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(rp, off, 0, 0));
        }
        if (psc) {
#pragma unroll
          for (int r = 0; r < 16; ++r) pv[r] = fmaf(xv[r], sc, sh);
        }
        const bool pon = psc || L->st_post;
        double S = 0.0, D = 0.0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float y = acc[i][j][r];
          const float gg = pon ? (pv[r] > 0.f ? y : y * psl) : y;
          S += (double)gg;
          D += (double)(gg * (xv[r] - mu));
        }
        S += __shfl_xor(S, 32);
        D += __shfl_xor(D, 32);
        if (lh == 0 && col < N) {
          double* dst = L->st_part + (chunk * N + col) * 2;
          dst[0] = S;
          dst[1] = D;
        }
      }
    } else if (L->st_part && L->st_nv && rowb < P->st_gr && rowb + 32 > min(gldi(L->st_nv), P->st_gr / hw) * hw) {
      // a chunk of the short first call that holds padding rows: {sum, M2 about the mean} over its real rows
      // only (the finalize derives every chunk's count from the same *st_nv)
      const int nvr = min(gldi(L->st_nv), P->st_gr / hw) * hw;
      const long chunk = P->st_off + rowb / 32;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        double sm = 0.0, cn = 0.0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const bool in = row0 + (r & 3) + 8 * (r >> 2) < nvr;
          sm += in ? (double)acc[i][j][r] : 0.0;
          cn += in ? 1.0 : 0.0;
        }
        sm += __shfl_xor(sm, 32);
        cn += __shfl_xor(cn, 32);
        const double mu = cn > 0.0 ? sm / cn : 0.0;
        double m2 = 0.0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const double dd = (double)acc[i][j][r] - mu;
          m2 += row0 + (r & 3) + 8 * (r >> 2) < nvr ? dd * dd : 0.0;
        }
        m2 += __shfl_xor(m2, 32);
        const int col = n0 + 32 * j + li;
        if (lh == 0 && col < N) {
          double* dst = L->st_part + (chunk * N + col) * 2;
          dst[0] = sm;
          dst[1] = m2;
        }
      }
    } else if (L->st_part) {
      const int g = rowb / P->st_gr;
      const long chunk = (long)g * L->st_cpg + P->st_off + (rowb - g * P->st_gr) / 32;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        double sm = 0.0;
#pragma unroll
        for (int r = 0; r < 16; ++r) sm += (double)acc[i][j][r];
        sm += __shfl_xor(sm, 32);
        const double mu = sm * (1.0 / 32.0);
        double m2 = 0.0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const double dd = (double)acc[i][j][r] - mu;
          m2 += dd * dd;
        }
        m2 += __shfl_xor(m2, 32);
        const int col = n0 + 32 * j + li;
        if (lh == 0 && col < N) {
          double* dst = L->st_part + (chunk * N + col) * 2;
          dst[0] = sm;
          dst[1] = m2;
        }
      }
    }
    // stores through a buffer resource based at the block's first output pixel (output pixels grow
    // with the row, so every offset is >= 0): rows past M / columns past N get an out-of-range
    // offset and are dropped by the hardware -- no per-element branches
    const auto rs = __builtin_amdgcn_make_buffer_rsrc(Y + (long)pixb * ldy, (short)0, 0x7fffffff, 0x00020000);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const bool rok = row0 + (r & 3) + 8 * (r >> 2) < M;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int col = n0 + 32 * j + li;
        const int off = (rok && col < N) ? ((pix[r] - pixb) * ldy + col) * 4 : (int)0x80000000;
        // (through a scalar copy: a bit_cast of the vector element itself was lowered to element 0)
        const float v = acc[i][j][r];
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_int(v), rs, off, 0, 0);
      }
    }
  }
}

template <int TM, int TN, bool FAST, bool BNIN = false, bool LDSM = false, int DT = CGL_DTYPE_F32>
__global__ __launch_bounds__(256) void cgl_conv_fwd(CglConvLaunch args) {
  (void)args;
  extern __shared__ float cgl_conv_lds[];
  CglKL L = cgl_conv_args();
  const int bid = blockIdx.x;
  if (L->ilv) {
    // problems sharing one input (the 4 output parities of an upsampling conv in phase form, the
    // input-parity problems of a stride-2 input gradient): unit u = (tile u / np of problem u % np),
    // units XCD-contiguous, so the np tiles reading one input window run back to back in one L2
    const int np = L->np;
    const int unit = cgl_xcd_tile(bid, L->p[0].tiles_m * L->p[0].tiles_n * np);
    cgl_conv_fwd_body<TM, TN, FAST, BNIN, false, LDSM, DT>(L, &L->p[unit % np], unit / np, cgl_conv_lds, true);
    return;
  }
  const int pi = cgl_conv_prob(L, bid);
  CglKP P = &L->p[pi];
  cgl_conv_fwd_body<TM, TN, FAST, BNIN, false, LDSM, DT>(L, P, bid - P->wg_begin, cgl_conv_lds);
}

// The phase-form upsampling conv with its input window staged in LDS (HALO path of cgl_conv_fwd_body): one
// workgroup per (64-row tile, 64-output-channel slice), its 4 waves = the 4 output-parity problems
// (launch_conv_mma: conv_halo_ok).
template <bool BNIN, int DT = CGL_DTYPE_F32>
__global__ __launch_bounds__(256) void cgl_conv_fwd_halo(CglConvLaunch args) {
  (void)args;
  extern __shared__ float cgl_conv_lds[];
  CglKL L = cgl_conv_args();
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // XCD-contiguous tile order: the N-halves of one row tile and vertically adjacent tiles (which share
  // window rows) run on one XCD's L2
  CglKP P = &L->p[wave];
  cgl_conv_fwd_body<2, 2, true, BNIN, true, false, DT>(L, P, cgl_xcd_tile(blockIdx.x, P->tiles_m * P->tiles_n),
                                                        cgl_conv_lds, true);
}

// ------------------------------------------------------------------------------------------
// Weight gradient: part[s][n][k] = sum over the pixels m of split s of dY[pos(m)][n] * A[m][k]
// (A = the tap table's implicit im2col of X).  Rows of the result tile are output channels
// (operand A = dY, 32 consecutive channels of one pixel per lane group: coalesced), columns are
// im2col columns (operand B, consecutive channels of one tap: coalesced); each lane half takes 8
// consecutive pixels of a 16-pixel chunk (the MFMA k permutation of cgl_gemm.hip).
// Work unit = one wave: (tile, split) with a (32 TM) x (32 TN) result tile; a workgroup runs 4
// consecutive units (no LDS, no barriers), so small layers (Conv2d(1, 16): 16 x 9 results) do not
// pay for a large workgroup tile.
// Read-only zeros: operand loads of padded taps / pixels past M point here instead of being masked
// after the load (saves the mask bookkeeping and the per-MFMA-operand selects of the k-loop).  The
// loads index it with an output channel (< N) or an input channel (< Cin), so it covers
// CGL_ZERO_PAGE floats; conv_bwd_weight_impl refuses larger layers (dense layers reach N = 8192).
#define CGL_ZERO_PAGE 65536
static __device__ float cgl_zero_page[CGL_ZERO_PAGE];   // (one per translation unit that holds these kernels)

// ROW: every problem of the launch has OW % 8 == 0 and M % 16 == 0, so the 8 pixels of a lane
// half are always valid and lie in one output row: one pixel decode per chunk, constant address
// strides along the row, the tap's row bounds checked once (a fraction of the generic path's VALU).
// BNIN: X is the PRE-BatchNorm map (groups of L->in_gimg images, scale / shift in L->in_coef): each valid
// im2col value is fmaf(x, scale, shift) (+ LeakyReLU), cgl_eltwise's arithmetic; padded taps stay zero
// DT: as in cgl_conv_fwd_body -- the finished dY / im2col fragments (the BatchNorm applied, the bias column's ones
// set) are rounded to bf16 as they enter the MFMA, so the bias column sums the ROUNDED dY
template <int TM, int TN, bool ROW, bool BNIN = false, int DT = CGL_DTYPE_F32>
__device__ __forceinline__ void cgl_conv_wgrad_body(CglKL L, CglKP P, int local) {
#ifndef CGL_WGRAD_S
#define CGL_WGRAD_S 2
#endif
  constexpr int S = CGL_WGRAD_S;   // operand register sets in rotation (S - 1 chunks of loads in flight)
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, li = lane & 31, lh = lane >> 5;
  const int tiles = P->tiles_m * P->tiles_n;
  const int unit = local * 4 + wave;
  if (unit >= tiles * P->splits) return;
  const int split = unit / tiles;
  const int tile = unit - split * tiles;
  const int tn = tile % P->tiles_n, tm = tile / P->tiles_n;
  const int M = P->M, N = P->N, K = P->K, Kp = P->Kp, Cin = P->Cin;
  const int IH = P->IH, IW = P->IW, ish = P->ish, XW = P->XW, XH = P->XH, Tx = P->Tx;
  const int n0 = tm * 32 * TM;
  const int k0c = tn * 32 * TN;
  const float* __restrict__ X = P->X;
  const float* __restrict__ dY = P->Y;
  const int ldy = P->ldy, YH = P->YH, YW = P->YW;
  const int osy = P->osy, osx = P->osx, ooy = P->ooy, oox = P->oox, isy = P->isy, isx = P->isx;
  const int OH = P->OH, OW = P->OW;

  int rch[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) rch[i] = min(n0 + 32 * i + li, N - 1);
  int cdy[TN], cdx[TN], cci[TN];
  bool cok[TN], cone[TN];
  const int wbias = L->wbias;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int kc = k0c + 32 * j + li;
    cok[j] = kc < K;
    cone[j] = wbias && kc == K;   // the bias column: B = 1 for every valid pixel
    const int kk = min(kc, K - 1);
    const int t = kk / Cin;
    cci[j] = kk - t * Cin;
    const int ty = t / Tx, tx = t - ty * Tx;
    cdy[j] = P->dy[ty];
    cdx[j] = P->dx[tx];
  }
  // BNIN: this lane's columns' scale / shift for up to two BatchNorm groups (the D step's two calls: group
  // in_g0 + img / in_gimg)
  float bsc[2][TN], bsh[2][TN];
  const int bg = BNIN ? max(1, min(L->in_groups - L->in_g0, 2)) : 1;
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const long gq = L->in_g0 + min(q, bg - 1);
      bsc[q][j] = BNIN ? gld(L->in_coef + gq * Cin + cci[j]) : 0.f;
      bsh[q][j] = BNIN ? gld(L->in_coef + (L->in_groups + gq) * Cin + cci[j]) : 0.f;
    }
  const float in_sl = BNIN ? cgl_bnin_slope(L) : 0.f;       // (in registers: see the halo staging)
  auto bn = [&](float x, int img, int j) {
    const int q = (bg > 1 && img >= L->in_gimg) ? 1 : 0;     // (<= 2 groups: no division per value)
    float v = fmaf(x, q ? bsc[1][j] : bsc[0][j], q ? bsh[1][j] : bsh[0][j]);
    v = fmaxf(v, v * in_sl);
    return v;
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // operands of invalid pixels / out-of-bounds taps are loaded from cgl_zero_page (no masks)
  const float* __restrict__ zp = cgl_zero_page;
  auto load = [&](int c, float (&A)[TM][8], float (&B)[TN][8], int& okm) {
    okm = 0;
    if (ROW) {
      int img, oy, ox;
      cgl_conv_pix(P, c * 16 + 8 * lh, img, oy, ox);
      const float* ya0 = dY + (((long)img * YH + oy * osy + ooy) * YW + ox * osx + oox) * ldy;
      const long ystep = (long)osx * ldy;
#pragma unroll
      for (int q = 0; q < 8; ++q)
#pragma unroll
        for (int i = 0; i < TM; ++i) A[i][q] = ((gcfp)(ya0 + q * ystep))[rch[i]];
      const float* ximg = X + (long)img * XH * XW * Cin;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int iy = oy * isy + cdy[j];
        const bool rowok = cok[j] && (unsigned)iy < (unsigned)IH;
        const float* rb = ximg + (long)(rowok ? (iy >> ish) : 0) * XW * Cin + cci[j];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int ix = (ox + q) * isx + cdx[j];
          const bool ok = rowok && (unsigned)ix < (unsigned)IW;
          const float* bb = ok ? rb + (long)(ix >> ish) * Cin : zp + cci[j];
          B[j][q] = *(gcfp)bb;
          if (BNIN) B[j][q] = ok ? bn(B[j][q], img, j) : 0.f;
        }
      }
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int q = 0; q < 8; ++q) B[j][q] = cone[j] ? 1.f : B[j][q];
      return;
    }
    // decode the first pixel of this lane half once, then step along the row (wrapping)
    int img, oy, ox;
    cgl_conv_pix(P, min(c * 16 + 8 * lh, M - 1), img, oy, ox);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int m = c * 16 + 8 * lh + q;
      const bool mv = m < M;
      if (q > 0) {
        // branch-free stepping (the nested ifs compiled to divergent exec-mask branches per pixel: the lane
        // halves step different pixels)
        ++ox;
        const bool wx = ox == OW;
        ox = wx ? 0 : ox;
        oy += wx ? 1 : 0;
        const bool wy = oy == OH;
        oy = wy ? 0 : oy;
        img += wy ? 1 : 0;
        img = mv ? img : 0;
        oy = mv ? oy : 0;
        ox = mv ? ox : 0;
      }
      const long ya = (((long)img * YH + oy * osy + ooy) * YW + ox * osx + oox) * ldy;
      const float* ab = mv ? dY + ya : zp;
#pragma unroll
      for (int i = 0; i < TM; ++i) A[i][q] = ((gcfp)ab)[rch[i]];
      const long xo = (long)img * XH * XW * Cin;
      const int iyb = oy * isy, ixb = ox * isx;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int iy = iyb + cdy[j], ix = ixb + cdx[j];
        const bool ok = mv && cok[j] && (unsigned)iy < (unsigned)IH && (unsigned)ix < (unsigned)IW;
        const float* bb = ok ? X + xo + ((long)(iy >> ish) * XW + (ix >> ish)) * Cin : zp;
        B[j][q] = ((gcfp)bb)[cci[j]];
        if (BNIN) B[j][q] = ok ? bn(B[j][q], img, j) : 0.f;
        B[j][q] = cone[j] ? (mv ? 1.f : 0.f) : B[j][q];
      }
    }
  };
  auto compute = [&](float (&A)[TM][8], float (&B)[TN][8], int okm) {
    (void)okm;
    if constexpr (DT != CGL_DTYPE_F32) {
      cgl_conv_mm16<DT>(acc, A, B);
      return;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[i][q], B[j][q], acc[i][j], 0, 0, 0);
  };

  const int nchk = (M + 15) >> 4;
  const int splits = P->splits;
  const int cb = (int)(((long)split * nchk) / splits), ce = (int)(((long)(split + 1) * nchk) / splits);
  if (cb < ce) {
    float xa[S][TM][8], xb[S][TN][8];
    int okm[S];
#pragma unroll
    for (int s = 0; s < S; ++s) load(min(cb + s, ce - 1), xa[s], xb[s], okm[s]);
    int c = cb;
    for (; c + S <= ce; c += S) {
#pragma unroll
      for (int s = 0; s < S; ++s) {
        compute(xa[s], xb[s], okm[s]);
        load(min(c + s + S, ce - 1), xa[s], xb[s], okm[s]);
      }
    }
#pragma unroll
    for (int s = 0; s < S - 1; ++s)
      if (c + s < ce) compute(xa[s], xb[s], okm[s]);
  }

  float* __restrict__ part = P->part + (long)split * N * Kp;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int kc = k0c + 32 * j + li;
    if (kc >= K + wbias) continue;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = n0 + 32 * i + 4 * lh + (r & 3) + 8 * (r >> 2);
        if (n < N) gst(part + (long)n * Kp + kc, acc[i][j][r]);
      }
  }
}

template <int TM, int TN, bool ROW = false, bool BNIN = false, int DT = CGL_DTYPE_F32>
__global__ __launch_bounds__(256) void cgl_conv_wgrad(CglConvLaunch args) {
  (void)args;
  CglKL L = cgl_conv_args();
  const int bid = blockIdx.x;
  const int pi = cgl_conv_prob(L, bid);
  CglKP P = &L->p[pi];
  cgl_conv_wgrad_body<TM, TN, ROW, BNIN, DT>(L, P, bid - P->wg_begin);
}

// ------------------------------------------------------------------------------------------
// Weight gradient with LDS-staged panels (the large upsampling convs of the LSGAN generator: 16K - 64K
// pixels per phase problem, N = 64 / 128 output channels, K = 512).  A workgroup owns an R x C result tile
// (R = 64 WM output channels, C = 64 WN im2col columns; 4 waves of 2 x 2 32x32 blocks) over one pixel
// split.  Per 16-pixel chunk its 256 threads fetch the dY panel [16][R] and the im2col panel [16][C] with
// 16-byte loads (4 channels of one pixel) and stage them in LDS, where WN waves share each dY element and
// WM waves each X element: the wave-unit kernel's 4-byte fragment loads (one per MFMA operand and wave)
// become a quarter of the load instructions and 1 / WN + 1 / WM of the bytes.  Chunk c + 2's loads are in
// flight while chunk c is multiplied (two register sets, two LDS buffers, one barrier per chunk).  Same
// partials [split][N][Kp] and k permutation as cgl_conv_wgrad (pixel 8 lh + q of a chunk is lane half lh's
// k of MFMA step q), so cgl_conv_wgrad_reduce is shared.  Requirements: wgrad_lds_wm.
// KS = 2: 512-thread workgroups of two 4-wave halves that take alternate chunks of one (twice as long) pixel
// split, each half with its own LDS buffers, summed through LDS at the end (half 0 + half 1, fixed order):
// the same waves per SIMD with half the splits, so half the partials to write and to reduce.
#define CGL_WLDS_PAD 4
// BNIN: X is the PRE-BatchNorm map of one forward call (group L->in_g0): the staged im2col values are
// LeakyReLU(fmaf(x, scale, shift)) -- cgl_eltwise's arithmetic, so the panel equals the applied activation
// DT: the panels stay fp32 in LDS; a lane's 8 pixels of each panel column are rounded to bf16 as they enter the MFMA
template <int WM, int WN, int KS, bool BNIN = false, int DT = CGL_DTYPE_F32>
__global__ __launch_bounds__(256 * KS, 2 / KS) void cgl_conv_wgrad_lds(CglConvLaunch args) {
  (void)args;
  static_assert(KS == 1 || KS == 2, "one or two halves");
  static_assert(DT == CGL_DTYPE_F32 || DT == CGL_DTYPE_BF16, "fp32 or bf16 MFMA operands");
  constexpr int R = 64 * WM, C = 64 * WN;
  constexpr int RP = R + CGL_WLDS_PAD, CP = C + CGL_WLDS_PAD;   // padded rows: the lane halves (8 rows
                                                                 // apart) land on disjoint banks
  constexpr int FA = R / 4, FB = C / 4;                          // float4 per pixel row of each panel
  constexpr int NA = 16 * FA / 256, NB = 16 * FB / 256;          // float4 loads per thread and chunk
  static_assert(WM * WN == 4 && NA >= 1 && NB >= 1, "4 waves, whole panels");
  constexpr int HALF = 2 * 16 * (RP + CP);                       // one half's two A and two B buffers
  static_assert(KS == 1 || KS * HALF >= 256 * 64, "the halves' merge reuses the staging LDS");
  __shared__ __attribute__((aligned(16))) float pool[KS * HALF];
  CglKL L = cgl_conv_args();
  const int pi = cgl_conv_prob(L, blockIdx.x);
  CglKP P = &L->p[pi];
  const int tiles = P->tiles_m * P->tiles_n;
  const int local = cgl_xcd_tile(blockIdx.x - P->wg_begin, tiles * P->splits);
  const int split = local / tiles, tile = local - split * tiles;
  const int n0 = (tile / P->tiles_n) * R, k0 = (tile % P->tiles_n) * C;
  const int half = KS == 1 ? 0 : __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 8);
  const int tid = threadIdx.x & 255;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, li = lane & 31, lhf = lane >> 5;
  const int wm = wave / WN, wn = wave - (wave / WN) * WN;
  float* const sa0 = pool + half * HALF;                          // [2][16 RP]
  float* const sb0 = sa0 + 2 * 16 * RP;                           // [2][16 CP]
  const int N = P->N, Kp = P->Kp, Cin = P->Cin;
  const int IH = P->IH, IW = P->IW, ish = P->ish, XW = P->XW, XH = P->XH;
  const int ldy = P->ldy, YH = P->YH, YW = P->YW;
  const int osy = P->osy, osx = P->osx, ooy = P->ooy, oox = P->oox, isy = P->isy, isx = P->isx;
  const int lw = __builtin_ctz(P->OW), lhw = __builtin_ctz(P->OW) + __builtin_ctz(P->OH);
  const int mw = P->OW - 1, mh = P->OH - 1;
  const float* __restrict__ X = P->X;
  const float* __restrict__ dY = P->Y;
  // this thread's fixed panel columns: dY channel n0 + 4 fa, im2col columns k0 + 4 fb .. + 3 (one tap)
  const int fa = tid % FA, pa = tid / FA;
  const int fb = tid % FB, pb = tid / FB;
  const int kk = k0 + 4 * fb;
  const int tap = kk / Cin, ci = kk - tap * Cin;
  const int cdy = P->dy[tap / P->Tx], cdx = P->dx[tap - (tap / P->Tx) * P->Tx];
  f32x4 bsc = {0.f, 0.f, 0.f, 0.f}, bsh = bsc;
  const float in_sl = BNIN ? cgl_bnin_slope(L) : 0.f;       // (in registers: see the halo staging)
  if constexpr (BNIN) {
    bsc = *(gcf4p)(L->in_coef + (long)L->in_g0 * Cin + ci);
    bsh = *(gcf4p)(L->in_coef + (long)(L->in_groups + L->in_g0) * Cin + ci);
  }
  // A 16-pixel chunk never crosses an image (OH OW >= 16, powers of two): pixel c 16 + p decodes as the chunk's
  // (img0, oy0, ox0) -- uniform, scalar -- plus (p >> lw, p & mw) without carries, so each load slot keeps a
  // constant element offset from the chunk's base pointer and only the X bounds test is per chunk and lane.
  int aoff[NA], bky[NB], bkx[NB], boff[NB];
#pragma unroll
  for (int r = 0; r < NA; ++r) {
    const int p = pa + (256 / FA) * r, py = p >> lw, px = p & mw;
    aoff[r] = (py * osy * YW + px * osx) * ldy + n0 + 4 * fa;
  }
#pragma unroll
  for (int r = 0; r < NB; ++r) {
    const int p = pb + (256 / FB) * r, py = p >> lw, px = p & mw;
    bky[r] = py * isy + cdy;
    bkx[r] = px * isx + cdx;
    boff[r] = (bky[r] * XW + bkx[r]) * Cin + ci;
  }
  (void)ish; (void)XH;

  // (the out-of-bounds taps' zeros are applied when staging, so nothing waits on a load before the MFMAs)
  auto load = [&](int c, f32x4 (&ra)[NA], f32x4 (&rb)[NB], int& okb) {
    const int m0 = c * 16;
    const int img0 = m0 >> lhw, oy0 = (m0 >> lw) & mh, ox0 = m0 & mw;
    const float* ya = dY + ((long)(img0 * YH + oy0 * osy + ooy) * YW + ox0 * osx + oox) * ldy;
#pragma unroll
    for (int r = 0; r < NA; ++r) ra[r] = *(gcf4p)(ya + aoff[r]);
    const int Y0 = oy0 * isy, X0 = ox0 * isx;
    const float* xa = X + ((long)img0 * XH * XW + (long)Y0 * XW + X0) * Cin;
    okb = 0;
#pragma unroll
    for (int r = 0; r < NB; ++r) {
      const bool ok = (unsigned)(Y0 + bky[r]) < (unsigned)IH && (unsigned)(X0 + bkx[r]) < (unsigned)IW;
      okb |= ok ? (1 << r) : 0;
      rb[r] = *(gcf4p)(ok ? xa + boff[r] : X + ci);
    }
  };
  auto stage = [&](int buf, const f32x4 (&ra)[NA], const f32x4 (&rb)[NB], int okb) {
#pragma unroll
    for (int r = 0; r < NA; ++r) *(f32x4*)&sa0[buf * 16 * RP + (pa + (256 / FA) * r) * RP + 4 * fa] = ra[r];
#pragma unroll
    for (int r = 0; r < NB; ++r) {
      f32x4 v = rb[r];
      if constexpr (BNIN) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          float w = fmaf(v[u], bsc[u], bsh[u]);
          w = fmaxf(w, w * in_sl);
          v[u] = w;
        }
      }
      *(f32x4*)&sb0[buf * 16 * CP + (pb + (256 / FB) * r) * CP + 4 * fb] =
          ((okb >> r) & 1) ? v : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  // all 32 operands of the chunk are read from LDS before the first MFMA (the reads of step q + 1 do not
  // wait behind step q's MFMAs; the waits are progressive)
  auto compute = [&](int buf) {
    const float* A = &sa0[buf * 16 * RP + 8 * lhf * RP + wm * 64 + li];
    const float* B = &sb0[buf * 16 * CP + 8 * lhf * CP + wn * 64 + li];
    if constexpr (DT != CGL_DTYPE_F32) {
      float a[2][8], b[2][8];   // [block][pixel q of this lane half]: the 16-bit MFMA's fragment
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        a[0][q] = A[q * RP];
        a[1][q] = A[q * RP + 32];
        b[0][q] = B[q * CP];
        b[1][q] = B[q * CP + 32];
      }
      __builtin_amdgcn_sched_barrier(0);
      cgl_conv_mm16<DT>(acc, a, b);
      return;
    }
    float a[8][2], b[8][2];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      a[q][0] = A[q * RP];
      a[q][1] = A[q * RP + 32];
      b[q][0] = B[q * CP];
      b[q][1] = B[q * CP + 32];
    }
    __builtin_amdgcn_sched_barrier(0);   // keep the reads ahead (the scheduler would sink them to their MFMAs)
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q][0], b[q][0], acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q][0], b[q][1], acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q][1], b[q][0], acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q][1], b[q][1], acc[1][1], 0, 0, 0);
    }
  };

  const int nchk = P->M >> 4, splits = P->splits;
  const int cb = (int)(((long)split * nchk) / splits), ce = (int)(((long)(split + 1) * nchk) / splits);
  // this half's chunks: cb + half + KS i, i < ni (the same count for both halves: every barrier is shared;
  // a half whose last chunk lies past ce loads a clamped one and skips its MFMAs)
  const int ni = (ce - cb + KS - 1) / KS;
  auto chunk = [&](int i) { return min(cb + half + KS * i, ce - 1); };
  auto live = [&](int i) { return cb + half + KS * i < ce; };
  if (ni > 0) {
    f32x4 r0a[NA], r0b[NB], r1a[NA], r1b[NB];
    int ok0, ok1;
    load(chunk(0), r0a, r0b, ok0);
    load(chunk(min(1, ni - 1)), r1a, r1b, ok1);
    stage(0, r0a, r0b, ok0);
    __syncthreads();
    int i = 0;
    for (; i + 2 <= ni; i += 2) {
      // buffer 0 holds step i, r1 step i + 1
      load(chunk(min(i + 2, ni - 1)), r0a, r0b, ok0);
      if (KS == 1 || live(i)) compute(0);   // (KS 1: no branch, so the staging interleaves with the MFMAs)
      stage(1, r1a, r1b, ok1);
      __syncthreads();
      load(chunk(min(i + 3, ni - 1)), r1a, r1b, ok1);
      if (KS == 1 || live(i + 1)) compute(1);
      stage(0, r0a, r0b, ok0);
      __syncthreads();
    }
    if (i < ni && (KS == 1 || live(i))) compute(0);   // an odd last step
  }
  if constexpr (KS == 2) {
    // half 1 hands its accumulators to half 0 through the (now idle) staging LDS
    __syncthreads();
    if (half == 1) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) pool[((i * 2 + j) * 16 + r) * 256 + tid] = acc[i][j][r];
    }
    __syncthreads();
    if (half == 1) return;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] += pool[((i * 2 + j) * 16 + r) * 256 + tid];
  }
  float* __restrict__ part = P->part + (long)split * N * Kp;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int kc = k0 + wn * 64 + 32 * j + li;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = n0 + wm * 64 + 32 * i + 4 * lhf + (r & 3) + 8 * (r >> 2);
        gst(part + (long)n * Kp + kc, acc[i][j][r]);
      }
  }
}

// ------------------------------------------------------------------------------------------
// The launch record (cgl_conv_last_launches): every launch site of the conv path stores what it launches, through
// CGL_LAUNCH -- the kernel's id, its template arguments written out beside the instantiation they name, and the
// grid / block / LDS expressions of the launch itself (evaluated once, for both).  The record repeats no selection
// condition: it is filled where the launch is, so it is what was launched.  Host only, per thread.
void cgl_conv_rec_push(const cgl_conv_launch_rec& r);   // (defined with the host dispatch below)
void cgl_conv_rec_clear();

// the launch descriptor's own fields (what the kernel is given, not how it was chosen)
inline int cgl_conv_rec_lflags(const CglConvLaunch& L) {
  return (L.st_part ? (L.st_mode ? CGL_LF_STATS_BWD : CGL_LF_STATS_FWD) : 0) | (L.st_nv ? CGL_LF_NVALID : 0) |
         (L.wbias ? CGL_LF_BIAS_COL : 0) | (L.ilv ? CGL_LF_ILV : 0);
}

inline void cgl_conv_rec_w(int kernel, int tm, int tn, int wm, int wn, int wk, int flags, dim3 grid, dim3 block,
                           size_t lds, int np, int splits) {
  cgl_conv_launch_rec r;
  r.kernel = kernel; r.tm = tm; r.tn = tn; r.wm = wm; r.wn = wn; r.wk = wk; r.flags = flags;
  r.grid = (int)(grid.x * grid.y * grid.z); r.block = (int)(block.x * block.y * block.z); r.lds_bytes = (int)lds;
  r.np = np; r.splits = splits;
  cgl_conv_rec_push(r);
}

inline void cgl_conv_rec(int kernel, int tm, int tn, int flags, dim3 grid, dim3 block, size_t lds,
                         const CglConvLaunch* L = nullptr, int splits = 0) {
  if (L)
    cgl_conv_rec_w(kernel, tm, tn, L->WM, L->WN, L->WK, flags | cgl_conv_rec_lflags(*L), grid, block, lds, L->np,
                   splits);
  else cgl_conv_rec_w(kernel, tm, tn, 0, 0, 0, flags, grid, block, lds, 1, splits);
}

// record + launch: REC = CGL_REC(kernel id, tm, tn, flags); CGL_LAUNCH_L also takes the launch descriptor (its
// waves per workgroup, problem count and runtime flags go into the record) and problem 0's pixel splits
#define CGL_REC(...) __VA_ARGS__
#define CGL_LAUNCH_L(REC, LP, SPLITS, kern, grid, block, lds, s, ...)  \
  do {                                                                \
    const dim3 cgl_g_ = (grid), cgl_b_ = (block);                     \
    const size_t cgl_l_ = (lds);                                      \
    cgl_conv_rec(REC, cgl_g_, cgl_b_, cgl_l_, (LP), (SPLITS));        \
    hipLaunchKernelGGL(kern, cgl_g_, cgl_b_, cgl_l_, s, __VA_ARGS__); \
  } while (0)
#define CGL_LAUNCH(REC, kern, grid, block, lds, s, ...) \
  CGL_LAUNCH_L(CGL_REC(REC), nullptr, 0, kern, grid, block, lds, s, __VA_ARGS__)
// cgl_conv_wgrad_lds<WM, WN, KS, BNIN, DT>: its waves come from the template (the descriptor's WM / WN / WK are 1)
#define CGL_LAUNCH_WLDS(WM_, WN_, KS_, BNIN_, DT_, wgl, threads, s, L)                                            \
  do {                                                                                                          \
    const dim3 cgl_g_ = dim3(wgl), cgl_b_ = dim3(threads);                                                      \
    cgl_conv_rec_w(CGL_K_CONV_WGRAD_LDS, 0, 0, WM_, WN_, KS_,                                                   \
                   (BNIN_ ? CGL_LF_BNIN : 0) | (DT_ == CGL_DTYPE_BF16 ? CGL_LF_BF16 : 0) | cgl_conv_rec_lflags(L), \
                   cgl_g_, cgl_b_, 0, (L).np, (L).p[0].splits);                                                 \
    hipLaunchKernelGGL((cgl_conv_wgrad_lds<WM_, WN_, KS_, BNIN_, DT_>), cgl_g_, cgl_b_, 0, s, L);               \
  } while (0)

// ------------------------------------------------------------------------------------------
// One launcher per MFMA kernel family, a template on the operand type: the family's route table -- which template
// arguments exist, and so which kernels are instantiated -- is stated here once for fp32 and bf16.  The host
// dispatch (launch_conv_mma, conv_bwd_weight_impl in cgl_conv.hip) passes what it planned through CGL_BY_DT; each
// launcher stores the launch record, launches, and returns hipGetLastError().  A combination outside the table
// returns CGL_E_ARG: conv_tiling_for gives (TM, TN) of (2, 2), (2, 1) or (1, 1), wgrad_plan any of {1, 2} x {1, 2}
// and wgrad_lds_wm 1 or 2, so the dispatch reaches none.  The explicit instantiations (cgl_conv.hip: fp32,
// cgl_conv_bf16.hip: bf16) put each operand type's kernels into one object.
#define CGL_BY_DT(dt, fn, ...) \
  ((dt) == CGL_DTYPE_BF16 ? fn<CGL_DTYPE_BF16>(__VA_ARGS__) : fn<CGL_DTYPE_F32>(__VA_ARGS__))
#define CGL_LF_OF_DT(DT_) (DT_ == CGL_DTYPE_BF16 ? CGL_LF_BF16 : 0)

// the forward's LDS-staged operand panels (LDSM): A and B, two buffers of [128][20] floats each
constexpr int CGL_CONV_LDSM_BYTES = 2 * 2 * 128 * 20 * 4;

// cgl_conv_fwd on wg workgroups with lds bytes of LDS (CGL_CONV_LDSM_BYTES when ldsm)
template <int DT>
int cgl_conv_fwd_launch(int tm, int tn, bool fast, bool bnin, bool ldsm, int wg, int lds, hipStream_t s,
                        const CglConvLaunch& L) {
#define CGL_FWD(TM, TN, FAST, BNIN, LDSM)                                                                         \
  CGL_LAUNCH_L(CGL_REC(CGL_K_CONV_FWD, TM, TN,                                                                    \
                       CGL_LF_OF_DT(DT) | (FAST ? CGL_LF_FAST : 0) | (BNIN ? CGL_LF_BNIN : 0) | (LDSM ? CGL_LF_LDSM : 0)), \
               &L, 0, (cgl_conv_fwd<TM, TN, FAST, BNIN, LDSM, DT>), dim3(wg), dim3(256), lds, s, L)
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

template <int DT>
int cgl_conv_fwd_halo_launch(bool bnin, int grid, int lds, hipStream_t s, const CglConvLaunch& L) {
#define CGL_HALO(BNIN)                                                                                         \
  CGL_LAUNCH_L(CGL_REC(CGL_K_CONV_FWD_HALO, 0, 0, CGL_LF_OF_DT(DT) | CGL_LF_HALO | (BNIN ? CGL_LF_BNIN : 0)), &L, 0, \
               (cgl_conv_fwd_halo<BNIN, DT>), dim3(grid), dim3(256), lds, s, L)
  if (bnin) CGL_HALO(true);
  else CGL_HALO(false);
#undef CGL_HALO
  return (int)hipGetLastError();
}

// cgl_conv_wgrad on wg workgroups of 4 wave units
template <int DT>
int cgl_conv_wgrad_launch(int tm, int tn, bool row, bool bnin, int wg, hipStream_t s, const CglConvLaunch& L) {
#define CGL_WGK(TM, TN, ROW, BNIN)                                                                                 \
  CGL_LAUNCH_L(CGL_REC(CGL_K_CONV_WGRAD, TM, TN, CGL_LF_OF_DT(DT) | (ROW ? CGL_LF_ROW : 0) | (BNIN ? CGL_LF_BNIN : 0)), \
               &L, L.p[0].splits, (cgl_conv_wgrad<TM, TN, ROW, BNIN, DT>), dim3(wg), dim3(256), 0, s, L)
#define CGL_WG(TM, TN)                              \
  do {                                              \
    if (row && bnin) CGL_WGK(TM, TN, true, true);   \
    else if (row) CGL_WGK(TM, TN, true, false);     \
    else if (bnin) CGL_WGK(TM, TN, false, true);    \
    else CGL_WGK(TM, TN, false, false);             \
  } while (0)
  if (tm == 2 && tn == 2) CGL_WG(2, 2);
  else if (tm == 1 && tn == 2) CGL_WG(1, 2);
  else if (tm == 2 && tn == 1) CGL_WG(2, 1);
  else if (tm == 1 && tn == 1) CGL_WG(1, 1);
  else return CGL_E_ARG;
#undef CGL_WG
#undef CGL_WGK
  return (int)hipGetLastError();
}

// cgl_conv_wgrad_lds on wgl workgroups of 256 ks threads (the folded BatchNorm input: ks 1 only)
template <int DT>
int cgl_conv_wgrad_lds_launch(int wm, int ks, bool bnin, int wgl, hipStream_t s, const CglConvLaunch& L) {
  if ((wm != 1 && wm != 2) || (ks != 1 && ks != 2) || (bnin && ks != 1)) return CGL_E_ARG;
#define CGL_LDS(WM_, WN_, KS_, BNIN, THREADS) CGL_LAUNCH_WLDS(WM_, WN_, KS_, BNIN, DT, wgl, THREADS, s, L)
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

