// fp32 MFMA GEMM for the MLP GAN step (gfx950, v_mfma_f32_32x32x2_f32).
//
// Replaces the reference's implicit cuBLAS addmm / mm calls of nn.Linear forward and
// autograd backward (model/mnist_model.py:11,22,77,79,81); its epilogue also writes the
// per-tile statistics partials of the BatchNorm1d(train) that follows (model/mnist_model.py:13-14).
//
// Design (MI355X-first, not a CUDA tiling):
//  * one wave owns TM x TN 32x32 f32 MFMA accumulators (1x1 for small problems, 2x2 for the
//    large ones); v_mfma_f32_32x32x2_f32 issues every 64 cycles with a 64-cycle dependent
//    latency, so even a single accumulation chain runs at the f32 matrix peak;
//  * a 256-thread workgroup holds 4 waves arranged WM x WN x WK: WK > 1 splits K inside the
//    workgroup (skinny, batch-256 GEMMs need it to put >= 1024 waves on the 256 CUs) and the
//    split is summed through LDS in a fixed order (deterministic, no atomics);
//  * operands are loaded straight into the MFMA fragment registers.  The k index of the
//    32x32x2 fragment is permuted so that lane half h owns 8 CONSECUTIVE k of every 16-k
//    chunk: a k-contiguous operand is then two float4 loads per lane per 8 MFMAs;
//  * prologue fusion: the A operand rows can be gathered through an index list (the sampled
//    real batch) from two sources (real rows, then generated rows) and written out once
//    (the copy-out of each 16-k chunk is spread over the workgroups that load it);
//  * epilogue fusion: bias, LeakyReLU / Tanh, LeakyReLU' mask, Tanh' (1 - t^2), the
//    bias-gradient column (B's extra all-ones column), per-column {sum, M2} partials of the
//    stored output for the next layer's forward BatchNorm, and per-column {sum dy,
//    sum (y - mean) dy} partials of the stored gradient for its backward BatchNorm.
#include "cgl_internal.h"

#include <type_traits>

__device__ __forceinline__ const float* cgl_row(const CglRowSrc& s, int r) {
  if (r < s.split) {
    int rr = r;
    if (s.idx0) rr = gldi(s.idx0 + (s.idx_off ? gldi(s.idx_off) : 0) + r);
    return s.p0 + (long)rr * s.ld;
  }
  return s.p1 + (long)(r - s.split) * s.ld;
}

// Loads are issued UNCONDITIONALLY from clamped (always valid) addresses and masked only when
// the values are consumed: a predicated "load or zero" compiles to a branch around every load
// with a full vmcnt(0) drain, which serialises the memory pipeline (measured: one full memory
// latency per 16-k chunk).

// Operand pointers come out of the descriptor in memory, so the compiler cannot prove they are
// global and would emit flat_load_* -- which return out of order and force
// s_waitcnt vmcnt(0) lgkmcnt(0) at every use.  Casting to address space 1 gives global_load_*
// with counted waits.
// raw: 8 consecutive k of one row of a k-contiguous operand (k clamped into [0, K))
template <int VEC>
__device__ __forceinline__ void cgl_ld_kc(const float* __restrict__ rp_, int k, int K, float v[8]) {
  gcfp rp = (gcfp)rp_;
  if (VEC) {  // K % 4 == 0, 16-byte aligned rows
    const f32x4 x = *(gcf4p)(rp + min(k, K - 4));
    const f32x4 y = *(gcf4p)(rp + min(k + 4, K - 4));
    v[0] = x[0]; v[1] = x[1]; v[2] = x[2]; v[3] = x[3];
    v[4] = y[0]; v[5] = y[1]; v[6] = y[2]; v[7] = y[3];
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = rp[min(k + j, K - 1)];
  }
}

// raw: rows k..k+7 (clamped) at one column of a row-major [K][ld] (mn-contiguous) operand
__device__ __forceinline__ void cgl_ld_mn(const float* __restrict__ p_, int ld, int k, int K, float v[8]) {
  gcfp p = (gcfp)p_;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = p[(long)min(k + j, K - 1) * ld];
}

__device__ __forceinline__ void cgl_mask(float v[8], bool ok, int k, int K) {
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = (ok && k + j < K) ? v[j] : 0.f;
}

// Epilogue Adam of one accumulator block's 16 gradient values (rows rb + (r & 3) + 8 (r >> 2), column col
// of a row-major [M][ld] tensor): all parameter / moment loads issued first, then cgl_adam_update -- the
// arithmetic of cgl_adam on the same gradient values, so the result is bitwise cgl_adam's.
__device__ __forceinline__ void cgl_epi_adam(const CglGemmDesc* __restrict__ d, float* p_, float* m_, float* v_,
                                             int rb, int M, int col, int ld, const float* g) {
  const float ss = gld(d->ad_ss), bc = gld(d->ad_bc);
  float p[16], m[16], v[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const long e = (long)min(rb + (r & 3) + 8 * (r >> 2), M - 1) * ld + col;
    p[r] = gld(p_ + e);
    m[r] = gld(m_ + e);
    v[r] = gld(v_ + e);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = rb + (r & 3) + 8 * (r >> 2);
    cgl_adam_update(p[r], g[r], m[r], v[r], ss, bc, d->ad_b2, d->ad_w1, d->ad_w2, d->ad_eps);
    if (row < M) {
      const long e = (long)row * ld + col;
      gst(m_ + e, m[r]);
      gst(v_ + e, v[r]);
      gst(p_ + e, p[r]);
    }
  }
}

// ------------------------------------------------------------------------------------------
// Main body.  One wave owns TM x TN 32x32 accumulator blocks ((32 TM) x (32 TN) outputs); the
// workgroup tile is (32 TM WM) x (32 TN WN), K split WK ways.  Operand fragments of S chunks
// (16 k each) are in flight in a rotation of S register sets, so (S - 1) x TM TN x 512 MFMA
// cycles cover an L2 / MALL miss; TM = TN = 2 halves the operand traffic per FLOP and
// quadruples the MFMA work per load batch for the large problems.
template <int TM, int TN>
struct CglPipe {
#ifndef CGL_GEMM_STAGES
#define CGL_GEMM_STAGES 3
#endif
#ifndef CGL_GEMM_STAGES1
#define CGL_GEMM_STAGES1 CGL_GEMM_STAGES
#endif
  // 1x1-block waves (16 staging floats per chunk) can afford a deeper rotation than 2x2 ones
  static constexpr int S = (TM * TN == 1) ? CGL_GEMM_STAGES1 : CGL_GEMM_STAGES;
};

// Compile-time flags of a main-loop version: packed A, packed B (layout 0 only), A copy-out.
template <bool A_, bool B_, bool C_>
struct CglLoopFl {
  static constexpr bool PA = A_, PB = B_, CP = C_;
};

// Dynamic LDS: the split-K partials of the waves with wk > 0
template <int LAYOUT, int VEC, int TM, int TN, int DT = 0, bool ADAM = false>
__device__ __forceinline__ void cgl_gemm_body(const CglGemmDesc* __restrict__ d, int bid, float* __restrict__ s_dyn,
                                              double* __restrict__ s_bnd, unsigned long long t_entry = 0) {
  constexpr int S = CglPipe<TM, TN>::S;
  // The descriptor fields the set-up and the k-loop prologue need, read in ONE round of scalar loads before the
  // first branch and pinned there: left to the compiler, each load is issued in the block that uses it, after
  // that block's branch -- a chain of dependent scalar round trips (~0.16 us each, tools/launch_probe.hip) at
  // every launch start (tools/gemm_trace.py: ~1.7 us from kernel entry to the k-loop in the round 4 build).
  const int M = d->M, N = d->N, K = d->K;
  const int WN = d->WN, WK = d->WK, WM = d->WM;
  const int h_tm = d->tiles_m, h_tn = d->tiles_n, h_wg0 = d->wg_begin;
  const int h_gen = d->a_gen;
  const int h_ones = (LAYOUT != 0) ? d->b_ones_col : 0, h_apk = d->a_pk, h_bpk = d->b_pk;
  const float* const h_bias = d->bias;
  const float* const h_mref = d->mask_ref;
  const float* const h_tref = d->tanh_ref;
  const int h_mld = d->mask_ld, h_tld = d->tanh_ld, h_crow0 = d->a_copy_row0;
  float* const h_copy = d->a_copy;
  const CglRowSrc h_a = d->a, h_b = d->b;
  // the epilogue's fields too (they would otherwise cost one more scalar round trip after the k-loop)
  const int e_act = d->act, e_ldc = d->ldc, e_gr = d->stat_gr;
#ifndef CGL_GEMM_NO_CPERM
  const int e_cperm = d->c_perm;
#else
  const int e_cperm = 0;     // (A/B builds: the output-row permutation compiled out)
#endif
  const float e_slope = d->slope;
  float* const e_C = d->C;
  float* const e_bout = d->bias_out;
  float* const e_stat = d->stat_part;
  // every read above issued before anything uses one of them: ONE batch of scalar loads and one wait (left to
  // itself the scheduler started the tile arithmetic on the first batch and waited a second time)
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("" ::"s"(M), "s"(N), "s"(K), "s"(WN), "s"(WK), "s"(WM), "s"(h_tm), "s"(h_tn), "s"(h_wg0), "s"(h_gen),
               "s"(h_ones), "s"(h_apk), "s"(h_bpk));
  asm volatile("" ::"s"(e_act), "s"(e_ldc), "s"(e_gr), "s"(e_slope), "s"(e_C), "s"(e_bout), "s"(e_stat), "s"(e_cperm));
  asm volatile("" ::"s"(h_bias), "s"(h_mref), "s"(h_tref), "s"(h_mld), "s"(h_tld), "s"(h_crow0), "s"(h_copy),
               "s"(h_a.p0), "s"(h_a.p1), "s"(h_a.idx0), "s"(h_a.idx_off), "s"(h_a.split), "s"(h_a.ld), "s"(h_b.p0),
               "s"(h_b.p1), "s"(h_b.idx0), "s"(h_b.idx_off), "s"(h_b.split), "s"(h_b.ld));
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int li = lane & 31, lh = lane >> 5;
  const int wk = wave % WK, wmn = wave / WK;
  const int wm = wmn / WN, wn = wmn % WN;
  // XCD-aware tile order (blocks b and b+8 land on the same XCD): each XCD takes a contiguous
  // range of tiles in n-major order, so its L2 holds ~1/8 of the B panels (the weights) plus the
  // A panels, instead of all of both.  Bijective for any count (guide T1).
  const int local = bid - h_wg0;
  const int nwg = h_tm * h_tn;
  int tile = local;
  if (nwg >= 16) {
    const int xcd = local & 7, pos = local >> 3, q = nwg >> 3, r = nwg & 7;
    tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + pos;
  }
  const int tn = tile / h_tm, tm = tile % h_tm;
#ifdef CGL_GEMM_TRACE
  unsigned long long* trc = (d->trace && local < CGL_GEMM_TRACE_WGS) ? d->trace + (long)local * CGL_GEMM_TRACE_W : nullptr;
  if (trc && tid == 0) {
    trc[0] = t_entry;
    trc[1] = wall_clock64();
  }
#endif
  const int BM = 32 * TM * WM;
  const int m0 = tm * BM + wm * 32 * TM;            // first row of this wave's tile
  const int n0 = (tn * WN + wn) * 32 * TN;          // first column of this wave's tile

  // ---------------- generated A rows (the fused round prologue): this tile's rows of z, drawn here
  if (h_gen) {
    const int r0 = tm * BM, r1 = min(r0 + BM, M);
    const long q0 = ((long)r0 * K) >> 2, q1 = ((long)r1 * K + 3) >> 2;
    const uint32_t rnd = (uint32_t)(gldi(d->gen_round) + 1);
    for (long q = q0 + tid; q < q1; q += CGL_GEMM_THREADS)
      cgl_normal_at(q, const_cast<float*>(h_a.p0), d->gen_n, d->gen_seed, rnd, 0);
    __syncthreads();   // (workgroup release / acquire: the rows are read back below, by every wave)
  }

  // ---------------- epilogue operands, issued before the k-loop
  // The bias and the LeakyReLU' / Tanh' reference of the stored tile are loaded by the owner waves
  // ahead of the first chunk's operands: they return with that chunk (loads count in order) instead
  // of costing one more dependent memory round trip after the k-loop.  (A descriptor carries at most
  // one of mask_ref / tanh_ref.)  Clamped addresses, unconditional per lane.  CGL_GEMM_EPI_PF=0 keeps the
  // loads in the epilogue.
#ifndef CGL_GEMM_EPI_PF
#define CGL_GEMM_EPI_PF 1
#endif
  constexpr bool EPF = CGL_GEMM_EPI_PF && !ADAM && TM * TN == 1;   // (2x2 waves: no registers to spare)
  float pf_bias[TN], pf_ref[EPF ? TM : 1][EPF ? TN : 1][16];
  if constexpr (EPF) {
    if (wk == 0) {
      const float* ref = h_mref ? h_mref : h_tref;
      const long ldr = h_mref ? h_mld : h_tld;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int colc = min(n0 + 32 * j + li, N - 1);
        pf_bias[j] = h_bias ? gld(h_bias + colc) : 0.f;
        if (ref) {
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int row = min(m0 + 4 * lh + 32 * i + (r & 3) + 8 * (r >> 2), M - 1);
              pf_ref[i][j][r] = gld(ref + (long)row * ldr + colc);
            }
        }
      }
    }
  }

  // ---------------- main loop
  const int b_ones = h_ones;
  const int nmem = N - b_ones;     // columns of B actually in memory
  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
#ifndef CGL_GEMM_NACC
#define CGL_GEMM_NACC 2
#endif
  // 1x1 blocks: NACC independent accumulation chains over alternating k-steps of a chunk (summed in
  // a fixed order after the k-loop), so consecutive MFMAs do not wait on each other's result
  constexpr int NX = (TM * TN == 1 && DT == CGL_DTYPE_F32) ? CGL_GEMM_NACC : 1;
  f32x16 accx[NX > 1 ? NX - 1 : 1];
#pragma unroll
  for (int x = 0; x < (NX > 1 ? NX - 1 : 1); ++x)
#pragma unroll
    for (int r = 0; r < 16; ++r) accx[x][r] = 0.f;

#ifdef CGL_GEMM_TRACE
  if (trc && tid == 0) trc[2] = wall_clock64();
#endif
  {
  const int nch = (K + CGL_GEMM_KCHUNK - 1) / CGL_GEMM_KCHUNK;
  // chunk range of this wave: slice wk of WK equal slices of the K chunks
  const int cb = (wk * nch) / WK, ce = ((wk + 1) * nch) / WK;
  const int lda = h_a.ld, ldb = h_b.ld;
  float* __restrict__ a_copy = h_copy;
  // copy-out: chunk c of a row block is written by the one wave of the (tiles_n x WN) that load
  // it whose column index equals c modulo their count (the copy work spread over every workgroup)
  const int copy_n = h_tn * WN, copy_me = tn * WN + wn;

  // per-lane operand rows / columns of each block, clamped (always dereferenceable) bases
  const float* a_base[TM];
  const float* b_base[TN];
  bool b_is_ones[TN], copy_row[TM];
  const int kcn = (K + CGL_GEMM_KCHUNK - 1) / CGL_GEMM_KCHUNK;   // k chunks (packed block stride)
  const bool apk = LAYOUT == 0 && h_apk, bpk = LAYOUT == 0 && h_bpk;
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int am = m0 + 32 * i + li;      // A row (kc) or A column (mn)
    a_base[i] = (LAYOUT != 2) ? cgl_row(h_a, min(am, M - 1)) : h_a.p0 + min(am, M - 1);
    // packed A: the lane's float4 of chunk 0 of its (clamped) 32-row block
    if (apk) a_base[i] = h_a.p0 + (long)(min(m0 + 32 * i, (M - 1) & ~31) >> 5) * kcn * 512 + lane * 4;
    copy_row[i] = (LAYOUT != 2) && a_copy && am < M && am >= h_crow0;
  }
  // A copy-out in the main loop (full chunks, 16-byte form) as buffer stores whose offset is pushed out of range
  // for the lanes / chunks that do not write: no branch in the loop body, so every s_waitcnt there still counts
  // exactly the loads of the set it consumes (a conditional store made the compiler drain vmcnt(0) at the top of
  // every rotation).  The range check drops the out-of-range stores.
  const auto rc_copy = __builtin_amdgcn_make_buffer_rsrc(a_copy ? a_copy : const_cast<float*>(h_a.p0), (short)0,
                                                         0x7fffffff, 0x00020000);
  unsigned copy_off[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i)
    copy_off[i] = copy_row[i] ? (unsigned)((m0 + 32 * i + li) * d->a_copy_ld) * 4u : 0x7fffffffu;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int bc = n0 + 32 * j + li;      // B row (NT) or B column (NN/TN)
    b_is_ones[j] = b_ones && (bc == N - 1);
    b_base[j] = (LAYOUT == 0) ? cgl_row(h_b, min(bc, N - 1)) : h_b.p0 + max(0, min(bc, nmem - 1));
    if (bpk) b_base[j] = h_b.p0 + (long)(min(n0 + 32 * j, (N - 1) & ~31) >> 5) * kcn * 512 + lane * 4;
  }

  // Full chunks (k + 16 <= K) load without clamps and multiply without masks: rows / columns
  // past M / N come from clamped (valid) addresses and only feed accumulator rows / columns
  // that are never stored.  Only the K-tail chunk clamps its k and zeroes k >= K.
  auto load_a = [&](auto tail, int c, const float* const (&base)[TM], int ld, float (&A_)[TM][8], auto pkc) {
    constexpr bool T = decltype(tail)::value;
    constexpr bool pk = decltype(pkc)::value;
    const int k = c * CGL_GEMM_KCHUNK + 8 * lh;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      if constexpr (LAYOUT == 0 && pk) {          // packed: two contiguous 1 KB wave loads (padding past K)
        const f32x4 x = *(gcf4p)(base[i] + c * 512), y = *(gcf4p)(base[i] + c * 512 + 256);
        A_[i][0] = x[0]; A_[i][1] = x[1]; A_[i][2] = x[2]; A_[i][3] = x[3];
        A_[i][4] = y[0]; A_[i][5] = y[1]; A_[i][6] = y[2]; A_[i][7] = y[3];
      } else if (LAYOUT == 2) {
        if (T) {
          cgl_ld_mn(base[i], ld, k, K, A_[i]);
        } else {
          gcfp q = (gcfp)base[i] + (long)k * ld;
#pragma unroll
          for (int j = 0; j < 8; ++j) A_[i][j] = q[(long)j * ld];
        }
      } else {
        if (T) {
          cgl_ld_kc<VEC>(base[i], k, K, A_[i]);
        } else if (VEC) {
          const f32x4 x = *(gcf4p)(base[i] + k), y = *(gcf4p)(base[i] + k + 4);
          A_[i][0] = x[0]; A_[i][1] = x[1]; A_[i][2] = x[2]; A_[i][3] = x[3];
          A_[i][4] = y[0]; A_[i][5] = y[1]; A_[i][6] = y[2]; A_[i][7] = y[3];
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) A_[i][j] = ((gcfp)base[i])[k + j];
        }
      }
    }
  };
  // fl: the loop version's compile-time flags (LoopFl: packed A, packed B, copy-out) -- see run_loop below
  auto load_chunk = [&](auto tail, int c, float (&A_)[TM][8], float (&B_)[TN][8], auto fl) {
    constexpr bool T = decltype(tail)::value;
    const int k = c * CGL_GEMM_KCHUNK + 8 * lh;
    load_a(tail, c, a_base, lda, A_, std::integral_constant<bool, decltype(fl)::PA>());
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      if constexpr (LAYOUT == 0 && decltype(fl)::PB) {
        const f32x4 x = *(gcf4p)(b_base[j] + c * 512), y = *(gcf4p)(b_base[j] + c * 512 + 256);
        B_[j][0] = x[0]; B_[j][1] = x[1]; B_[j][2] = x[2]; B_[j][3] = x[3];
        B_[j][4] = y[0]; B_[j][5] = y[1]; B_[j][6] = y[2]; B_[j][7] = y[3];
      } else if (LAYOUT == 0) {
        if (T) {
          cgl_ld_kc<VEC>(b_base[j], k, K, B_[j]);
        } else if (VEC) {
          const f32x4 x = *(gcf4p)(b_base[j] + k), y = *(gcf4p)(b_base[j] + k + 4);
          B_[j][0] = x[0]; B_[j][1] = x[1]; B_[j][2] = x[2]; B_[j][3] = x[3];
          B_[j][4] = y[0]; B_[j][5] = y[1]; B_[j][6] = y[2]; B_[j][7] = y[3];
        } else {
#pragma unroll
          for (int q = 0; q < 8; ++q) B_[j][q] = ((gcfp)b_base[j])[k + q];
        }
      } else {
        if (T) {
          cgl_ld_mn(b_base[j], ldb, k, K, B_[j]);
        } else {
          gcfp q = (gcfp)b_base[j] + (long)k * ldb;
#pragma unroll
          for (int u = 0; u < 8; ++u) B_[j][u] = q[(long)u * ldb];
        }
      }
    }
  };
  auto compute_chunk = [&](auto tail, int c, float (&A_)[TM][8], float (&B_)[TN][8], auto fl) {
    constexpr bool T = decltype(tail)::value;
    const int k = c * CGL_GEMM_KCHUNK + 8 * lh;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      if (T) cgl_mask(A_[i], true, k, K);
      if constexpr (!decltype(fl)::CP) continue;
      if (VEC && !T) {
        const unsigned off = (c % copy_n) == copy_me ? copy_off[i] + 4u * k : 0x7fffffffu;
        __builtin_amdgcn_raw_buffer_store_b128(f32x4{A_[i][0], A_[i][1], A_[i][2], A_[i][3]}, rc_copy, off, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b128(f32x4{A_[i][4], A_[i][5], A_[i][6], A_[i][7]}, rc_copy, off + 16u, 0, 0);
      } else if (copy_row[i] && (c % copy_n) == copy_me) {
        float* dst = a_copy + (long)(m0 + 32 * i + li) * d->a_copy_ld;
        if (VEC && (!T || k + 7 < K)) {
          *(gf4p)(dst + k) = f32x4{A_[i][0], A_[i][1], A_[i][2], A_[i][3]};
          *(gf4p)(dst + k + 4) = f32x4{A_[i][4], A_[i][5], A_[i][6], A_[i][7]};
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (!T || k + j < K) gst(dst + k + j, A_[i][j]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      if (T) cgl_mask(B_[j], true, k, K);
      if (b_ones) {
#pragma unroll
        for (int q = 0; q < 8; ++q)
          if (b_is_ones[j]) B_[j][q] = (!T || k + q < K) ? 1.f : 0.f;
      }
    }
    if constexpr (DT != CGL_DTYPE_F32) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) cgl_mfma16<DT>(acc[i][j], A_[i], B_[j]);
    } else if constexpr (NX > 1) {
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        if (q % NX == 0)
          acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(A_[0][q], B_[0][q], acc[0][0], 0, 0, 0);
        else
          accx[q % NX - 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(A_[0][q], B_[0][q], accx[q % NX - 1], 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int q = 0; q < 8; ++q)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(A_[i][q], B_[j][q], acc[i][j], 0, 0, 0);
    }
  };

  // S register sets in rotation: set s holds chunk c + s; after its MFMAs are issued it is
  // refilled with chunk c + s + S, so S - 1 chunks of loads are always in flight.  The bulk
  // loop body must be branch-free (refills past the end re-load the last full chunk, harmlessly), so
  // that every s_waitcnt waits for exactly the set it consumes: the operand forms (packed A / B) and the
  // A copy-out are therefore compile-time flags of a loop VERSION (run_loop, dispatched once below).  With them
  // as run-time branches inside the loop (rounds 1-4) the compiler could not count the loads across the
  // branch merges and drained every load at the top of each rotation (s_waitcnt vmcnt(0)): one chunk in three
  // waited for all loads in flight (tools/gemm_trace.py per-chunk stamps: 0.32 / 0.32 / 0.52 us).
  const int cfull = min(ce, K / CGL_GEMM_KCHUNK);   // end of this wave's full chunks
  std::integral_constant<bool, false> full;
  std::integral_constant<bool, true> tailc;
  auto run_loop = [&](auto fl) {
    if (cb < cfull) {
      float xa[S][TM][8], xb[S][TN][8];
#pragma unroll
      for (int s = 0; s < S; ++s) load_chunk(full, min(cb + s, cfull - 1), xa[s], xb[s], fl);
      int c = cb;
      for (; c + S <= cfull; c += S) {
#pragma unroll
        for (int s = 0; s < S; ++s) {
          compute_chunk(full, c + s, xa[s], xb[s], fl);
#ifdef CGL_GEMM_TRACE
          if (trc && tid == 0 && c == cb && s == 0) trc[3] = wall_clock64();   // chunk 0's operands arrived
#ifdef CGL_GEMM_TRACE_CHUNKS
          if (trc && tid == 0 && c + s - cb < CGL_GEMM_TRACE_W - 8) trc[8 + c + s - cb] = wall_clock64();
#endif
#endif
          // the refill stays right behind the chunk it replaces: without the fences the scheduler sinks all S
          // refills to the end of the rotation, where the next rotation's first chunk waits on them at once
          __builtin_amdgcn_sched_barrier(0);
          load_chunk(full, min(c + s + S, cfull - 1), xa[s], xb[s], fl);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
#pragma unroll
      for (int s = 0; s < S - 1; ++s)
        if (c + s < cfull) compute_chunk(full, c + s, xa[s], xb[s], fl);
    }
    if (cfull < ce) {   // the K tail (at most one chunk, owned by the last k-group)
      float xa[TM][8], xb[TN][8];
      load_chunk(tailc, cfull, xa, xb, fl);
      compute_chunk(tailc, cfull, xa, xb, fl);
    }
  };
  const bool cp = LAYOUT != 2 && a_copy != nullptr;
  if constexpr (LAYOUT == 0) {
    if (apk && bpk)
      cp ? run_loop(CglLoopFl<true, true, true>()) : run_loop(CglLoopFl<true, true, false>());
    else if (apk)
      cp ? run_loop(CglLoopFl<true, false, true>()) : run_loop(CglLoopFl<true, false, false>());
    else if (bpk)
      cp ? run_loop(CglLoopFl<false, true, true>()) : run_loop(CglLoopFl<false, true, false>());
    else
      cp ? run_loop(CglLoopFl<false, false, true>()) : run_loop(CglLoopFl<false, false, false>());
  } else {
    cp ? run_loop(CglLoopFl<false, false, true>()) : run_loop(CglLoopFl<false, false, false>());
  }
  }   // (register-pipelined main loop)

  if constexpr (NX > 1) {
#pragma unroll
    for (int x = 0; x < NX - 1; ++x)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[0][0][r] += accx[x][r];
  }

  // ---------------- split-K reduction (fixed order: wk = 1, 2, 3)
  if (WK > 1) {
    constexpr int NB = TM * TN;
    if (wk > 0) {
      float* dst = s_dyn + ((wmn * (WK - 1) + (wk - 1)) * NB * 16) * 64;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) dst[((i * TN + j) * 16 + r) * 64 + lane] = acc[i][j][r];
    }
    __syncthreads();
    if (wk == 0) {
      for (int q = 1; q < WK; ++q) {
        const float* src = s_dyn + ((wmn * (WK - 1) + (q - 1)) * NB * 16) * 64;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] += src[((i * TN + j) * 16 + r) * 64 + lane];
      }
    }
  }

#ifdef CGL_GEMM_TRACE
  if (trc && tid == 0) trc[4] = wall_clock64();
#endif
  // ---------------- epilogue (waves with wk == 0 own the tile)
  // register r of block (i, j): row m0 + 32 i + 4 lh + (r & 3) + 8 (r >> 2), column n0 + 32 j + li
  const bool owner = (wk == 0);
  const int rbase = m0 + 4 * lh;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = n0 + 32 * j + li;
    const bool colok = col < N;
    const bool ones_col = b_ones && col == N - 1;
    if (owner && colok && !ones_col) {
      float bb;
      if constexpr (EPF) bb = pf_bias[j];
      else bb = h_bias ? gld(h_bias + col) : 0.f;
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        float* v = (float*)&acc[i][j];
        if (h_bias) {
#pragma unroll
          for (int r = 0; r < 16; ++r) v[r] += bb;
        }
        if (e_act == CGL_EPI_ACT_LEAKY) {
          const float sl = e_slope;
#pragma unroll
          for (int r = 0; r < 16; ++r) v[r] = v[r] > 0.f ? v[r] : v[r] * sl;
        } else if (e_act == CGL_EPI_ACT_TANH) {
#pragma unroll
          for (int r = 0; r < 16; ++r) v[r] = tanhf(v[r]);   // (double tanh here costs ~4 us on G L4)
        } else if (e_act == CGL_EPI_ACT_SIGMOID) {
#pragma unroll
          for (int r = 0; r < 16; ++r) v[r] = 1.f / (1.f + expf(-v[r]));
        }
        if (h_mref) {
          const float sl = e_slope;
          float ref[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            if constexpr (EPF) {
              ref[r] = pf_ref[i][j][r];
            } else {
              const int row = min(rbase + 32 * i + (r & 3) + 8 * (r >> 2), M - 1);
              ref[r] = gld(h_mref + (long)row * h_mld + col);
            }
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) v[r] = ref[r] > 0.f ? v[r] : v[r] * sl;
        }
        if (h_tref) {
          float t[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            if constexpr (EPF) {
              t[r] = pf_ref[i][j][r];
            } else {
              const int row = min(rbase + 32 * i + (r & 3) + 8 * (r >> 2), M - 1);
              t[r] = gld(h_tref + (long)row * h_tld + col);
            }
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) v[r] = cgl_dtanh(v[r], t[r]);
        }
      }
    }
  }

  // the tile's stores first: they drain while the BatchNorm partials below are reduced (the partials only
  // read the accumulators)
  // (stored row of result row r: ((r & pmask) << pq) + (r >> pl); the identity without a permutation)
  const int pl = e_cperm ? (e_cperm & 255) : 31, pq = e_cperm ? (e_cperm >> 8) : 0;
  const int pmask = e_cperm ? (1 << pl) - 1 : 0x7fffffff;
  if (owner) {
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int col = n0 + 32 * j + li;
      if (col >= N) continue;
      const bool ones_col = b_ones && col == N - 1;
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const float* v = (const float*)&acc[i][j];
        if (ones_col) {
          if (e_bout) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int row = rbase + 32 * i + (r & 3) + 8 * (r >> 2);
              if (row < M) gst(e_bout + (((row & pmask) << pq) + (row >> pl)), v[r]);
            }
            if constexpr (ADAM) cgl_epi_adam(d, d->ad_pb, d->ad_mb, d->ad_vb, rbase + 32 * i, M, 0, 1, v);
          }
        } else {
          float* __restrict__ C = e_C;
          const int ldc = e_ldc;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row0 = rbase + 32 * i + (r & 3) + 8 * (r >> 2);
            const bool rok = row0 < M;
            const int row = ((row0 & pmask) << pq) + (row0 >> pl);
#ifndef CGL_C_STORE_WB
            // write-through (agent-scope) output stores: no dirty C lines are left in the XCD's L2 for the
            // end-of-kernel write-back, and the next launch (on any XCD) reads them from MALL either way.
            // Measured -1.0 us per B = 256 round, interleaved x3 twice (profiles/r04_store_wt_ab.txt); making
            // every plain store write-through (CGL_GST_WT) gave nothing.  -DCGL_C_STORE_WB: plain stores.
            if (rok)
              __hip_atomic_store((CGL_GLOBAL float*)(C + (long)row * ldc + col), v[r], __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
#else
            if (rok) gst(C + (long)row * ldc + col, v[r]);
#endif
          }
          if constexpr (ADAM) cgl_epi_adam(d, d->ad_p, d->ad_m, d->ad_v, rbase + 32 * i, M, col, ldc, v);
        }
      }
    }
  }

  // forward BatchNorm partials of the stored output: per column, per group slot {sum, M2 about the
  // tile-slot mean} over the workgroup's BM rows.  Each lane reduces its own rows two-pass (count, sum,
  // M2 about its own mean), the two lane halves and then the WM waves of the column are merged by
  // Chan's pairwise update in a fixed order: one workgroup barrier per slot, and a slot holding none
  // of the tile's rows (a tile spans <= 2 forward calls; usually one) costs nothing.
  if (e_stat) {
    const int gr = e_gr;
    const int trow0 = tm * BM;
    const int gfirst = trow0 / gr;
    const int gsplit = (gfirst + 1) * gr;   // first row of slot 1
    float* s_st = (float*)s_bnd;            // [WM WN TN 32][3] {n, sum, M2}
    for (int s = 0; s < 2; ++s) {
      const int ra = max(trow0, (gfirst + s) * gr), rb = min(min(trow0 + BM, M), (gfirst + s + 1) * gr);
      if (rb - ra <= 0) {                   // workgroup-uniform
        if (owner && wm == 0 && lh == 0)
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            const int col = n0 + 32 * j + li;
            if (col < N) {
              float* p = e_stat + ((long)(tm * 2 + s) * N + col) * 2;
              gst(p, 0.f);
              gst(p + 1, 0.f);
            }
          }
        continue;
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const bool colok = n0 + 32 * j + li < N;
        float cn = 0.f, sum = 0.f, m2 = 0.f;
        if (owner && colok) {
#pragma unroll
          for (int i = 0; i < TM; ++i) {
            const float* v = (const float*)&acc[i][j];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int row = rbase + 32 * i + (r & 3) + 8 * (r >> 2);
              const bool in = row < M && (row >= gsplit) == (s == 1);
              sum += in ? v[r] : 0.f;
              cn += in ? 1.f : 0.f;
            }
          }
          const float mu = cn > 0.f ? sum / cn : 0.f;
#pragma unroll
          for (int i = 0; i < TM; ++i) {
            const float* v = (const float*)&acc[i][j];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int row = rbase + 32 * i + (r & 3) + 8 * (r >> 2);
              const bool in = row < M && (row >= gsplit) == (s == 1);
              const float dd = v[r] - mu;
              m2 += in ? dd * dd : 0.f;
            }
          }
        }
        {   // lane half 0 (a) with lane half 1 (b)
          const float cb = __shfl_xor(cn, 32), sb = __shfl_xor(sum, 32), mb = __shfl_xor(m2, 32);
          const float ca = lh ? cb : cn, sa = lh ? sb : sum, ma = lh ? mb : m2;
          const float c2 = lh ? cn : cb, s2 = lh ? sum : sb, m22 = lh ? m2 : mb;
          const float nt = ca + c2;
          const float dl = (ca > 0.f && c2 > 0.f) ? s2 / c2 - sa / ca : 0.f;
          cn = nt;
          sum = sa + s2;
          m2 = ma + m22 + (nt > 0.f ? dl * dl * (ca * c2 / nt) : 0.f);
        }
        if (WM == 1) {         // one wave row per column tile: its merge is the tile's (no LDS, no barrier;
          const int col = n0 + 32 * j + li;   // the same values the one-entry merge below would store)
          if (owner && lh == 0 && col < N) {
            float* p = e_stat + ((long)(tm * 2 + s) * N + col) * 2;
            gst(p, 0.f + sum);
            gst(p + 1, 0.f + m2);
          }
        } else if (owner && lh == 0) {
          float* e = s_st + (((wm * WN + wn) * TN + j) * 32 + li) * 3;
          e[0] = cn;
          e[1] = sum;
          e[2] = m2;
        }
      }
      if (WM == 1) continue;
      __syncthreads();
      if (owner && wm == 0 && lh == 0) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int col = n0 + 32 * j + li;
          float cn = 0.f, sum = 0.f, m2 = 0.f;
          for (int q = 0; q < WM; ++q) {
            const float* e = s_st + (((q * WN + wn) * TN + j) * 32 + li) * 3;
            const float c2 = e[0], s2 = e[1];
            const float nt = cn + c2;
            const float dl = (cn > 0.f && c2 > 0.f) ? s2 / c2 - sum / cn : 0.f;
            m2 += e[2] + (nt > 0.f ? dl * dl * (cn * c2 / nt) : 0.f);
            sum += s2;
            cn = nt;
          }
          if (col < N) {
            float* p = e_stat + ((long)(tm * 2 + s) * N + col) * 2;
            gst(p, sum);
            gst(p + 1, m2);
          }
        }
      }
      __syncthreads();
    }
  }

  // dynamic loss scaling (16-bit operand instantiations only): a non-finite stored weight gradient
  // raises the model's found flag (GradScaler's found_inf), read by that model's Adam launch
  if constexpr (DT != CGL_DTYPE_F32) {
    if (owner && d->inf_flag) {
      bool bad = false;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const bool colok = n0 + 32 * j + li < N;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const float* v = (const float*)&acc[i][j];
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = rbase + 32 * i + (r & 3) + 8 * (r >> 2);
            bad |= colok && row < M && !isfinite(v[r]);
          }
        }
      }
      if (bad) atomicOr(d->inf_flag, 1u);
    }
  }
#ifdef CGL_GEMM_TRACE
  if (trc) {
    __syncthreads();
    if (tid == 0) trc[5] = wall_clock64();
  }
#endif
}

// One kernel per per-wave block shape (TM x TN), shared by every GEMM of the step; a grouped
// launch may mix layouts (e.g. the weight gradient (TN) and the input gradient (NN) of one
// layer side by side).  Separate symbols keep the 1x1 variant's register budget (and so its
// occupancy) independent of the 2x2 variant's.
// Dynamic LDS: the split-K partials of the waves with wk > 0.
// sel (kernel arguments): the launch's problem selection -- first workgroup of problems 1 and 2 (INT_MAX: absent), each
// problem's layout | vec << 2 in 4 bits, and whether d[0] carries a deferred head reduction -- so that a workgroup finds
// its problem and body without reading the descriptor array first.
template <int TM, int TN, int DT = CGL_DTYPE_F32>
__global__ __launch_bounds__(CGL_GEMM_THREADS) void cgl_gemm_f32(const CglGemmDesc* __restrict__ descs, int sel_wg1,
                                                                 int sel_wg2, int sel_meta, int sel_fin,
                                                                 const int* __restrict__ pf, int pf_lines) {
  // (the selection as scalar kernel arguments: with kernarg preloading they arrive in SGPRs at wave start)
  const CglGemmSel sel{sel_wg1, sel_wg2, sel_meta, sel_fin};
#ifdef CGL_GEMM_TRACE
  const unsigned long long t_entry = wall_clock64();
#else
  const unsigned long long t_entry = 0;
#endif
  extern __shared__ float cgl_dyn_lds[];
  __shared__ double s_bnd[4 * TN * 32 * 2];     // per-column BatchNorm partials across waves (WM WN <= 4)
  const int bid = blockIdx.x;
  // the previous head launch's deferred batch-mean loss reduction rides in one extra workgroup (the last)
  if (sel.fin && bid == (int)gridDim.x - 1) {
    cgl_head_finish(descs[0].fin_head, descs[0].fin_head->nwg, cgl_dyn_lds);
    return;
  }
  // L2 warm-up of the next GEMM launch's descriptors: they are read once per round, through the scalar cache,
  // at the head of that launch's dependent chain (descriptor -> operand addresses -> operands); after a round's
  // streaming they have left L2.  Workgroups 0..7 land on XCDs 0..7 (round-robin dispatch), one line per lane;
  // the value is held to the end of the kernel, so the load is issued here and never waited on early.
  int pfv = 0;
  if (bid < 8 && (int)threadIdx.x < pf_lines) pfv = pf[threadIdx.x * 32];
  const int di = bid >= sel.wg2 ? 2 : (bid >= sel.wg1 ? 1 : 0);
  const CglGemmDesc* __restrict__ d = descs + di;
  const int meta = (sel.meta >> (4 * di)) & 15;
  const int layout = meta & 3;
  // VEC: every operand allows 16-byte loads along its contiguous dimension
  const int vec = (meta >> 2) & 1;
#define CGL_BODY(L)                                               \
  do {                                                            \
    if (vec)                                                      \
      cgl_gemm_body<L, 1, TM, TN, DT>(d, bid, cgl_dyn_lds, s_bnd, t_entry);    \
    else                                                          \
      cgl_gemm_body<L, 0, TM, TN, DT>(d, bid, cgl_dyn_lds, s_bnd, t_entry);    \
  } while (0)
  if (layout == 0)
    CGL_BODY(0);
  else if (layout == 1)
    CGL_BODY(1);
  else
    CGL_BODY(2);
#undef CGL_BODY
  asm volatile("" ::"v"(pfv));
}

// The same problems for W co-located workers in one launch: descs = [W][q] (q <= 3 problems per worker, the W
// copies of a problem identical in shape, layout and tiles, different in their pointers), every worker owning wpw
// consecutive workgroups.  A workgroup finds its worker by one division and its problem among the worker's q by
// the scalar selection (first workgroup of problems 1 and 2 within a worker, layout | vec << 2 per problem), then
// runs the body of cgl_gemm_f32 on that descriptor -- whose wg_begin counts from the start of the launch -- so
// each worker's result is bitwise what its own launch of the q problems computes.
template <int TM, int TN, int DT = CGL_DTYPE_F32>
__global__ __launch_bounds__(CGL_GEMM_THREADS) void cgl_gemm_grp(const CglGemmDesc* __restrict__ descs, int wpw, int q,
                                                                 int sel_wg1, int sel_wg2, int sel_meta,
                                                                 const int* __restrict__ pf, int pf_lines) {
  extern __shared__ float cgl_dyn_lds[];
  __shared__ double s_bnd[4 * TN * 32 * 2];
  const int bid = blockIdx.x;
  int pfv = 0;     // the next GEMM launch's descriptors into every XCD's L2 (as cgl_gemm_f32)
  if (bid < 8 && (int)threadIdx.x < pf_lines) pfv = pf[threadIdx.x * 32];
  const int w = bid / wpw, lb = bid - w * wpw;
  const int di = lb >= sel_wg2 ? 2 : (lb >= sel_wg1 ? 1 : 0);
  const CglGemmDesc* __restrict__ d = descs + w * q + di;
  const int meta = (sel_meta >> (4 * di)) & 15;
  const int layout = meta & 3;
  const int vec = (meta >> 2) & 1;
#define CGL_BODY_GRP(L)                                        \
  do {                                                         \
    if (vec)                                                   \
      cgl_gemm_body<L, 1, TM, TN, DT>(d, bid, cgl_dyn_lds, s_bnd);  \
    else                                                       \
      cgl_gemm_body<L, 0, TM, TN, DT>(d, bid, cgl_dyn_lds, s_bnd);  \
  } while (0)
  if (layout == 0)
    CGL_BODY_GRP(0);
  else if (layout == 1)
    CGL_BODY_GRP(1);
  else
    CGL_BODY_GRP(2);
#undef CGL_BODY_GRP
  asm volatile("" ::"v"(pfv));
}

// One problem whose descriptor travels in the kernel arguments (the single-op entry points cgl_linear_*):
// nothing is uploaded before the launch, so the ops need no host synchronisation and can be captured into
// a graph.  fp32, no deferred head.
template <int TM, int TN>
__global__ __launch_bounds__(CGL_GEMM_THREADS) void cgl_gemm_f32_arg(const CglGemmDesc desc) {
  extern __shared__ float cgl_dyn_lds[];
  __shared__ double s_bnd[4 * TN * 32 * 2];
  const CglGemmDesc* __restrict__ d = &desc;
  const int bid = blockIdx.x;
  const int vec = d->a_vec && d->b_vec;
#define CGL_BODY_ARG(L)                                                                             \
  do {                                                                                              \
    if (vec)                                                                                        \
      cgl_gemm_body<L, 1, TM, TN>(d, bid, cgl_dyn_lds, s_bnd);     \
    else                                                                                            \
      cgl_gemm_body<L, 0, TM, TN>(d, bid, cgl_dyn_lds, s_bnd);     \
  } while (0)
  if (d->layout == 0)
    CGL_BODY_ARG(0);
  else if (d->layout == 1)
    CGL_BODY_ARG(1);
  else
    CGL_BODY_ARG(2);
#undef CGL_BODY_ARG
}

// Host helpers: a problem's dynamic LDS bytes (the split-K partials) and its workgroups.
inline int cgl_gemm_stage_bytes(const CglGemmDesc& d) {
  return (d.WK > 1) ? d.WM * d.WN * (d.WK - 1) * d.TM * d.TN * 16 * 64 * 4 : 0;
}
inline int cgl_gemm_wgs(const CglGemmDesc& d) { return d.tiles_m * d.tiles_n; }
