// BatchNorm2d and the elementwise passes of the conv path, device side: the channel reductions, the finalize
// kernels (whole and sliced), the apply / activation-backward kernels, and the small host helpers that launch them
// (chunk size, column sums, record + launch).  Included by cgl_conv.hip ahead of its deferred-reduction kernel,
// which finishes column sums with cgl_bn_finalize_at; the C entry points are in cgl_conv_bn.hip.
#pragma once
#include "cgl_conv_mma.h"

// ------------------------------------------------------------------------------------------
// Per-channel reductions over an NHWC tensor [rows][C] (C a power of two <= 256), one chunk of R
// rows per workgroup, double accumulation, fixed order:
//   mode 0  {sum x, M2 about the chunk mean}                            (BatchNorm2d statistics)
//   mode 1  {sum g, sum g (x - mean_group)},  g = dY * leaky'(post)      (BatchNorm2d backward)
//   mode 2  {sum x, 0}                                                  (bias gradient)
struct CglChanArgs {
  const float* X; int rows, C, R, mode, hw, gr;
  const float* dY; const float* post; float slope;
  const float* mean;         // [groups][C] (mode 1)
  double* part;              // [nchunks][C][2]
  const int* nv;             // mode 0: only rows < *nv * hw of the first group (rows < gr) count, or null
  // mode 1 without the post-activation tensor: LeakyReLU'(post) from the sign of the forward's own
  // fmaf(x, scale, shift) (scale = psc[c], shift = psc[psc_ld + c]) -- post > 0 exactly when that value is
  // (slope > 0), so the gradient is bitwise the one read from post, and post's bytes are not read
  const float* psc; int psc_ld;
};

// rows of the first BatchNorm group that carry data: a short real call (DataLoader's short final batch)
// holds *nv real images, the rest of its gr rows are padding; null = the whole group
__device__ __forceinline__ int cgl_nv_rows(const int* nv, int hw, int gr) {
  return nv ? min(gldi(nv) * hw, gr) : gr;
}

__global__ __launch_bounds__(256) void cgl_chan_reduce(CglChanArgs a) {
  __shared__ double s0[256], s1[256];
  const int C = a.C, rp = 256 / C;
  const int c = threadIdx.x % C, rl = threadIdx.x / C;
  const int r0 = blockIdx.x * a.R;
  int r1 = min(r0 + a.R, a.rows);
  if (a.mode == 0 && a.nv && r0 < a.gr) r1 = max(r0, min(r1, cgl_nv_rows(a.nv, a.hw, a.gr)));
  double x0 = 0.0, x1 = 0.0;
  // rows r0 + rl + rp * i, issued 8 at a time (independent loads in flight), summed in order
  if (a.mode == 1) {
    const float mu = gld(a.mean + (long)(r0 / a.gr) * C + c);
    for (int rb = r0 + rl; rb < r1; rb += 8 * rp) {
      float g[8], xv[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int r = min(rb + i * rp, r1 - 1);
        const long o = (long)r * C + c;
        g[i] = gld(a.dY + o);
        xv[i] = gld(a.X + o);   // (before the sign below reads it, as in cgl_chan_reduce4)
        if (a.psc) g[i] = fmaf(xv[i], a.psc[c], a.psc[a.psc_ld + c]) > 0.f ? g[i] : g[i] * a.slope;
        else if (a.post) g[i] = gld(a.post + o) > 0.f ? g[i] : g[i] * a.slope;
      }
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (rb + i * rp < r1) {
          x0 += (double)g[i];
          x1 += (double)(g[i] * (xv[i] - mu));
        }
    }
  } else {
    for (int rb = r0 + rl; rb < r1; rb += 8 * rp) {
      float xv[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) xv[i] = gld(a.X + (long)min(rb + i * rp, r1 - 1) * C + c);
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (rb + i * rp < r1) x0 += (double)xv[i];
    }
  }
  s0[threadIdx.x] = x0;
  s1[threadIdx.x] = x1;
  __syncthreads();
  if (a.mode == 0) {
    if (rl == 0) {
      double t = 0.0;
      for (int q = 0; q < rp; ++q) t += s0[q * C + c];
      s0[c] = t;
    }
    __syncthreads();
    const double mean = s0[c] / max(r1 - r0, 1);
    double m2 = 0.0;
    for (int rb = r0 + rl; rb < r1; rb += 8 * rp) {
      float xv[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) xv[i] = gld(a.X + (long)min(rb + i * rp, r1 - 1) * C + c);
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (rb + i * rp < r1) {
          const double d = (double)xv[i] - mean;
          m2 += d * d;
        }
    }
    __syncthreads();
    s1[threadIdx.x] = m2;
    __syncthreads();
    if (rl == 0) {
      double t = 0.0;
      for (int q = 0; q < rp; ++q) t += s1[q * C + c];
      a.part[((long)blockIdx.x * C + c) * 2] = s0[c];
      a.part[((long)blockIdx.x * C + c) * 2 + 1] = t;
    }
    return;
  }
  if (rl == 0) {
    double t0 = 0.0, t1 = 0.0;
    for (int q = 0; q < rp; ++q) {
      t0 += s0[q * C + c];
      t1 += s1[q * C + c];
    }
    a.part[((long)blockIdx.x * C + c) * 2] = t0;
    a.part[((long)blockIdx.x * C + c) * 2 + 1] = t1;
  }
}

// 16-byte variant of cgl_chan_reduce for C % 4 == 0 (every BatchNorm2d of model/lsgan.py): a lane owns
// a float4 of channels, so each row of a wave's load is one 16-byte access per lane (4x fewer vector
// memory instructions than the per-channel lanes above) and 8 rows x 16 B are in flight per lane.
// Same outputs (double partials per chunk and channel; rows summed per lane in row order, lanes in
// a fixed order).
__global__ __launch_bounds__(256) void cgl_chan_reduce4(CglChanArgs a) {
  __shared__ double s0[1024], s1[1024], tot[256];
  const int C = a.C, CW = C >> 2, rp = 256 / CW;
  const int cs = threadIdx.x % CW, rl = threadIdx.x / CW, c = 4 * cs;
  const int r0 = blockIdx.x * a.R;
  int r1 = min(r0 + a.R, a.rows);
  if (a.mode == 0 && a.nv && r0 < a.gr) r1 = max(r0, min(r1, cgl_nv_rows(a.nv, a.hw, a.gr)));
  double x0[4] = {0.0, 0.0, 0.0, 0.0}, x1[4] = {0.0, 0.0, 0.0, 0.0};
  if (a.mode == 1) {
    const f32x4 mu = *(gcf4p)(a.mean + (long)(r0 / a.gr) * C + c);
    const f32x4 ps = a.psc ? *(gcf4p)(a.psc + c) : mu, ph = a.psc ? *(gcf4p)(a.psc + a.psc_ld + c) : mu;
    for (int rb = r0 + rl; rb < r1; rb += 8 * rp) {
      f32x4 g[8], xv[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const long o = (long)min(rb + i * rp, r1 - 1) * C + c;
        g[i] = *(gcf4p)(a.dY + o);
        xv[i] = *(gcf4p)(a.X + o);
        if (a.psc) {
#pragma unroll
          for (int j = 0; j < 4; ++j) g[i][j] = fmaf(xv[i][j], ps[j], ph[j]) > 0.f ? g[i][j] : g[i][j] * a.slope;
        } else if (a.post) {
          const f32x4 p = *(gcf4p)(a.post + o);
#pragma unroll
          for (int j = 0; j < 4; ++j) g[i][j] = p[j] > 0.f ? g[i][j] : g[i][j] * a.slope;
        }
      }
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (rb + i * rp < r1) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            x0[j] += (double)g[i][j];
            x1[j] += (double)(g[i][j] * (xv[i][j] - mu[j]));
          }
        }
    }
  } else {
    for (int rb = r0 + rl; rb < r1; rb += 8 * rp) {
      f32x4 xv[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) xv[i] = *(gcf4p)(a.X + (long)min(rb + i * rp, r1 - 1) * C + c);
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (rb + i * rp < r1) {
#pragma unroll
          for (int j = 0; j < 4; ++j) x0[j] += (double)xv[i][j];
        }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    s0[threadIdx.x * 4 + j] = x0[j];
    s1[threadIdx.x * 4 + j] = x1[j];
  }
  __syncthreads();
  if (a.mode == 0) {
    if (rl == 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        double t = 0.0;
        for (int q = 0; q < rp; ++q) t += s0[(q * CW + cs) * 4 + j];
        tot[c + j] = t;
      }
    }
    __syncthreads();
    double mean[4], m2[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 4; ++j) mean[j] = tot[c + j] / max(r1 - r0, 1);
    for (int rb = r0 + rl; rb < r1; rb += 8 * rp) {
      f32x4 xv[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) xv[i] = *(gcf4p)(a.X + (long)min(rb + i * rp, r1 - 1) * C + c);
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (rb + i * rp < r1) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const double d = (double)xv[i][j] - mean[j];
            m2[j] += d * d;
          }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) s1[threadIdx.x * 4 + j] = m2[j];
    __syncthreads();
    if (rl == 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        double t = 0.0;
        for (int q = 0; q < rp; ++q) t += s1[(q * CW + cs) * 4 + j];
        a.part[((long)blockIdx.x * C + c + j) * 2] = tot[c + j];
        a.part[((long)blockIdx.x * C + c + j) * 2 + 1] = t;
      }
    }
    return;
  }
  if (rl == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double t0 = 0.0, t1 = 0.0;
      for (int q = 0; q < rp; ++q) {
        t0 += s0[(q * CW + cs) * 4 + j];
        t1 += s1[(q * CW + cs) * 4 + j];
      }
      a.part[((long)blockIdx.x * C + c + j) * 2] = t0;
      a.part[((long)blockIdx.x * C + c + j) * 2 + 1] = t1;
    }
  }
}

// launch the 16-byte variant when every operand allows it
inline void launch_chan_reduce(const CglChanArgs& a, int nch, hipStream_t s) {
  auto ok = [](const void* p) { return p == nullptr || ((uintptr_t)p & 15) == 0; };
  if (a.C % 4 == 0 && a.C >= 4 && a.C <= 256 && 256 % (a.C / 4) == 0 && ok(a.X) && ok(a.dY) && ok(a.post) &&
      ok(a.mean) && !getenv("CGL_CHAN_SCALAR"))
    CGL_LAUNCH(CGL_REC(CGL_K_CHAN_REDUCE4, a.mode, 0, a.nv ? CGL_LF_NVALID : 0), cgl_chan_reduce4, dim3(nch), dim3(256),
               0, s, a);
  else
    CGL_LAUNCH(CGL_REC(CGL_K_CHAN_REDUCE, a.mode, 0, a.nv ? CGL_LF_NVALID : 0), cgl_chan_reduce, dim3(nch), dim3(256), 0,
               s, a);
}

// Column sums of X [rows][C] per chunk of R rows (any C): part[chunk][c][0] (double); 8 loads in
// flight per thread, summed in row order.
__global__ __launch_bounds__(256) void cgl_colsum_k(const float* X, int rows, int C, int R, double* part) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const int r0 = blockIdx.y * R, r1 = min(r0 + R, rows);
  double t = 0.0;
  for (int rb = r0; rb < r1; rb += 8) {
    float xv[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) xv[i] = gld(X + (long)min(rb + i, r1 - 1) * C + c);
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (rb + i < r1) t += (double)xv[i];
  }
  part[((long)blockIdx.y * C + c) * 2] = t;
  part[((long)blockIdx.y * C + c) * 2 + 1] = 0.0;
}

// BatchNorm2d finalize: ONE WORKGROUP PER CHANNEL, threads over the chunk partials (thread t takes
// chunks t, t + 256, ... in order, then a fixed xor-tree in each wave and the 4 wave sums in wave
// order: deterministic), groups in the reference's call order.
//   fwd (mode 0): mean / biased var per group from the chunk partials (Chan), save_mean / invstd,
//                 scale = invstd * gamma, shift = beta - mean * scale, running stats (momentum,
//                 unbiased variance) group by group; eval: the same from running stats.
//   bwd (mode 1): per group gm = S / n, k = D invstd^2 / n; dgamma = sum_g D invstd, dbeta = sum_g S.
//   bias (mode 2): out = sum of every chunk.
struct CglBnFinArgs {
  const double* part; int C, groups, chunks_per_group, R, gr, mode, train;
  const float* gamma; const float* beta;
  double eps, momentum;
  float* run_mean; float* run_var;
  float* save_mean; float* save_invstd;     // [groups][C]
  float* coef0; float* coef1;               // [groups][C]: fwd scale, shift; bwd gm, k
  float* dgamma; float* dbeta;              // bwd, or bias out (mode 2: dgamma)
  int nocache;                              // A/B switch: stream the partials twice (CGL_FIN_NOCACHE)
  // a short first call (the D step's real call on DataLoader's short final batch): only its first *nv images
  // (hw rows each) carry data -- group 0 counts nv * hw rows, and chunk q of it min(max(nv hw - q R, 0), R)
  const int* nv; int hw;
};

// rows of group g and of chunk q of it (cgl_nv_rows for the short first call)
__device__ __forceinline__ int cgl_fin_rows(const CglBnFinArgs& a, int g) {
  return g == 0 ? cgl_nv_rows(a.nv, a.hw, a.gr) : a.gr;
}
__device__ __forceinline__ int cgl_fin_chunk_rows(int n, int q, int R) { return min(max(n - q * R, 0), R); }

__device__ __forceinline__ double cgl_wave_sum_d(double x) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

// sum over the 256 threads of a workgroup, returned to every thread (every thread must call it)
__device__ __forceinline__ double cgl_block_sum_d(double x, double* red) {
  x = cgl_wave_sum_d(x);
  __syncthreads();                       // red[] free (a previous call may still be reading it)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// sum over chunks q = lane, lane + 256, ... < cnt of f(part pair at chunk q0 + q) -- 8 independent
// 16-byte loads in flight per thread, accumulated in chunk order (the per-thread order is fixed)
// (fn(pair, q): q = the chunk's index within its group, qbase = that of chunk q0)
template <class Fn>
__device__ __forceinline__ double cgl_fin_sum(const double* part, long q0, int cnt, int C, int c, int lane, Fn fn,
                                              int qbase = 0) {
  typedef double f64x2 __attribute__((ext_vector_type(2)));
  typedef const CGL_GLOBAL f64x2* gcd2p;
  double t = 0.0;
  for (int qb = lane; qb < cnt; qb += 8 * 256) {
    f64x2 v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = *(gcd2p)(part + ((q0 + min(qb + 256 * i, cnt - 1)) * C + c) * 2);
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (qb + 256 * i < cnt) t += fn(v[i], qbase + qb + 256 * i);
  }
  return t;
}

// This thread's chunk pairs of up to 2 groups x NI chunks (chunk q0_g + lane + 256 i), all loaded
// up front: the second pass over the partials (and every group) then costs no memory round trip.
// sum(g, fn) accumulates in the same chunk order as cgl_fin_sum.
template <int NI>
struct CglFinCache {
  typedef double f64x2 __attribute__((ext_vector_type(2)));
  f64x2 v[2][NI];
  int cnt, lane;
  __device__ __forceinline__ void load(const double* part, long gstride, int groups, int cnt_, int C, int c,
                                       int lane_, long q0 = 0) {
    typedef const CGL_GLOBAL f64x2* gcd2p;
    cnt = cnt_;
    lane = lane_;
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int q = min(lane + 256 * i, cnt - 1);
        const int gg = min(g, groups - 1);
        v[g][i] = *(gcd2p)(part + ((q0 + gg * gstride + q) * C + c) * 2);
      }
  }
  template <class Fn>
  __device__ __forceinline__ double sum(int g, Fn fn, int qbase = 0) const {
    // the group is selected, not indexed: a runtime index into v[][] puts the cache in scratch
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < NI; ++i)
      if (lane + 256 * i < cnt) t += fn(g ? v[1][i] : v[0][i], qbase + lane + 256 * i);
    return t;
  }
};

// channel c's finalize by one workgroup (cgl_bn_finalize; the deferred column-sum finish of
// cgl_conv_wgrad_reduce_multi); red: 4 doubles of LDS
template <class FA>
__device__ __forceinline__ void cgl_bn_finalize_at(const FA& a, int c, double* red) {
  const int lane = threadIdx.x;          // thread index within the channel's workgroup
  const int C = a.C;
  const double* part = a.part;
  // <= 1024 chunks per call and <= 2 calls: every partial this thread needs is loaded once, up front
  CglFinCache<4> fc;
  const bool cached = a.chunks_per_group <= 1024 && a.groups <= 2 && a.mode != 2 && (a.mode == 1 || a.train) &&
                      !a.nocache;
  if (cached) fc.load(part, a.chunks_per_group, a.groups, a.chunks_per_group, C, c, lane);
  auto gsum = [&](int g, auto fn) -> double {
    return cached ? fc.sum(g, fn) : cgl_fin_sum(part, (long)g * a.chunks_per_group, a.chunks_per_group, C, c, lane, fn);
  };
  if (a.mode == 2) {
    const int nch = a.groups * a.chunks_per_group;
    double t = cgl_fin_sum(part, 0, nch, C, c, lane, [](auto v, int) { return (double)v[0]; });
    t = cgl_block_sum_d(t, red);
    if (lane == 0) gst(a.dgamma + c, (float)t);
    return;
  }
  const float w = a.gamma ? gld(a.gamma + c) : 1.f;
  if (a.mode == 1) {
    double dg = 0.0, db = 0.0;
    for (int g = 0; g < a.groups; ++g) {
      double S = gsum(g, [](auto v, int) { return (double)v[0]; });
      double D = gsum(g, [](auto v, int) { return (double)v[1]; });
      S = cgl_block_sum_d(S, red);
      D = cgl_block_sum_d(D, red);
      const float invstd = gld(a.save_invstd + (long)g * C + c);
      const int ng = cgl_fin_rows(a, g);
      if (lane == 0) {
        gst(a.coef0 + (long)g * C + c, (float)(S / ng));
        gst(a.coef1 + (long)g * C + c, (float)D * invstd * invstd / ng);
      }
      dg += D * (double)invstd;
      db += S;
    }
    if (lane == 0) {
      if (a.dgamma) gst(a.dgamma + c, (float)dg);
      if (a.dbeta) gst(a.dbeta + c, (float)db);
    }
    return;
  }
  const float b = a.beta ? gld(a.beta + c) : 0.f;
  if (!a.train) {
    if (lane != 0) return;
    const double invstd = 1.0 / sqrt((double)gld(a.run_var + c) + a.eps);
    const float sc = (float)invstd * w;
    for (int g = 0; g < a.groups; ++g) {
      gst(a.coef0 + (long)g * C + c, sc);
      gst(a.coef1 + (long)g * C + c, b - gld(a.run_mean + c) * sc);
    }
    return;
  }
  float rm = a.run_mean ? gld(a.run_mean + c) : 0.f, rv = a.run_var ? gld(a.run_var + c) : 0.f;
  for (int g = 0; g < a.groups; ++g) {
    double s = gsum(g, [](auto v, int) { return (double)v[0]; });
    s = cgl_block_sum_d(s, red);
    const int ng = cgl_fin_rows(a, g);
    const double n = ng;
    const double mu = s / n;
    const double R = a.R;
    const bool full = ng == a.gr;            // every chunk holds R rows (the common case: one code path)
    double m2 = gsum(g, [&](auto v, int q) {
      const double cnt = full ? R : (double)cgl_fin_chunk_rows(ng, q, a.R);
      if (cnt == 0.0) return 0.0;
      const double dd = v[0] / cnt - mu;
      return (double)v[1] + cnt * dd * dd;
    });
    m2 = cgl_block_sum_d(m2, red);
    const double invstd = 1.0 / sqrt(m2 / n + a.eps);
    const float sc = (float)invstd * w;
    if (lane == 0) {
      gst(a.coef0 + (long)g * C + c, sc);
      gst(a.coef1 + (long)g * C + c, b - (float)mu * sc);
      if (a.save_mean) {
        gst(a.save_mean + (long)g * C + c, (float)mu);
        gst(a.save_invstd + (long)g * C + c, (float)invstd);
      }
    }
    if (a.run_mean) {
      const double mom = a.momentum;
      rm = (float)(mom * mu + (1.0 - mom) * (double)rm);
      rv = (float)(mom * (n > 1 ? m2 / (n - 1) : m2 / n) + (1.0 - mom) * (double)rv);
    }
  }
  if (a.run_mean && lane == 0) {
    gst(a.run_mean + c, rm);
    gst(a.run_var + c, rv);
  }
}

__global__ __launch_bounds__(256) void cgl_bn_finalize(CglBnFinArgs a) {
  __shared__ double red[4];
  cgl_bn_finalize_at(a, (int)blockIdx.x, red);
}


// Sliced training-mode BatchNorm2d finalize for statistics with many chunks (the 32-row chunks a
// conv epilogue writes: 8192 per forward call of the generator's last BatchNorm at B=256): block
// (s, c) merges slice s of channel c's chunks of every call into {mean_s, M2_s} (two passes, fixed
// order), publishes them with agent-scope atomic stores and takes a ticket; the last block of
// channel c merges the S slices in slice order (Chan) and finishes exactly as cgl_bn_finalize mode
// 0.  The caller zeroes the tickets once; a launch counts a channel's ticket up to S and its last block
// stores 0 again, so launches that share a scratch (stream-ordered) may differ in S.
#define CGL_FIN_MAXS 64
struct CglBnFinSliced {
  CglBnFinArgs f;
  int S, L;                  // slices per channel, chunks per slice
  double* sl;                // [C][groups][S][2] slice {mean, M2}
  unsigned int* ctr;         // [C] tickets
};

__global__ __launch_bounds__(256) void cgl_bn_finalize_sliced(CglBnFinSliced a) {
  __shared__ double red[4];
  __shared__ double smu[CGL_FIN_MAXS], sm2[CGL_FIN_MAXS];
  __shared__ int last;
  const int s = blockIdx.x, c = blockIdx.y, lane = threadIdx.x;
  const int C = a.f.C, cpg = a.f.chunks_per_group, G = a.f.groups, S = a.S;
  const int q_lo = s * a.L, cnt = min(q_lo + a.L, cpg) - q_lo;
  const double R = a.f.R;
  CglFinCache<2> fc;                     // a slice is <= 512 chunks: <= 2 per thread and call
  if (G <= 2 && a.L <= 512) fc.load(a.f.part, cpg, G, cnt, C, c, lane, q_lo);
  for (int g = 0; g < G; ++g) {
    const long q0 = (long)g * cpg + q_lo;
    auto gsum = [&](auto fn) -> double {
      return (G <= 2 && a.L <= 512) ? fc.sum(g, fn, q_lo) : cgl_fin_sum(a.f.part, q0, cnt, C, c, lane, fn, q_lo);
    };
    const int ng = cgl_fin_rows(a.f, g);
    const bool full = ng == a.f.gr;
    const int srows = full ? cnt * a.f.R : min(max(ng - q_lo * a.f.R, 0), cnt * a.f.R);   // this slice's rows
    double sm = gsum([](auto v, int) { return (double)v[0]; });
    sm = cgl_block_sum_d(sm, red);
    const double mu = full ? sm / (cnt * R) : (srows > 0 ? sm / srows : 0.0);
    double m2 = gsum([&](auto v, int q) {
      const double rq = full ? R : (double)cgl_fin_chunk_rows(ng, q, a.f.R);
      if (rq == 0.0) return 0.0;
      const double dd = v[0] / rq - mu;
      return (double)v[1] + rq * dd * dd;
    });
    m2 = cgl_block_sum_d(m2, red);
    if (lane == 0) {
      double* dst = a.sl + (((long)c * G + g) * S + s) * 2;
      cgl_pubd(dst, mu);
      cgl_pubd(dst + 1, m2);
    }
  }
  if (lane == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the published words have landed
    const unsigned int old = __hip_atomic_fetch_add((cgl_gu32*)(a.ctr + c), 1u, __ATOMIC_RELAXED,
                                                    __HIP_MEMORY_SCOPE_AGENT);
    last = old == (unsigned)(S - 1);
    // every block of the channel has drawn its ticket, so nothing in this launch touches it again: back to 0 at once
    // (the store overlaps the merge below), and the next launch on this scratch -- stream-ordered after this one --
    // may cut the channel into another number of slices
    if (last) __hip_atomic_store((cgl_gu32*)(a.ctr + c), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (!last) return;
  const float w = a.f.gamma ? gld(a.f.gamma + c) : 1.f;
  const float b = a.f.beta ? gld(a.f.beta + c) : 0.f;
  float rm = a.f.run_mean ? gld(a.f.run_mean + c) : 0.f, rv = a.f.run_var ? gld(a.f.run_var + c) : 0.f;
  for (int g = 0; g < G; ++g) {
    if (lane < S) {
      const double* src = a.sl + (((long)c * G + g) * S + lane) * 2;
      smu[lane] = __longlong_as_double((long long)cgl_ld64(src));
      sm2[lane] = __longlong_as_double((long long)cgl_ld64(src + 1));
    }
    __syncthreads();
    if (lane == 0) {
      const int ng = cgl_fin_rows(a.f, g);
      const bool full = ng == a.f.gr;
      const double n = ng;
      // rows of slice q (all of its chunks' R rows, or the short call's share of them)
      auto qrows = [&](int q) -> double {
        const int rq = (min((q + 1) * a.L, cpg) - q * a.L) * a.f.R;
        return full ? (double)(min((q + 1) * a.L, cpg) - q * a.L) * R : (double)min(max(ng - q * a.L * a.f.R, 0), rq);
      };
      double tot = 0.0;
      for (int q = 0; q < S; ++q) tot += full ? smu[q] * (min((q + 1) * a.L, cpg) - q * a.L) * R : smu[q] * qrows(q);
      const double mu = tot / n;
      double m2 = 0.0;
      for (int q = 0; q < S; ++q) {
        const double dd = smu[q] - mu;
        m2 += sm2[q] + qrows(q) * dd * dd;
      }
      const double invstd = 1.0 / sqrt(m2 / n + a.f.eps);
      const float sc = (float)invstd * w;
      gst(a.f.coef0 + (long)g * C + c, sc);
      gst(a.f.coef1 + (long)g * C + c, b - (float)mu * sc);
      if (a.f.save_mean) {
        gst(a.f.save_mean + (long)g * C + c, (float)mu);
        gst(a.f.save_invstd + (long)g * C + c, (float)invstd);
      }
      if (a.f.run_mean) {
        const double mom = a.f.momentum;
        rm = (float)(mom * mu + (1.0 - mom) * (double)rm);
        rv = (float)(mom * (n > 1 ? m2 / (n - 1) : m2 / n) + (1.0 - mom) * (double)rv);
      }
    }
    __syncthreads();
  }
  if (a.f.run_mean && lane == 0) {
    gst(a.f.run_mean + c, rm);
    gst(a.f.run_var + c, rv);
  }
}

// Elementwise NHWC passes (float4 over channels; C % 4 == 0):
//   mode 0  Y = act(X * coef0[g][c] + coef1[g][c])                               (BatchNorm2d apply)
//   mode 1  dX = (g - coef0[g][c] - (X - mean[g][c]) coef1[g][c]) invstd[g][c] gamma[c],
//           g = dY * leaky'(post)  (BatchNorm2d backward apply), then * drop * leaky'(post_out)
//   mode 2  dX = dY * leaky'(post_out) * drop                      (Dropout2d + LeakyReLU backward)
//   mode 3  dX = dY * (1 - Y^2)                                                  (Tanh backward)
struct CglEltArgs {
  int mode, rows, C, gr, hw, act;
  int row0;                  // the first row of X / out is row row0 of the whole tensor (its BatchNorm group)
  float slope;
  const float* X; const float* dY; const float* post;
  const float* coef0; const float* coef1; const float* mean; const float* invstd; const float* gamma;
  const float* post_out; const float* drop;
  float* out;
  const int* nv;             // mode 1, short first call: rows >= *nv * hw of group 0 are padding -> dX = 0
  const float* psc; int psc_ld;   // mode 1: LeakyReLU'(post) from the forward's scale / shift (CglChanArgs)
  // cgl_eltwise1, C == 1, one element per thread: also the column-sum partials of the output per 256-row chunk
  // (= block), {sum, 0} -- bitwise cgl_chan_reduce mode 2 with R = 256 over the stored output
  double* colsum;
};

// one float4 of cgl_eltwise mode 1 (the BatchNorm2d backward apply) at element e = (row r, channel c), BatchNorm
// group g (gc = g C + c), nvr: the data rows of a short first call (cgl_eltwise, cgl_bnb_apply_colsum)
__device__ __forceinline__ f32x4 cgl_elt_bnb4(const CglEltArgs& a, long e, int r, int c, int g, long gc, int nvr) {
  const float sl = a.slope;
  f32x4 o;
  const f32x4 x = *(gcf4p)(a.X + e), dy = *(gcf4p)(a.dY + e);
  const f32x4 gm = *(gcf4p)(a.coef0 + gc), kk = *(gcf4p)(a.coef1 + gc);
  const f32x4 mu = *(gcf4p)(a.mean + gc), is = *(gcf4p)(a.invstd + gc), w = *(gcf4p)(a.gamma + c);
  f32x4 p = dy;
  if (a.psc) {
    const f32x4 ps = *(gcf4p)(a.psc + c), ph = *(gcf4p)(a.psc + a.psc_ld + c);
#pragma unroll
    for (int j = 0; j < 4; ++j) p[j] = fmaf(x[j], ps[j], ph[j]);
  } else if (a.post) {
    p = *(gcf4p)(a.post + e);
  }
  const bool pon = a.psc || a.post;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float gg = pon ? (p[j] > 0.f ? dy[j] : dy[j] * sl) : dy[j];
    o[j] = (gg - gm[j] - (x[j] - mu[j]) * kk[j]) * is[j] * w[j];
  }
  if (a.post_out) {
    const f32x4 po = *(gcf4p)(a.post_out + e);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = po[j] > 0.f ? o[j] : o[j] * sl;
  }
  if (a.drop) {
    const f32x4 dm = *(gcf4p)(a.drop + (long)(r / a.hw) * a.C + c);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] *= dm[j];
  }
  if (g == 0 && r + a.row0 >= nvr) o = f32x4{0.f, 0.f, 0.f, 0.f};   // padding of a short first call
  return o;
}

// cgl_eltwise mode 1 (the BatchNorm2d backward apply) over 256-row chunks, one per workgroup, that also writes the
// per-chunk column sums of its output in cgl_chan_reduce4 mode 2's lane mapping, order and layout (R = 256:
// part[chunk][c] = {sum, 0}) -- bitwise the apply followed by col_sum's channel reduction over the stored output
// (the bias gradient of the conv whose output gradient this is), one pass over the tensor fewer.  Rows of a lane
// in batches of NB (their loads in flight together), accumulated in row order.
#ifndef CGL_BNB_NB
#define CGL_BNB_NB 4   // rows of a lane in flight together (16 measured the same, gpurun_out/r06zg)
#endif
template <int NB>
__global__ __launch_bounds__(256) void cgl_bnb_apply_colsum(CglEltArgs a, double* __restrict__ part) {
  __shared__ double s0[1024];
  const int C = a.C, CW = C >> 2, rp = 256 / CW;
  const int cs = threadIdx.x % CW, rl = threadIdx.x / CW, c = 4 * cs;
  const int r0 = blockIdx.x * 256, r1 = min(r0 + 256, a.rows);
  const int nvr = cgl_nv_rows(a.nv, a.hw, a.gr);
  double x0[4] = {0.0, 0.0, 0.0, 0.0};
  for (int rb = r0 + rl; rb < r1; rb += NB * rp) {
    f32x4 o[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int r = min(rb + i * rp, r1 - 1);
      const int g = (r + a.row0) / a.gr;
      o[i] = cgl_elt_bnb4(a, (long)r * C + c, r, c, g, (long)g * C + c, nvr);
    }
#pragma unroll
    for (int i = 0; i < NB; ++i)
      if (rb + i * rp < r1) {
        *(gf4p)(a.out + (long)(rb + i * rp) * C + c) = o[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) x0[j] += (double)o[i][j];
      }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) s0[threadIdx.x * 4 + j] = x0[j];
  __syncthreads();
  if (rl == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double t0 = 0.0, t1 = 0.0;
      for (int q = 0; q < rp; ++q) t0 += s0[(q * CW + cs) * 4 + j];
      part[((long)blockIdx.x * C + c + j) * 2] = t0;
      part[((long)blockIdx.x * C + c + j) * 2 + 1] = t1;
    }
  }
}

__global__ __launch_bounds__(256) void cgl_eltwise(CglEltArgs a) {
  const long n4 = (long)a.rows * a.C / 4;
  const int C = a.C;
  const float sl = a.slope;
  const int nvr = a.mode == 1 ? cgl_nv_rows(a.nv, a.hw, a.gr) : a.gr;
  // 32-bit index arithmetic when the tensor allows it (a 64-bit division per float4 costs more VALU
  // than the element work)
  const bool small = n4 < (1L << 29);
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < n4; q += (long)gridDim.x * 256) {
    const long e = q * 4;
    int r, c;
    if (small) {
      const unsigned eu = (unsigned)e, ru = eu / (unsigned)C;
      r = (int)ru;
      c = (int)(eu - ru * (unsigned)C);
    } else {
      r = (int)(e / C);
      c = (int)(e - (long)r * C);
    }
    const int g = (r + a.row0) / a.gr;
    const long gc = (long)g * C + c;
    f32x4 o;
    if (a.mode == 0) {
      const f32x4 x = *(gcf4p)(a.X + e);
      const f32x4 s = *(gcf4p)(a.coef0 + gc), h = *(gcf4p)(a.coef1 + gc);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float v = fmaf(x[j], s[j], h[j]);
        if (a.act == CGL_EPI_ACT_LEAKY) v = v > 0.f ? v : v * sl;
        o[j] = v;
      }
    } else if (a.mode == 1) {
      o = cgl_elt_bnb4(a, e, r, c, g, gc, nvr);
    } else if (a.mode == 2) {
      const f32x4 dy = *(gcf4p)(a.dY + e);
      o = dy;
      if (a.post_out) {
        const f32x4 po = *(gcf4p)(a.post_out + e);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = po[j] > 0.f ? o[j] : o[j] * sl;
      }
      if (a.drop) {
        const f32x4 dm = *(gcf4p)(a.drop + (long)(r / a.hw) * C + c);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] *= dm[j];
      }
    } else {
      const f32x4 dy = *(gcf4p)(a.dY + e), y = *(gcf4p)(a.X + e);
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = cgl_dtanh(dy[j], y[j]);
    }
    *(gf4p)(a.out + e) = o;
  }
}

// Scalar fallback of mode 2 / 3 for C % 4 != 0 (single-channel tensors: the generator image).
__global__ __launch_bounds__(256) void cgl_eltwise1(CglEltArgs a) {
  const long n = (long)a.rows * a.C;
  float ov = 0.f;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
    const int r = (int)(e / a.C), c = (int)(e - (long)r * a.C);
    float o = gld(a.dY + e);
    if (a.mode == 3) {
      const float y = gld(a.X + e);
      o = cgl_dtanh(o, y);
    } else {
      if (a.post_out) o = gld(a.post_out + e) > 0.f ? o : o * a.slope;
      if (a.drop) o *= gld(a.drop + (long)(r / a.hw) * a.C + c);
    }
    gst(a.out + e, o);
    ov = o;
  }
  if (a.colsum) {      // (uniform) the chunk's rows summed in row order, as cgl_chan_reduce's thread 0 does
    __shared__ double s0[256];
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    s0[threadIdx.x] = e < n ? (double)ov : 0.0;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = 0.0;
      for (int q = 0; q < 256; ++q) t += s0[q];
      a.colsum[(long)blockIdx.x * 2] = t;
      a.colsum[(long)blockIdx.x * 2 + 1] = 0.0;
    }
  }
}

namespace {

int fin_nocache() {
  static const int v = getenv("CGL_FIN_NOCACHE") ? atoi(getenv("CGL_FIN_NOCACHE")) : 0;
  return v;
}

// Rows per channel-reduction chunk (one workgroup each): 128, halved down to 32 while a BatchNorm call would
// get fewer than 64 chunks -- the discriminator's 2 x 2 and 4 x 4 maps (1024-4096 rows per call) otherwise ran
// their reduction on 8-32 workgroups, latency-bound (CGL_CHAN_MINCH=0: plain 128).
int chan_chunk(int64_t gr) {
  static const int minch = getenv("CGL_CHAN_MINCH") ? atoi(getenv("CGL_CHAN_MINCH")) : 64;
  int R = 128;
  while (R > 1 && gr % R != 0) R >>= 1;
  while (R > 32 && gr / R < minch && gr % (R >> 1) == 0) R >>= 1;
  return R;
}

bool pow2_le256(int C) { return C >= 1 && C <= 256 && (C & (C - 1)) == 0; }

// record + launch: cgl_bn_finalize on one workgroup per channel
void launch_bn_finalize(const CglBnFinArgs& f, hipStream_t s) {
  CGL_LAUNCH(CGL_REC(CGL_K_BN_FINALIZE, f.mode, 0, f.nv ? CGL_LF_NVALID : 0), cgl_bn_finalize, dim3(f.C), dim3(256), 0,
             s, f);
}

// record + launch: cgl_eltwise, 256 float4 per workgroup, grid-stride beyond 8192 workgroups
void launch_eltwise(const CglEltArgs& e, hipStream_t s) {
  const long n4 = (long)e.rows * e.C / 4;
  CGL_LAUNCH(CGL_REC(CGL_K_ELTWISE, e.mode, 0, e.nv ? CGL_LF_NVALID : 0), cgl_eltwise,
             dim3((unsigned)std::min<long>((n4 + 255) / 256, 8192)), dim3(256), 0, s, e);
}

// per-column sum of X [rows][C] into out[C] (bias gradient): chunk partials (double), then a
// fixed-order sum over chunks (cgl_bn_finalize mode 2)
// the column sums' partial pass (launched) and their finalize's arguments (f: launched by the caller)
int col_sum_part(const float* X, int64_t rows, int C, double* part, float* out, hipStream_t s, CglBnFinArgs& f) {
  int nch;
  if (pow2_le256(C)) {
    const int R = 256;
    nch = (int)((rows + R - 1) / R);
    CglChanArgs a;
    std::memset(&a, 0, sizeof(a));
    a.X = X; a.rows = (int)rows; a.C = C; a.R = R; a.mode = 2; a.gr = (int)rows; a.part = part;
    launch_chan_reduce(a, nch, s);
  } else {
    const int R = 32;
    nch = (int)((rows + R - 1) / R);
    CGL_LAUNCH(CGL_REC(CGL_K_COLSUM, 0, 0, 0), cgl_colsum_k, dim3((C + 255) / 256, nch), dim3(256), 0, s, X, (int)rows, C,
               R, part);
  }
  std::memset(&f, 0, sizeof(f));
  f.part = part; f.C = C; f.groups = 1; f.chunks_per_group = nch; f.mode = 2; f.dgamma = out;
  f.nocache = fin_nocache();
  return (int)hipGetLastError();
}

int col_sum(const float* X, int64_t rows, int C, double* part, float* out, hipStream_t s) {
  CglBnFinArgs f;
  const int rc = col_sum_part(X, rows, C, part, out, s, f);
  if (rc) return rc;
  launch_bn_finalize(f, s);
  return (int)hipGetLastError();
}

}  // namespace
