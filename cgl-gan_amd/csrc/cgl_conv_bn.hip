// BatchNorm2d and the elementwise passes of the conv path, host side: the entry points over cgl_conv_bn.h's kernels
// and launch helpers.  Included by cgl_conv_tu.hip after cgl_conv.hip (CGL_CONV_ENTRY, al256, t_wdefer).
// Each BatchNorm2d direction has one path from chunk partials to the applied tensor: cgl_bn2d_fwd / cgl_bn2d_bwd run
// it behind their own channel reduction into the workspace (own), the _stats forms on the caller's partials.  Every
// check ahead of the workspace size returns CGL_E_ARG; they stand in the _stats forms' order.

namespace {

bool bn2d_shape_ok(int n, int hw, int C, int groups) {
  return n >= 1 && hw >= 1 && C % 4 == 0 && pow2_le256(C) && groups >= 1 && n % groups == 0;
}

// A cgl_bn2d_* call's workspace: the chunk partials of its own reduction (R = chan_chunk rows each), then the two
// [groups][C] coefficient slots of the finalize (fwd scale, shift; bwd gm, k)
struct Bn2dWs {
  int R;
  int64_t nch, part_bytes, coef_bytes;
  Bn2dWs(int n, int hw, int C, int groups)
      : R(chan_chunk((int64_t)(n / groups) * hw)), nch((int64_t)n * hw / R), part_bytes(al256(nch * C * 16)),
        coef_bytes(al256((int64_t)groups * C * 4)) {}
  int64_t bytes() const { return part_bytes + 4 * coef_bytes + 256; }
  float* coef(void* ws, int i) const { return (float*)((char*)ws + part_bytes + i * coef_bytes); }
};

// Forward from {sum, M2} partials of R rows (own: the call's reduction, training only): finalize -- sliced with
// `scratch` and more than 1024 chunks per group -- into `coef` ([2][groups][C]) or the workspace's slots, then the
// apply to images [apply_img0, n) (a consumer folds the rest into its operand load from `coef`)
int bn2d_fwd_impl(bool own, const double* part, int R, int train, const float* X, int n, int hw, int C, int groups,
                  const float* gamma, const float* beta, double eps, double momentum, float* running_mean,
                  float* running_var, int act, float slope, float* Y, float* save_mean, float* save_invstd,
                  void* scratch, float* coef, int apply_img0, const int* nvalid, void* ws, int64_t wsb, hipStream_t s) {
  if ((!own && !part) || !X || !Y || !gamma || !beta || !ws || !al16(ws) || !al16(X) || !al16(Y)) return CGL_E_ARG;
  if ((coef && !al16(coef)) || apply_img0 < 0 || apply_img0 > n) return CGL_E_ARG;
  if (!bn2d_shape_ok(n, hw, C, groups) || (act != 0 && act != 1)) return CGL_E_ARG;
  if ((running_mean == nullptr) != (running_var == nullptr)) return CGL_E_ARG;
  if ((save_mean == nullptr) != (save_invstd == nullptr)) return CGL_E_ARG;
  if (!train && !running_mean) return CGL_E_ARG;
  const int64_t gr = (int64_t)(n / groups) * hw, rows = (int64_t)n * hw;
  if (!own && (R < 1 || gr % R)) return CGL_E_ARG;
  if (train && gr < 2) return CGL_E_ARG;   // torch: "Expected more than 1 value per channel when training"
  const Bn2dWs w(n, hw, C, groups);
  if (wsb < w.bytes()) return CGL_E_SIZE;
  if (own) {
    part = (const double*)ws, R = w.R;
    if (train) {
      CglChanArgs a;
      std::memset(&a, 0, sizeof(a));
      a.X = X; a.rows = (int)rows; a.C = C; a.R = R; a.mode = 0; a.gr = (int)gr; a.part = (double*)ws;
      a.nv = nvalid; a.hw = hw;
      launch_chan_reduce(a, (int)w.nch, s);
    }
  }
  const int cpg = (int)(gr / R);
  CglBnFinArgs f;
  std::memset(&f, 0, sizeof(f));
  f.part = part; f.C = C; f.groups = groups; f.chunks_per_group = cpg; f.R = R; f.gr = (int)gr;
  f.nv = train ? nvalid : nullptr; f.hw = hw;
  f.mode = 0; f.train = train; f.gamma = gamma; f.beta = beta; f.eps = eps; f.momentum = momentum;
  f.run_mean = running_mean; f.run_var = running_var; f.save_mean = save_mean; f.save_invstd = save_invstd;
  f.coef0 = coef ? coef : w.coef(ws, 0);
  f.coef1 = coef ? coef + (int64_t)groups * C : w.coef(ws, 1);
  if (scratch && cpg > 1024) {   // many chunks: slices of <= 512 per block, merged by the last block
    if ((uintptr_t)scratch & 255) return CGL_E_ARG;
    CglBnFinSliced a;
    std::memset(&a, 0, sizeof(a));
    a.f = f;
    a.L = 512;
    a.S = (cpg + a.L - 1) / a.L;
    if (a.S > CGL_FIN_MAXS) a.L = (cpg + CGL_FIN_MAXS - 1) / CGL_FIN_MAXS, a.S = (cpg + a.L - 1) / a.L;
    a.ctr = (unsigned int*)scratch;
    a.sl = (double*)((char*)scratch + al256((int64_t)C * 4));
    CGL_LAUNCH(CGL_REC(CGL_K_BN_FINALIZE_SLICED, f.mode, 0, f.nv ? CGL_LF_NVALID : 0), cgl_bn_finalize_sliced,
               dim3(a.S, C), dim3(256), 0, s, a);
  } else {
    f.nocache = fin_nocache();
    launch_bn_finalize(f, s);
  }
  const int64_t row0 = (int64_t)apply_img0 * hw, arows = rows - row0;
  if (arows <= 0) return (int)hipGetLastError();
  CglEltArgs e;
  std::memset(&e, 0, sizeof(e));
  e.mode = 0; e.rows = (int)arows; e.C = C; e.gr = (int)gr; e.hw = hw; e.act = act; e.slope = slope;
  e.row0 = (int)row0;
  e.X = X + row0 * C; e.coef0 = f.coef0; e.coef1 = f.coef1; e.out = Y + row0 * C;
  launch_eltwise(e, s);
  return (int)hipGetLastError();
}

// Backward from {sum g, sum g (x - mean)} partials of R rows (own: the call's reduction): finalize (dgamma, dbeta,
// gm, k), then the apply -- with colsum_part on 256-row chunks that also leave the output's column sums per chunk
// (a bias gradient's col_sum partials)
int bn2d_bwd_impl(bool own, const double* part, int R, const float* dY, const float* post, const float* X, int n,
                  int hw, int C, int groups, const float* save_mean, const float* save_invstd, const float* gamma,
                  float slope, const float* post_out, const float* drop, float* dX, float* dgamma, float* dbeta,
                  const float* post_coef, int post_coef_ld, const int* nvalid, double* colsum_part, void* ws,
                  int64_t wsb, hipStream_t s) {
  if (post_coef && (post || groups != 1 || !al16(post_coef) || post_coef_ld % 4)) return CGL_E_ARG;
  // C < 4 first: 256 % (C / 4) divides by zero for C = 0 (C = 1 .. 3 leave at C % 4)
  if (colsum_part && (((uintptr_t)colsum_part & 15) || C < 4 || C % 4 || 256 % (C / 4) || ((int64_t)n * hw) % 256))
    return CGL_E_ARG;
  if ((!own && !part) || !dY || !X || !save_mean || !save_invstd || !gamma || !dX || !ws || !al16(ws))
    return CGL_E_ARG;
  if (!al16(dY) || !al16(X) || !al16(dX) || (post && !al16(post)) || (post_out && !al16(post_out))) return CGL_E_ARG;
  if (!al16(save_mean) || !al16(save_invstd) || !al16(gamma) || (drop && !al16(drop))) return CGL_E_ARG;
  if (!bn2d_shape_ok(n, hw, C, groups)) return CGL_E_ARG;
  const int64_t gr = (int64_t)(n / groups) * hw, rows = (int64_t)n * hw;
  if (!own && (R < 1 || gr % R)) return CGL_E_ARG;
  const Bn2dWs w(n, hw, C, groups);
  if (wsb < w.bytes()) return CGL_E_SIZE;
  if (own) {
    part = (const double*)ws, R = w.R;
    CglChanArgs a;
    std::memset(&a, 0, sizeof(a));
    a.X = X; a.rows = (int)rows; a.C = C; a.R = R; a.mode = 1; a.gr = (int)gr; a.part = (double*)ws;
    a.dY = dY; a.post = post; a.slope = slope; a.mean = save_mean;
    a.psc = post_coef; a.psc_ld = post_coef_ld;
    launch_chan_reduce(a, (int)w.nch, s);
  }
  CglBnFinArgs f;
  std::memset(&f, 0, sizeof(f));
  f.part = part; f.C = C; f.groups = groups; f.chunks_per_group = (int)(gr / R); f.R = R; f.gr = (int)gr;
  f.mode = 1; f.gamma = gamma; f.save_invstd = const_cast<float*>(save_invstd);
  f.coef0 = w.coef(ws, 0); f.coef1 = w.coef(ws, 1); f.dgamma = dgamma; f.dbeta = dbeta;
  f.nv = nvalid; f.hw = hw;
  f.nocache = fin_nocache();
  launch_bn_finalize(f, s);
  CglEltArgs e;
  std::memset(&e, 0, sizeof(e));
  e.mode = 1; e.rows = (int)rows; e.C = C; e.gr = (int)gr; e.hw = hw; e.slope = slope;
  e.X = X; e.dY = dY; e.post = post; e.coef0 = f.coef0; e.coef1 = f.coef1; e.mean = save_mean; e.invstd = save_invstd;
  e.gamma = gamma; e.post_out = post_out; e.drop = drop; e.out = dX; e.nv = nvalid;
  e.psc = post_coef; e.psc_ld = post_coef_ld;
  if (colsum_part)
    CGL_LAUNCH(CGL_REC(CGL_K_BNB_APPLY_COLSUM, e.mode, 0, e.nv ? CGL_LF_NVALID : 0), cgl_bnb_apply_colsum<CGL_BNB_NB>,
               dim3((unsigned)(rows / 256)), dim3(256), 0, s, e, colsum_part);
  else
    launch_eltwise(e, s);
  return (int)hipGetLastError();
}

// Dropout2d + LeakyReLU backward (mode 2) or Tanh backward (mode 3, post = the forward's output) over [n hw][C]
CglEltArgs act_drop_args(const float* dY, const float* post, const float* drop, int n, int hw, int C, float slope,
                         int tanh_y, float* dX) {
  CglEltArgs e;
  std::memset(&e, 0, sizeof(e));
  e.mode = tanh_y ? 3 : 2;
  e.rows = n * hw; e.C = C; e.gr = n * hw; e.hw = hw; e.slope = slope;
  e.dY = dY; e.out = dX;
  if (tanh_y) e.X = post;
  else e.post_out = post;
  e.drop = drop;
  return e;
}

}  // namespace

extern "C" {

int64_t cgl_bn2d_workspace_bytes(int n, int hw, int C, int groups) {
  if (n < 1 || hw < 1 || C < 1 || groups < 1 || n % groups) return CGL_E_ARG;
  return Bn2dWs(n, hw, C, groups).bytes();
}

int64_t cgl_bn2d_stats_scratch_bytes(int C, int groups) {
  if (C < 1 || groups < 1) return CGL_E_ARG;
  return al256((int64_t)C * 4) + (int64_t)C * groups * CGL_FIN_MAXS * 16;
}

int cgl_bn2d_fwd(const float* X, int n, int hw, int C, int groups, const float* gamma, const float* beta, double eps,
                 double momentum, float* running_mean, float* running_var, int train, int act, float slope, float* Y,
                 float* save_mean, float* save_invstd, const int* nvalid, void* ws, int64_t wsb, void* stream) {
  CGL_CONV_ENTRY();
  return bn2d_fwd_impl(true, nullptr, 0, train, X, n, hw, C, groups, gamma, beta, eps, momentum, running_mean,
                       running_var, act, slope, Y, save_mean, save_invstd, nullptr, nullptr, 0, nvalid, ws, wsb,
                       (hipStream_t)stream);
}

int cgl_bn2d_fwd_stats(const double* part, int R, const float* X, int n, int hw, int C, int groups, const float* gamma,
                       const float* beta, double eps, double momentum, float* running_mean, float* running_var,
                       int act, float slope, float* Y, float* save_mean, float* save_invstd, void* scratch,
                       const int* nvalid, void* ws, int64_t wsb, void* stream) {
  CGL_CONV_ENTRY();
  return bn2d_fwd_impl(false, part, R, 1, X, n, hw, C, groups, gamma, beta, eps, momentum, running_mean, running_var,
                       act, slope, Y, save_mean, save_invstd, scratch, nullptr, 0, nvalid, ws, wsb,
                       (hipStream_t)stream);
}

int cgl_bn2d_fwd_stats_coef(const double* part, int R, const float* X, int n, int hw, int C, int groups,
                            const float* gamma, const float* beta, double eps, double momentum, float* running_mean,
                            float* running_var, int act, float slope, float* Y, float* save_mean, float* save_invstd,
                            void* scratch, float* coef, int apply_img0, const int* nvalid, void* ws, int64_t wsb,
                            void* stream) {
  CGL_CONV_ENTRY();
  return bn2d_fwd_impl(false, part, R, 1, X, n, hw, C, groups, gamma, beta, eps, momentum, running_mean, running_var,
                       act, slope, Y, save_mean, save_invstd, scratch, coef, apply_img0, nvalid, ws, wsb,
                       (hipStream_t)stream);
}

int cgl_bn2d_bwd_stats(const double* part, int R, const float* dY, const float* post, const float* X, int n, int hw,
                       int C, int groups, const float* save_mean, const float* save_invstd, const float* gamma,
                       float slope, const float* post_out, const float* drop, float* dX, float* dgamma, float* dbeta,
                       const float* post_coef, int post_coef_ld, const int* nvalid, double* colsum_part, void* ws,
                       int64_t wsb, void* stream) {
  CGL_CONV_ENTRY();
  return bn2d_bwd_impl(false, part, R, dY, post, X, n, hw, C, groups, save_mean, save_invstd, gamma, slope, post_out,
                       drop, dX, dgamma, dbeta, post_coef, post_coef_ld, nvalid, colsum_part, ws, wsb,
                       (hipStream_t)stream);
}

int cgl_bn2d_bwd(const float* dY, const float* post, const float* X, int n, int hw, int C, int groups,
                 const float* save_mean, const float* save_invstd, const float* gamma, float slope,
                 const float* post_out, const float* drop, float* dX, float* dgamma, float* dbeta,
                 const float* post_coef, int post_coef_ld, const int* nvalid, void* ws, int64_t wsb, void* stream) {
  CGL_CONV_ENTRY();
  return bn2d_bwd_impl(true, nullptr, 0, dY, post, X, n, hw, C, groups, save_mean, save_invstd, gamma, slope,
                       post_out, drop, dX, dgamma, dbeta, post_coef, post_coef_ld, nvalid, nullptr, ws, wsb,
                       (hipStream_t)stream);
}

int cgl_act_drop_bwd(const float* dY, const float* post, const float* drop, int n, int hw, int C, float slope,
                     int tanh_y, float* dX, void* stream) {
  CGL_CONV_ENTRY();
  if (!dY || !dX || n < 1 || hw < 1 || C < 1) return CGL_E_ARG;
  if (tanh_y && !post) return CGL_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  const CglEltArgs e = act_drop_args(dY, post, drop, n, hw, C, slope, tanh_y, dX);
  const long tot = (long)n * hw * C;
  if (C % 4 == 0 && al16(dY) && al16(dX) && (!post || al16(post)) && (!drop || al16(drop)))
    launch_eltwise(e, s);
  else
    CGL_LAUNCH(CGL_REC(CGL_K_ELTWISE1, e.mode, 0, 0), cgl_eltwise1,
               dim3((unsigned)std::min<long>((tot + 255) / 256, 8192)), dim3(256), 0, s, e);
  return (int)hipGetLastError();
}

int cgl_act_drop_bwd_colsum(const float* dY, const float* post, const float* drop, int n, int hw, int C, float slope,
                            int tanh_y, float* dX, double* part, void* stream) {
  CGL_CONV_ENTRY();
  const long tot = (long)n * hw * C;
  if (!dY || !dX || !part || n < 1 || hw < 1 || C != 1 || tot > 8192L * 256 || ((uintptr_t)part & 15)) return CGL_E_ARG;
  if (tanh_y && !post) return CGL_E_ARG;
  CglEltArgs e = act_drop_args(dY, post, drop, n, hw, C, slope, tanh_y, dX);
  e.colsum = part;
  CGL_LAUNCH(CGL_REC(CGL_K_ELTWISE1, e.mode, 0, 0), cgl_eltwise1, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0,
             (hipStream_t)stream, e);
  return (int)hipGetLastError();
}

int cgl_colsum_finalize(const double* part, int nch, int C, float* out, void* stream) {
  CGL_CONV_ENTRY();
  if (!part || !out || nch < 1 || C < 1) return CGL_E_ARG;
  CglBnFinArgs f;
  std::memset(&f, 0, sizeof(f));
  f.part = part; f.C = C; f.groups = 1; f.chunks_per_group = nch; f.mode = 2; f.dgamma = out;
  f.nocache = fin_nocache();
  if (t_wdefer.on && t_wdefer.add_fin(f)) {   // rides in the deferred reductions' launch
    cgl_conv_rec(CGL_K_BN_FINALIZE, f.mode, 0, CGL_LF_DEFERRED, dim3(C), dim3(256), 0);
    return CGL_OK;
  }
  launch_bn_finalize(f, (hipStream_t)stream);
  return (int)hipGetLastError();
}

}  // extern "C"
