// ops_bn.hip -- per-kernel test entries of the C ABI on the BatchNorm training kernels of batchnorm.hip (and their quantising fp8 forms), the channel sums and the
// view copies of elementwise.hip: one call per launch sequence.  Host arrays in and out, nothing a training step calls.
// Host tensors are channel-major [C][rows] (NCHW with B = 1).  y / dy are dense [rows][C] on the device as in the model (a unit's own buffers); z, res, dz and
// rg sit inside sentinel-padded views; partial-row workspaces and dy carry a sentinel guard behind them.
#include "ops_stage.h"

namespace {
constexpr int kEwMaxVec = 256;               // vectors per row the channel-reduction launchers take (EW_THREADS of batchnorm.hip)

// ys_stat_acc_add on test-supplied partial rows [P][2][C]: one thread per (row, which, channel) -- the device function every convolution epilogue calls
__global__ void __launch_bounds__(256)
stat_acc_push_kernel(const float* __restrict__ partial, int P, int C, unsigned long long* __restrict__ acc) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)P * 2 * C) return;
  const long row = i / (2L * C);
  const int which = (int)((i / C) & 1), c = (int)(i % C);
  ys_stat_acc_add(acc, row, C, c, which, partial[i]);
}

// z in a view of a buffer of its own.  res (optional) in a view of its own buffer too, or -- res_shares_z -- in other channels of z's, which is then wide
// enough for both.  `who` names the entry and the problem in the error texts.
int z_res_args(const char* who, int dtype, int C, const float* res, int res_pad, int res_coff, int z_pad, int z_coff, int res_shares_z) {
  YS_TRY(view_on_grid(who, dtype, C, z_coff + C + z_pad, z_coff));
  if (res) YS_TRY(view_on_grid(who, dtype, C, res_coff + C + res_pad, res_coff));
  YS_REQUIRE(!(res && res_shares_z) || res_coff + C <= z_coff || z_coff + C <= res_coff, "%s: res and z views overlap", who);
  return YS_OK;
}
int stage_z_res(hipStream_t st, int dtype, long rows, int C, const float* res, int res_pad, int res_coff, int z_pad, int z_coff, int res_shares_z, PadView& z,
                PadView& r) {
  const bool shared = res && res_shares_z;
  int ldz = z_coff + C + z_pad;
  if (shared && res_coff + C + z_pad > ldz) ldz = res_coff + C + z_pad;
  YS_TRY(z.alloc(st, dtype, rows, C, ldz, z_coff));
  if (!res) return YS_OK;
  if (shared) r.borrow(z, res_coff);
  else YS_TRY(r.alloc(st, dtype, rows, C, res_coff + C + res_pad, res_coff));
  return r.stage(st, res);
}
int check_z_res(hipStream_t st, const PadView& z, const PadView& r, int* ok) {
  YS_TRY(z.check(st, ok, r.p && !r.own.p ? &r : nullptr));
  if (r.own.p) YS_TRY(r.check(st, ok));
  return YS_OK;
}

// a dense [rows][C] device tensor (a unit's own buffer) from a channel-major host tensor
int stage_dense(hipStream_t st, int dtype, const float* host, long rows, int C, DevBuf& d) {
  YS_TRY(d.alloc((size_t)rows * C * ys_es(dtype)));
  return stage_view(st, dtype, host, 1, C, rows, d.p, C, 0);
}

struct BnFwdBufs {
  DevBuf y, par, part, acc;
  PadView z, res;
  int nblk = 0;
  size_t npart = 0;
  float *g, *bt, *rm, *rv, *sc, *sh, *mu, *rs, *nbt;
};
struct BnBwdBufs {
  DevBuf y, dy, par, part, srcp[YS_BNRED_MAXSEG];
  PadView dz, rg;
  int nblk = 0;
  size_t npart = 0;
  float *sc, *sh, *mu, *rs, *dg, *db, *k2, *k3;
};
}  // namespace

extern "C" int ys_bn_train_fwd(ys_ctx* ctx, int dtype, int mode, int act, int n, ys_bn_fwd_case* cases) {
  YS_REQUIRE(ctx && cases, "ys_bn_train_fwd: null argument");
  YS_REQUIRE(dtype == YS_F32 || dtype == YS_BF16, "ys_bn_train_fwd: bad dtype %d", dtype);
  YS_REQUIRE(mode >= 0 && mode <= 2 && n >= 1 && (mode == 2 || n == 1), "ys_bn_train_fwd: mode %d with %d problems", mode, n);
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int epl = ys_epl(dtype);
  if (n > YS_EW_GROUP_MAX) {                  // the grouped launcher's own refusal, before anything is staged
    std::vector<BnFinProb> none((size_t)n);
    return ys_bn_finalize_group_launch(st, none.data(), n, 1e-3f, 0.03f);
  }
  for (int i = 0; i < n; i++) {
    const ys_bn_fwd_case& c = cases[i];
    YS_REQUIRE(c.y && c.gamma && c.beta && c.run_mean && c.run_var && c.z && c.coef, "ys_bn_train_fwd: problem %d: null argument", i);
    YS_REQUIRE(c.rows >= 1 && c.C >= epl && c.C % epl == 0, "ys_bn_train_fwd: problem %d: rows=%d C=%d (C must be a multiple of %d)", i, c.rows, c.C, epl);
    const std::string who = "ys_bn_train_fwd: problem " + std::to_string(i);
    YS_TRY(z_res_args(who.c_str(), dtype, c.C, c.res, c.res_pad, c.res_coff, c.z_pad, c.z_coff, c.res_shares_z));
    YS_REQUIRE(mode != 1 || (c.partial && c.P >= 1), "ys_bn_train_fwd: mode 1 needs partial rows");
    // ys_chan_stats_launch's limit (one workgroup row holds every vector of a pixel), checked here so that nothing is staged or launched first
    if (mode != 1 && c.C / epl > kEwMaxVec) { ys_set_error("chan_stats: unsupported channel count %d", c.C); return YS_ERR_UNSUPPORTED; }
  }
  BnFwdBufs bufs[YS_EW_GROUP_MAX];
  for (int i = 0; i < n; i++) {
    ys_bn_fwd_case& c = cases[i];
    BnFwdBufs& b = bufs[i];
    const int C = c.C; const long rows = c.rows;
    const size_t cb = (size_t)C * 4;
    YS_TRY(stage_z_res(st, dtype, rows, C, c.res, c.res_pad, c.res_coff, c.z_pad, c.z_coff, c.res_shares_z, b.z, b.res));
    YS_TRY(stage_dense(st, dtype, c.y, rows, C, b.y));
    YS_TRY(b.par.alloc(9 * cb));
    float* par = (float*)b.par.p;
    b.g = par; b.bt = par + C; b.rm = par + 2 * C; b.rv = par + 3 * C; b.sc = par + 4 * C; b.sh = par + 5 * C; b.mu = par + 6 * C; b.rs = par + 7 * C;
    b.nbt = c.nbt ? par + 8 * C : nullptr;
    YS_CHECK_HIP(hipMemsetAsync(par, 0, 9 * cb, st));
    YS_TRY(h2d(st, b.g, c.gamma, cb)); YS_TRY(h2d(st, b.bt, c.beta, cb));
    YS_TRY(h2d(st, b.rm, c.run_mean, cb)); YS_TRY(h2d(st, b.rv, c.run_var, cb));
    if (c.nbt) YS_TRY(h2d(st, b.nbt, c.nbt, 4));
    if (mode == 1) {
      const size_t accb = (size_t)YS_STAT_SHARDS * C * 2 * sizeof(unsigned long long), np = (size_t)c.P * 2 * C;
      YS_TRY(b.part.alloc(np * 4));
      YS_TRY(h2d(st, b.part.p, c.partial, np * 4));
      YS_TRY(alloc_filled(b.acc, accb + kGuardFloats * 4, st));
      YS_CHECK_HIP(hipMemsetAsync(b.acc.p, 0, accb, st));
      const float* rows_p = (const float*)b.part.p;        // plain values: the interpreter build's launch captures its arguments by copy
      unsigned long long* acc_p = (unsigned long long*)b.acc.p;
      const int P = c.P;
      YS_LAUNCH(stat_acc_push_kernel, ys_cdiv((long)np, 256), 256, st, rows_p, P, C, acc_p);
      BnAccFin f{};
      f.acc = (const unsigned long long*)b.acc.p; f.count = (double)rows;
      f.gamma = b.g; f.beta = b.bt; f.run_mean = b.rm; f.run_var = b.rv; f.nbt = b.nbt;
      f.scale = b.sc; f.shift = b.sh; f.mean = b.mu; f.rstd = b.rs; f.eps = 1e-3f; f.momentum = 0.03f;
      YS_TRY(ys_bn_fin_apply_launch(st, dtype, b.y.p, rows, C, f, act, b.res.p, b.res.ld, c.res_coff, b.z.p, b.z.ld, c.z_coff));
    } else {
      b.npart = (size_t)ys_colsum_blocks(rows, C, dtype) * 2 * C;
      YS_TRY(alloc_filled(b.part, (b.npart + kGuardFloats) * 4, st));
      YS_TRY(ys_chan_stats_launch(st, dtype, b.y.p, rows, C, (float*)b.part.p, &b.nblk));
      YS_REQUIRE((size_t)b.nblk * 2 * C == b.npart, "ys_bn_train_fwd: the launcher wrote %d partial rows, %zu were reserved", b.nblk, b.npart / (2 * (size_t)C));
      if (mode == 0) {
        YS_TRY(ys_bn_finalize_launch(st, (const float*)b.part.p, b.nblk, C, rows, b.g, b.bt, 1e-3f, 0.03f, b.rm, b.rv, b.nbt, b.sc, b.sh, b.mu, b.rs));
        YS_TRY(ys_bn_act_apply_launch(st, dtype, b.y.p, rows, C, b.sc, b.sh, act, b.res.p, b.res.ld, c.res_coff, b.z.p, b.z.ld, c.z_coff));
      }
    }
  }
  if (mode == 2) {
    BnFinProb fp[YS_EW_GROUP_MAX]; BnApplyProb ap[YS_EW_GROUP_MAX];
    for (int i = 0; i < n; i++) {
      const BnFwdBufs& b = bufs[i];
      fp[i] = BnFinProb{(const float*)b.part.p, b.nblk, cases[i].C, (double)cases[i].rows, b.g, b.bt, b.rm, b.rv, b.nbt, b.sc, b.sh, b.mu, b.rs};
      ap[i] = BnApplyProb{b.y.p, (long)cases[i].rows, cases[i].C, b.sc, b.sh, b.res.p, b.res.ld, cases[i].res_coff, b.z.p, b.z.ld, cases[i].z_coff};
    }
    YS_TRY(ys_bn_finalize_group_launch(st, fp, n, 1e-3f, 0.03f));
    YS_TRY(ys_bn_act_apply_group_launch(st, dtype, ap, n, act));
  }
  for (int i = 0; i < n; i++) {
    ys_bn_fwd_case& c = cases[i];
    BnFwdBufs& b = bufs[i];
    const size_t cb = (size_t)c.C * 4, accb = (size_t)YS_STAT_SHARDS * c.C * 2 * sizeof(unsigned long long);
    YS_TRY(b.z.fetch(st, c.z));
    YS_TRY(d2h(st, c.coef, b.sc, 4 * cb));
    YS_TRY(d2h(st, c.run_mean, b.rm, cb)); YS_TRY(d2h(st, c.run_var, b.rv, cb));
    if (c.nbt) YS_TRY(d2h(st, c.nbt, b.nbt, 4));
    c.nblk = b.nblk;
    if (c.part_out && mode != 1) YS_TRY(d2h(st, c.part_out, b.part.p, b.npart * 4));
    if (c.acc_out && mode == 1) YS_TRY(d2h(st, c.acc_out, b.acc.p, accb));
    int ok = 1;
    YS_TRY(check_z_res(st, b.z, b.res, &ok));
    if (mode == 1) YS_TRY(check_guard(st, b.acc.p, accb, &ok));
    else YS_TRY(check_guard(st, b.part.p, b.npart * 4, &ok));
    YS_CHECK_HIP(hipStreamSynchronize(st));
    c.view_intact = ok;
  }
  YS_CHECK_HIP(hipGetLastError());
  return YS_OK;
}

extern "C" int ys_bn_train_bwd(ys_ctx* ctx, int dtype, int mode, int act, int n, ys_bn_bwd_case* cases) {
  YS_REQUIRE(ctx && cases, "ys_bn_train_bwd: null argument");
  YS_REQUIRE(dtype == YS_F32 || dtype == YS_BF16, "ys_bn_train_bwd: bad dtype %d", dtype);
  YS_REQUIRE(mode >= 0 && mode <= 3 && n >= 1 && (mode == 2 || n == 1), "ys_bn_train_bwd: mode %d with %d problems", mode, n);
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int epl = ys_epl(dtype);
  const size_t es = ys_es(dtype);
  if (n > YS_EW_GROUP_MAX) {
    std::vector<ChanFinProb> none((size_t)n);
    return ys_bn_bwd_finalize_group_launch(st, none.data(), n);
  }
  for (int i = 0; i < n; i++) {
    const ys_bn_bwd_case& c = cases[i];
    YS_REQUIRE(c.coef && c.dgamma && c.dbeta && c.k23, "ys_bn_train_bwd: problem %d: null argument", i);
    YS_REQUIRE(c.rows >= 1 && c.C >= epl && c.C % epl == 0, "ys_bn_train_bwd: problem %d: rows=%d C=%d (C must be a multiple of %d)", i, c.rows, c.C, epl);
    if (mode == 3) {
      YS_REQUIRE(c.nsrc >= 1 && c.nsrc <= YS_BNRED_MAXSEG, "ys_bn_train_bwd: %d partial-row sources", c.nsrc);
      for (int k = 0; k < c.nsrc; k++) YS_REQUIRE(c.src_part[k] && c.src_nblk[k] >= 1, "ys_bn_train_bwd: source %d is empty", k);
      continue;
    }
    YS_REQUIRE(c.dz && c.y && c.dy, "ys_bn_train_bwd: problem %d: null argument", i);
    YS_TRY(view_on_grid("ys_bn_train_bwd dz", dtype, c.C, c.dz_coff + c.C + c.dz_pad, c.dz_coff));
    if (c.rg) YS_TRY(view_on_grid("ys_bn_train_bwd rg", dtype, c.C, c.rg_coff + c.C + c.rg_pad, c.rg_coff));
    if (c.C / epl > kEwMaxVec) { ys_set_error("bn_bwd: unsupported channel count %d", c.C); return YS_ERR_UNSUPPORTED; }   // ys_bn_bwd_reduce_launch's limit, before anything is staged
  }
  BnBwdBufs bufs[YS_EW_GROUP_MAX];
  for (int i = 0; i < n; i++) {
    ys_bn_bwd_case& c = cases[i];
    BnBwdBufs& b = bufs[i];
    const int C = c.C; const long rows = c.rows;
    const size_t cb = (size_t)C * 4;
    YS_TRY(b.par.alloc(8 * cb));
    float* par = (float*)b.par.p;
    b.sc = par; b.sh = par + C; b.mu = par + 2 * C; b.rs = par + 3 * C; b.dg = par + 4 * C; b.db = par + 5 * C; b.k2 = par + 6 * C; b.k3 = par + 7 * C;
    YS_CHECK_HIP(hipMemsetAsync(par, kSentinelByte, 8 * cb, st));        // k2 / k3 start as the sentinel: an unwritten coefficient shows
    YS_TRY(h2d(st, b.sc, c.coef, 4 * cb));
    YS_TRY(h2d(st, b.dg, c.dgamma, cb)); YS_TRY(h2d(st, b.db, c.dbeta, cb));
    if (mode == 3) {
      FinSrc src{};
      src.n = c.nsrc;
      for (int k = 0; k < c.nsrc; k++) {
        const size_t nb = (size_t)c.src_nblk[k] * 2 * cb;
        YS_TRY(b.srcp[k].alloc(nb));
        YS_TRY(h2d(st, b.srcp[k].p, c.src_part[k], nb));
        src.p[k] = (const float*)b.srcp[k].p; src.nblk[k] = c.src_nblk[k]; src.c1[k] = c.src_c1[k];
      }
      YS_TRY(ys_bn_bwd_finalize_src_launch(st, src, C, rows, b.dg, b.db, b.k2, b.k3, b.sc, b.mu, b.rs));
      continue;
    }
    YS_TRY(b.dz.alloc(st, dtype, rows, C, c.dz_coff + C + c.dz_pad, c.dz_coff));
    YS_TRY(b.dz.stage(st, c.dz));
    YS_TRY(stage_dense(st, dtype, c.y, rows, C, b.y));
    if (c.rg) {
      YS_TRY(b.rg.alloc(st, dtype, rows, C, c.rg_coff + C + c.rg_pad, c.rg_coff));
      YS_TRY(b.rg.stage(st, c.rg));
    }
    YS_TRY(alloc_filled(b.dy, (size_t)rows * C * es + kGuardFloats * 4, st));
    b.npart = (size_t)ys_colsum_blocks(rows, C, dtype) * 2 * C;
    YS_TRY(alloc_filled(b.part, (b.npart + kGuardFloats) * 4, st));
    YS_TRY(ys_bn_bwd_reduce_launch(st, dtype, b.dz.p, b.dz.ld, c.dz_coff, b.y.p, rows, C, b.sc, b.sh, b.mu, b.rs, act, mode == 0 ? b.rg.p : nullptr, b.rg.ld, c.rg_coff,
                                   (float*)b.part.p, &b.nblk));
    YS_REQUIRE((size_t)b.nblk * 2 * C == b.npart, "ys_bn_train_bwd: the launcher wrote %d partial rows, %zu were reserved", b.nblk, b.npart / (2 * (size_t)C));
    if (mode == 2) continue;
    YS_TRY(ys_bn_bwd_finalize_launch(st, (const float*)b.part.p, b.nblk, C, rows, b.dg, b.db, b.k2, b.k3, b.sc, b.mu, b.rs));
    YS_TRY(ys_bn_bwd_apply_launch(st, dtype, b.dz.p, b.dz.ld, c.dz_coff, b.y.p, rows, C, b.sc, b.sh, b.k2, b.k3, act, b.dy.p, nullptr, mode == 1 ? b.rg.p : nullptr,
                                  b.rg.ld, c.rg_coff));
  }
  if (mode == 2) {
    ChanFinProb fp[YS_EW_GROUP_MAX]; BnBwdProb bp[YS_EW_GROUP_MAX];
    for (int i = 0; i < n; i++) {
      const BnBwdBufs& b = bufs[i];
      FinSrc src{}; src.n = 1; src.p[0] = (const float*)b.part.p; src.nblk[0] = b.nblk; src.c1[0] = cases[i].C;
      fp[i] = ChanFinProb{src, cases[i].C, (double)cases[i].rows, b.dg, b.db, b.k2, b.k3, b.sc, b.mu, b.rs};
      bp[i] = BnBwdProb{b.dz.p, b.dz.ld, cases[i].dz_coff, b.y.p, (long)cases[i].rows, cases[i].C, b.sc, b.sh, b.k2, b.k3, b.dy.p, b.rg.p, b.rg.ld, cases[i].rg_coff};
    }
    YS_TRY(ys_bn_bwd_finalize_group_launch(st, fp, n));
    YS_TRY(ys_bn_bwd_apply_group_launch(st, dtype, bp, n, act));
  }
  for (int i = 0; i < n; i++) {
    ys_bn_bwd_case& c = cases[i];
    BnBwdBufs& b = bufs[i];
    const int C = c.C; const long rows = c.rows;
    const size_t cb = (size_t)C * 4;
    YS_TRY(d2h(st, c.dgamma, b.dg, cb)); YS_TRY(d2h(st, c.dbeta, b.db, cb));
    YS_TRY(d2h(st, c.k23, b.k2, 2 * cb));
    int ok = 1;
    if (mode != 3) {
      YS_TRY(fetch_view(st, dtype, b.dy.p, C, 0, 1, C, rows, c.dy));
      if (c.rg) YS_TRY(b.rg.fetch(st, c.rg));
      c.nblk = b.nblk;
      if (c.part_out) YS_TRY(d2h(st, c.part_out, b.part.p, b.npart * 4));
      YS_TRY(b.dz.check(st, &ok));
      if (c.rg) YS_TRY(b.rg.check(st, &ok));
      YS_TRY(check_guard(st, b.part.p, b.npart * 4, &ok));
      YS_TRY(check_guard(st, b.dy.p, (size_t)rows * C * es, &ok));
    }
    YS_CHECK_HIP(hipStreamSynchronize(st));
    c.view_intact = ok;
  }
  YS_CHECK_HIP(hipGetLastError());
  return YS_OK;
}

// grad[C] += column sums of x [B][C][rows_per_b] (chan_reduce_kernel MODE 1 + chan_finalize_kernel MODE 1, the bias gradients): the view starts at channel coff
// of a [B * bstride][coff + Cp + ld_pad] buffer, Cp = C rounded up to the vector width over ZEROED padding channels; images are bstride >= rows_per_b rows apart
// and the rows between them hold the sentinel.
extern "C" int ys_colsum(ys_ctx* ctx, int dtype, const float* x, int B, int C, int rows_per_b, int bstride, int ld_pad, int coff, float* grad,
                         int32_t* view_intact) {
  YS_REQUIRE(ctx && x && grad, "ys_colsum: null argument");
  YS_REQUIRE(dtype == YS_F32 || dtype == YS_BF16, "ys_colsum: bad dtype %d", dtype);
  YS_REQUIRE(B >= 1 && C >= 1 && rows_per_b >= 1 && bstride >= rows_per_b, "ys_colsum: B=%d C=%d rows_per_b=%d bstride=%d", B, C, rows_per_b, bstride);
  const int epl = ys_epl(dtype);
  const size_t es = ys_es(dtype);
  const int Cp = ys_round_up(C, epl), ld = coff + Cp + ld_pad;
  YS_TRY(view_on_grid("ys_colsum", dtype, Cp, ld, coff));
  if (Cp / epl > kEwMaxVec) { ys_set_error("colsum: unsupported channel count %d", C); return YS_ERR_UNSUPPORTED; }    // ys_colsum_launch's limit, before anything is staged
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const long rows = (long)B * rows_per_b, brows = (long)B * bstride;
  DevBuf dx, dpart, dgrad;
  YS_TRY(alloc_filled(dx, (size_t)brows * ld * es, st));
  std::vector<float> hp((size_t)Cp * rows_per_b, 0.f);
  for (int b = 0; b < B; b++) {
    memcpy(hp.data(), x + (size_t)b * C * rows_per_b, (size_t)C * rows_per_b * 4);
    YS_TRY(stage_view(st, dtype, hp.data(), 1, Cp, rows_per_b, (char*)dx.p + (size_t)b * bstride * ld * es, ld, coff));
  }
  const size_t np = (size_t)ys_colsum_blocks(rows, Cp, dtype) * 2 * Cp;
  YS_TRY(alloc_filled(dpart, (np + kGuardFloats) * 4, st));
  YS_TRY(alloc_filled(dgrad, ((size_t)C + kGuardFloats) * 4, st));
  YS_TRY(h2d(st, dgrad.p, grad, (size_t)C * 4));
  YS_TRY(ys_colsum_launch(st, dtype, dx.p, ld, coff, rows, rows_per_b, bstride, C, (float*)dpart.p, (float*)dgrad.p));
  YS_TRY(d2h(st, grad, dgrad.p, (size_t)C * 4));
  int ok = 1;
  YS_TRY(check_guard(st, dpart.p, np * 4, &ok));
  YS_TRY(check_guard(st, dgrad.p, (size_t)C * 4, &ok));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  YS_CHECK_HIP(hipGetLastError());
  if (view_intact) *view_intact = ok;
  return YS_OK;
}

namespace {
// the argument checks ys_upsample2x and ys_copy_view share: both operands in padded views of C channels
int two_view_args(const char* who, ys_ctx* ctx, int dtype, const float* src, const float* dst, int C, int s_ldc, int s_coff, int d_ldc, int d_coff) {
  YS_REQUIRE(ctx && src && dst, "%s: null argument", who);
  YS_REQUIRE(dtype == YS_F32 || dtype == YS_BF16, "%s: bad dtype %d", who, dtype);
  YS_REQUIRE(C >= ys_epl(dtype) && C % ys_epl(dtype) == 0, "%s: C=%d", who, C);
  YS_TRY(view_on_grid(who, dtype, C, s_ldc, s_coff));
  return view_on_grid(who, dtype, C, d_ldc, d_coff);
}
// dst back to the host, both views intact
int two_view_finish(hipStream_t st, const PadView& s, const PadView& d, int B, float* dst, int32_t* view_intact) {
  YS_TRY(d.fetch(st, dst, B));
  int ok = 1;
  YS_TRY(d.check(st, &ok));
  YS_TRY(s.check(st, &ok));
  YS_CHECK_HIP(hipGetLastError());
  if (view_intact) *view_intact = ok;
  return YS_OK;
}
}  // namespace

// Nearest 2x up-sample of src [B][C][H*W] into dst [B][C][4*H*W] (backward = 0), or its gradient: src [B][C][4*H*W] summed 2 x 2 into dst [B][C][H*W]
// (backward = 1; with accumulate != 0 dst holds the gradient already in the buffer and receives dst_in + sum, one rounding).  Both operands in padded views.
extern "C" int ys_upsample2x(ys_ctx* ctx, int dtype, int backward, const float* src, int B, int H, int W, int C, int s_ldc, int s_coff, int d_ldc, int d_coff,
                             int accumulate, float* dst, int32_t* view_intact) {
  YS_TRY(two_view_args("ys_upsample2x", ctx, dtype, src, dst, C, s_ldc, s_coff, d_ldc, d_coff));
  YS_REQUIRE(B >= 1 && H >= 1 && W >= 1, "ys_upsample2x: B=%d H=%d W=%d C=%d", B, H, W, C);
  YS_REQUIRE(!accumulate || backward, "ys_upsample2x: only the backward pass accumulates");
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const long small = (long)H * W, big = 4 * small;
  PadView s, d;
  YS_TRY(s.alloc(st, dtype, B * (backward ? big : small), C, s_ldc, s_coff));
  YS_TRY(d.alloc(st, dtype, B * (backward ? small : big), C, d_ldc, d_coff));
  YS_TRY(s.stage(st, src, B));
  if (accumulate) YS_TRY(d.stage(st, dst, B));
  if (backward) YS_TRY(ys_upsample2x_bwd_launch(st, dtype, s.p, s_ldc, s_coff, B, H, W, C, d.p, d_ldc, d_coff, accumulate ? 1 : 0));
  else YS_TRY(ys_upsample2x_fwd_launch(st, dtype, s.p, s_ldc, s_coff, B, H, W, C, d.p, d_ldc, d_coff));
  return two_view_finish(st, s, d, B, dst, view_intact);
}

// dst view (+)= src view (copy_view_kernel): src, dst [C][rows]; with accumulate != 0 dst holds the destination's content on entry
extern "C" int ys_copy_view(ys_ctx* ctx, int dtype, const float* src, int rows, int C, int s_ldc, int s_coff, int d_ldc, int d_coff, int accumulate, float* dst,
                            int32_t* view_intact) {
  YS_TRY(two_view_args("ys_copy_view", ctx, dtype, src, dst, C, s_ldc, s_coff, d_ldc, d_coff));
  YS_REQUIRE(rows >= 1, "ys_copy_view: rows=%d C=%d", rows, C);
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  PadView s, d;
  YS_TRY(s.alloc(st, dtype, rows, C, s_ldc, s_coff));
  YS_TRY(d.alloc(st, dtype, rows, C, d_ldc, d_coff));
  YS_TRY(s.stage(st, src));
  if (accumulate) YS_TRY(d.stage(st, dst));
  YS_TRY(ys_copy_view_launch(st, dtype, s.p, s_ldc, s_coff, rows, C, d.p, d_ldc, d_coff, accumulate ? 1 : 0));
  return two_view_finish(st, s, d, 1, dst, view_intact);
}

// ---- the quantising BatchNorm passes of the fp8 path
extern "C" int ys_bn_apply_q8_fwd(ys_ctx* ctx, int act, const float* y, int rows, int C, const float* scale, const float* shift, const float* res, int res_pad,
                                  int res_coff, int z_pad, int z_coff, int res_shares_z, float qscale, float* z, uint8_t* q8, float* amax, int32_t* view_intact) {
  YS_REQUIRE(ctx && y && scale && shift && z && q8 && amax, "ys_bn_apply_q8_fwd: null argument");
  YS_REQUIRE(rows >= 1 && C >= 8 && C % 8 == 0, "ys_bn_apply_q8_fwd: rows=%d C=%d (C must be a multiple of 8)", rows, C);
  YS_TRY(z_res_args("ys_bn_apply_q8_fwd", YS_BF16, C, res, res_pad, res_coff, z_pad, z_coff, res_shares_z));
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int dtype = YS_BF16;
  const size_t n = (size_t)rows * C;
  DevBuf dy, dpar, dq, ds, dsc;
  PadView vz, vr;
  YS_TRY(stage_z_res(st, dtype, rows, C, res, res_pad, res_coff, z_pad, z_coff, res_shares_z, vz, vr));
  YS_TRY(stage_dense(st, dtype, y, rows, C, dy));
  YS_TRY(dpar.alloc((size_t)2 * C * 4));
  YS_TRY(h2d(st, dpar.p, scale, (size_t)C * 4)); YS_TRY(h2d(st, (float*)dpar.p + C, shift, (size_t)C * 4));
  YS_TRY(alloc_filled(dq, n + kGuardFloats * 4, st));
  YS_TRY(alloc_slots(ds, st));
  YS_TRY(scalar_to_device(st, dsc, qscale));
  YS_TRY(ys_bn_act_apply_q8_launch(st, dy.p, rows, C, (const float*)dpar.p, (const float*)dpar.p + C, act, vr.p, vr.ld, res_coff, vz.p, vz.ld, z_coff, dq.p,
                                   (const float*)dsc.p, (unsigned*)ds.p));
  YS_TRY(vz.fetch(st, z));
  YS_TRY(d2h(st, q8, dq.p, n));
  int ok = 1;
  YS_TRY(fetch_slots(st, ds, nullptr, amax, &ok));
  YS_TRY(check_guard(st, dq.p, n, &ok));
  YS_TRY(check_z_res(st, vz, vr, &ok));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  YS_CHECK_HIP(hipGetLastError());
  if (view_intact) *view_intact = ok;
  return YS_OK;
}

extern "C" int ys_bn_apply_q8_bwd(ys_ctx* ctx, int act, const float* dz, const float* y, int rows, int C, const float* coef, int dz_pad, int dz_coff, float* rg,
                                  int rg_pad, int rg_coff, float qscale, float* dy, uint8_t* q8, float* amax, int32_t* view_intact) {
  YS_REQUIRE(ctx && dz && y && coef && dy && q8 && amax, "ys_bn_apply_q8_bwd: null argument");
  YS_REQUIRE(rows >= 1 && C >= 8 && C % 8 == 0, "ys_bn_apply_q8_bwd: rows=%d C=%d (C must be a multiple of 8)", rows, C);
  YS_TRY(view_on_grid("ys_bn_apply_q8_bwd dz", YS_BF16, C, dz_coff + C + dz_pad, dz_coff));
  if (rg) YS_TRY(view_on_grid("ys_bn_apply_q8_bwd rg", YS_BF16, C, rg_coff + C + rg_pad, rg_coff));
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int dtype = YS_BF16;
  const size_t n = (size_t)rows * C;
  DevBuf dyb, ddy, dpar, dq, ds, dsc;
  PadView vdz, vrg;
  YS_TRY(vdz.alloc(st, dtype, rows, C, dz_coff + C + dz_pad, dz_coff));
  YS_TRY(vdz.stage(st, dz));
  YS_TRY(stage_dense(st, dtype, y, rows, C, dyb));
  if (rg) {
    YS_TRY(vrg.alloc(st, dtype, rows, C, rg_coff + C + rg_pad, rg_coff));
    YS_TRY(vrg.stage(st, rg));
  }
  YS_TRY(alloc_filled(ddy, n * 2 + kGuardFloats * 4, st));
  YS_TRY(dpar.alloc((size_t)4 * C * 4));
  YS_TRY(h2d(st, dpar.p, coef, (size_t)4 * C * 4));
  const float* par = (const float*)dpar.p;
  YS_TRY(alloc_filled(dq, n + kGuardFloats * 4, st));
  YS_TRY(alloc_slots(ds, st));
  YS_TRY(scalar_to_device(st, dsc, qscale));
  YS_TRY(ys_bn_bwd_apply_q8_launch(st, vdz.p, vdz.ld, dz_coff, dyb.p, rows, C, par, par + C, par + 2 * C, par + 3 * C, act, ddy.p, dq.p, (const float*)dsc.p,
                                   (unsigned*)ds.p, vrg.p, vrg.ld, rg_coff));
  YS_TRY(fetch_view(st, dtype, ddy.p, C, 0, 1, C, rows, dy));
  if (rg) YS_TRY(vrg.fetch(st, rg));
  YS_TRY(d2h(st, q8, dq.p, n));
  int ok = 1;
  YS_TRY(fetch_slots(st, ds, nullptr, amax, &ok));
  YS_TRY(check_guard(st, dq.p, n, &ok));
  YS_TRY(check_guard(st, ddy.p, n * 2, &ok));
  YS_TRY(vdz.check(st, &ok));
  if (rg) YS_TRY(vrg.check(st, &ok));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  YS_CHECK_HIP(hipGetLastError());
  if (view_intact) *view_intact = ok;
  return YS_OK;
}
