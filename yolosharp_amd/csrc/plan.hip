// plan.hip -- everything a model handle decides before its first step (the handle: ys_model.h; the graph: graph.hip; the step that follows these plans:
// model.hip): the flat parameter layout and the state_dict listing, the weight shadows and their preparation kernels, every device allocation, the stem
// routing predicates, and the per-batch-size plan of the fused BN-backward reduction.
#include "ys_model.h"
#include <cstring>
#include <algorithm>

namespace ysm {

int dev_alloc(ys_model* m, void** p, size_t bytes, bool zero) {
  if (bytes == 0) bytes = 16;
  hipError_t e = hipMalloc(p, bytes);
  if (e != hipSuccess) { ys_set_error("hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e)); return YS_ERR_OOM; }
  m->allocs.push_back(*p);
  if (zero) { e = hipMemsetAsync(*p, 0, bytes, m->ctx->stream); if (e != hipSuccess) { ys_set_error("hipMemset failed"); return YS_ERR_HIP; } }
  return YS_OK;
}

static void add_tensor(ys_model* m, const std::string& name, int kind, int conv, long off, std::vector<int64_t> shape, bool is_param) {
  TensorRec t; t.name = name; t.kind = kind; t.conv = conv; t.off = off; t.is_param = is_param;
  t.ndim = (int)shape.size(); t.count = 1;
  for (int i = 0; i < t.ndim; i++) { t.shape[i] = shape[i]; t.count *= shape[i]; }
  m->tensors.push_back(t);
}

// ---- parameter layout: [segment][group] contiguous ranges; group rule of YoloBaseTaskModel.cs:144-151 made disjoint:
//      0 = "bias" (conv bias, bn.bias), 1 = conv "weight", 2 = "bn" weight
int layout_params(ys_model* m) {
  long off = 0;
  for (int seg = 0; seg < ys_model::NSEG; seg++)
    for (int grp = 0; grp < 3; grp++) {
      const long start = off;
      for (auto& c : m->convs) {
        if (c.seg != seg) continue;
        if (grp == 0) { if (c.bn) { c.b_off = off; off += c.cout; } else { c.g_off = off; off += c.cout; } }   // bn.bias | conv bias (stored in g_off for plain convs)
        if (grp == 1) { c.w_off = off; off += c.dw ? (long)c.cout * 9 : c.ct ? 4L * c.cout * c.cin : (long)c.cout * c.k * c.k * c.cin; }
        if (grp == 2 && c.bn) { c.g_off = off; off += c.cout; }
      }
      m->seg_group[seg][grp] = {start, off - start};
    }
  m->n_params = off;
  m->n_params_real = off;
  for (auto& c : m->convs)
    if (c.cout_real != c.cout) m->n_params_real -= (long)(c.cout - c.cout_real) * ((long)c.k * c.k * c.cin + (c.bn ? 2 : 1));
  long so = 0;
  for (auto& c : m->convs)
    if (c.bn) { c.rm_off = so; so += c.cout; c.rv_off = so; so += c.cout; c.nbt_off = so; so += 1; }
  m->n_state = so;
  // state_dict listing: parameters in module REGISTRATION order, then buffers (TorchSharp named_parameters + named_buffers)
  std::vector<int> reg2;
  {
    std::vector<int> seen_e;
    std::vector<int> covered(m->convs.size(), 0);
    for (int e : m->reg) {
      if (std::find(seen_e.begin(), seen_e.end(), e) != seen_e.end()) continue;
      seen_e.push_back(e); reg2.push_back(e);
      covered[e & 0xfffff] += 1;
    }
    for (size_t i = 0; i < m->convs.size(); i++) {
      const int want = m->convs[i].members.empty() ? 1 : (int)m->convs[i].members.size();
      if (covered[i] != want) { ys_set_error("internal: registration list covers %d of %d modules of conv %zu (%s)", covered[i], want, i, m->convs[i].name.c_str()); return YS_ERR_STATE; }
    }
  }
  // (module name, first output row, rows) of a registration entry
  auto module_of = [&](int e, std::string& name, int& row0, int& rows) {
    const ConvL& c = m->convs[e & 0xfffff];
    if (c.members.empty()) { name = c.name; row0 = 0; rows = c.cout_real; }
    else { const ConvL::Member& mb = c.members[e >> 20]; name = mb.name; row0 = mb.row0; rows = mb.rows; }
  };
  for (int e : reg2) {
    const int i = e & 0xfffff;
    const ConvL& c = m->convs[i];
    std::string nm; int r0, nr;
    module_of(e, nm, r0, nr);
    const long wrow = c.dw ? 9 : (long)c.k * c.k * c.cin;
    if (c.bn) {
      if (c.dw) add_tensor(m, nm + ".conv.weight", 4, i, c.w_off, {nr, 1, 3, 3}, true);
      else add_tensor(m, nm + ".conv.weight", 0, i, c.w_off + r0 * wrow, {nr, c.cin, c.k, c.k}, true);
      add_tensor(m, nm + ".bn.weight", 1, i, c.g_off + r0, {nr}, true);
      add_tensor(m, nm + ".bn.bias", 1, i, c.b_off + r0, {nr}, true);
    } else {
      if (c.ct) add_tensor(m, nm + ".weight", 5, i, c.w_off, {c.cin, c.cout, 2, 2}, true);   // ConvTranspose2d: [Cin][Cout][kh][kw]
      else if (c.linear) add_tensor(m, nm + ".weight", 0, i, c.w_off + r0 * wrow, {nr, c.cin}, true);   // nn.Linear: [out, in]
      else add_tensor(m, nm + ".weight", 0, i, c.w_off + r0 * wrow, {nr, c.cin, c.k, c.k}, true);
      add_tensor(m, nm + ".bias", 1, i, c.g_off + r0, {nr}, true);
    }
    if (e == m->dfl_after_conv)
      add_tensor(m, m->head_prefix + ".dfl.conv.weight", 3, -1, 0, {1, m->d.reg_max, 1, 1}, true);   // Block.cs:28-30 (never trained, Head.cs:221)
  }
  for (int e : reg2) {
    const int i = e & 0xfffff;
    const ConvL& c = m->convs[i];
    if (!c.bn) continue;
    std::string nm; int r0, nr;
    module_of(e, nm, r0, nr);
    add_tensor(m, nm + ".bn.running_mean", 2, i, c.rm_off + r0, {nr}, false);
    add_tensor(m, nm + ".bn.running_var", 2, i, c.rv_off + r0, {nr}, false);
    add_tensor(m, nm + ".bn.num_batches_tracked", 2, i, c.nbt_off, {1}, false);   // members of a fused unit share the counter: they always step together
  }
  return YS_OK;
}

namespace {
// ---- batched weight preparation: fp32 master [Cout][taps][Cin] -> T forward [Cout][taps][Cin_pad]
//                                                                  -> T dgrad   [Cin][taps flipped][Cout_pad]
template <class T>
__global__ void __launch_bounds__(256)
weight_prep_all_kernel(const float* __restrict__ params, const PrepDesc* __restrict__ desc, int n, long total_f, long total_d,
                       T* __restrict__ wf_all, T* __restrict__ wd_all, const float* __restrict__ amax_w,
                       unsigned char* __restrict__ wf8_all, unsigned char* __restrict__ wd8_all) {
  // fp8 mode: e4m3 copies of both shadows (same element order) with the layer's current scale 448 / amax(|W|)
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total_f) {
    int lo = 0, hi = n - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (desc[mid].nf_start <= i) lo = mid; else hi = mid - 1; }
    const PrepDesc d = desc[lo];
    const long e = i - d.nf_start;
    const int ci = (int)(e % d.cin_pad);
    const long r = e / d.cin_pad;
    const T tv = Elem<T>::from_f(ci < d.cin_real ? params[d.w_off + r * d.cin_real + ci] : 0.f);
    wf_all[d.wf_off + e] = tv;
    if (wf8_all) { const float aw = amax_w[lo]; wf8_all[d.wf_off + e] = ys_f32_to_e4m3_dev(Elem<T>::to_f(tv) * (aw > 0.f ? YS_E4M3_MAX / aw : 1.0f)); }
  }
  if (i < total_d) {
    int lo = 0, hi = n - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (desc[mid].nd_start <= i) lo = mid; else hi = mid - 1; }
    const PrepDesc d = desc[lo];
    if (d.has_wd) {
      const long e = i - d.nd_start;
      int co, ci, tap;
      if (d.phase) {          // stride-2 3x3 layer on the bf16 path: phase-major dgrad weights (conv_dgrad_s2_phases)
        ys_phase_wd_index(e, d.cin_real, d.cout_pad, ci, tap, co);
      } else {
        co = (int)(e % d.cout_pad);
        const long r = e / d.cout_pad;
        const int tapf = (int)(r % d.taps);
        ci = (int)(r / d.taps);
        tap = d.taps - 1 - tapf;
      }
      const T tv = Elem<T>::from_f(co < d.cout && ci < d.cin_real ? params[d.w_off + ((long)co * d.taps + tap) * d.cin_real + ci] : 0.f);
      wd_all[d.wd_off + e] = tv;
      if (wd8_all) { const float aw = amax_w[lo]; wd8_all[d.wd_off + e] = ys_f32_to_e4m3_dev(Elem<T>::to_f(tv) * (aw > 0.f ? YS_E4M3_MAX / aw : 1.0f)); }
    }
  }
}

// Round 5: the bf16 form of the above as three block ranges of ONE launch.  The element-per-thread kernel spent its time in two 8-step binary searches over the
// descriptor table and three 64-bit divisions PER ELEMENT, stored 2 bytes per lane, and read the master weights of the dgrad shadow with a stride of taps * Cin floats
// between neighbouring lanes: 48 us per YOLOv8n step, 1.11 ms per YOLOv8x step -- a tenth of the HBM rate for a pass that moves 8 bytes per parameter.
//   blocks [0, nbF):        forward shadow, 8 consecutive elements per thread (one search, 32-bit index arithmetic, two 16-byte loads, one 16-byte store)
//   blocks [nbF, nbF+nbT):  dgrad shadow of the plain layers as 64 (cout) x 64 (cin) tiles of one tap through LDS: rows of 256 B read along cin, rows of 128 B written along cout
//   blocks [nbF+nbT, ...):  dgrad shadow of the stride-2 layers (phase-major order, conv_dgrad_s2_phases): the element form, on their own compact table
// Same values as weight_prep_all_kernel<bf16_t> element for element (round-to-nearest-even; e4m3 copies from the ROUNDED bf16 value).
__global__ void __launch_bounds__(256)
weight_prep_fast_kernel(const float* __restrict__ params, const PrepDesc* __restrict__ desc, int n, long total_f8,
                        const PrepDesc* __restrict__ tdesc, int nt, long nbF, long nbT,
                        const PrepDesc* __restrict__ pdesc, int np, long total_p,
                        bf16_t* __restrict__ wf_all, bf16_t* __restrict__ wd_all, const float* __restrict__ amax_w,
                        unsigned char* __restrict__ wf8_all, unsigned char* __restrict__ wd8_all) {
  __shared__ float sT[64][65];
  const long blk = blockIdx.x;
  const int tid = threadIdx.x;
  if (blk < nbF) {
    const long u = blk * 256 + tid;            // 8-element unit
    if (u >= total_f8) return;
    const long i = u * 8;
    int lo = 0, hi = n - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (desc[mid].nf_start <= i) lo = mid; else hi = mid - 1; }
    const PrepDesc d = desc[lo];
    const unsigned e = (unsigned)(i - d.nf_start);
    const unsigned r = e / (unsigned)d.cin_pad, ci = e - r * (unsigned)d.cin_pad;     // cin_pad is a multiple of 8: the unit stays inside one row
    const long src = d.w_off + (long)r * d.cin_real + ci;
    float f[8];
    if ((int)ci + 8 <= d.cin_real && (src & 3) == 0) {
      const float4 a = *(const float4*)(params + src), b = *(const float4*)(params + src + 4);
      f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
    } else {
#pragma unroll
      for (int k = 0; k < 8; k++) f[k] = (int)ci + k < d.cin_real ? params[src + k] : 0.f;
    }
    const uint4 pk = ys_pack<bf16_t>(f);
    *(uint4*)(wf_all + d.wf_off + e) = pk;
    if (wf8_all) {
      const float aw = amax_w[lo], sc = aw > 0.f ? YS_E4M3_MAX / aw : 1.0f;
      float g[8];
      ys_unpack<bf16_t>(pk, g);
      unsigned w0 = 0, w1 = 0;
#pragma unroll
      for (int k = 0; k < 4; k++) { w0 |= (unsigned)ys_f32_to_e4m3_dev(g[k] * sc) << (8 * k); w1 |= (unsigned)ys_f32_to_e4m3_dev(g[4 + k] * sc) << (8 * k); }
      *(uint2*)(wf8_all + d.wf_off + e) = make_uint2(w0, w1);
    }
    return;
  }
  if (blk < nbF + nbT) {
    const long t = blk - nbF;
    int lo = 0, hi = nt - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (tdesc[mid].tile_start <= t) lo = mid; else hi = mid - 1; }
    const PrepDesc d = tdesc[lo];
    const int tl = (int)(t - d.tile_start);
    const int per_tap = d.tiles_ci * d.tiles_co;
    const int tapf = tl / per_tap, rem = tl - tapf * per_tap;
    const int tci = rem / d.tiles_co, tco = rem - tci * d.tiles_co;
    const int tap = d.taps - 1 - tapf;                 // spatial flip of a square kernel
    const int co0 = tco * 64, ci0 = tci * 64;
    // load: thread -> (row = tid / 16 + 16 rr, 4 consecutive cin)
    const int lr = tid >> 4, lc = (tid & 15) * 4;
#pragma unroll
    for (int rr = 0; rr < 4; rr++) {
      const int co = co0 + lr + 16 * rr, ci = ci0 + lc;
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (co < d.cout && ci < d.cin_real) {
        const long src = d.w_off + ((long)co * d.taps + tap) * d.cin_real + ci;
        if (ci + 4 <= d.cin_real && (src & 3) == 0) { const float4 a = *(const float4*)(params + src); v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; }
        else {
#pragma unroll
          for (int k = 0; k < 4; k++) if (ci + k < d.cin_real) v[k] = params[src + k];
        }
      }
#pragma unroll
      for (int k = 0; k < 4; k++) sT[lr + 16 * rr][lc + k] = v[k];
    }
    __syncthreads();
    // store: thread -> (cin row = tid / 4, 16 consecutive cout)
    const int sr = tid >> 2, sc0 = (tid & 3) * 16;
    const int ci = ci0 + sr;
    if (ci < d.cin_pad) {
      const float aw = wd8_all ? amax_w[d.layer] : 0.f, sc = aw > 0.f ? YS_E4M3_MAX / aw : 1.0f;
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int co = co0 + sc0 + 8 * h;
        if (co < d.cout_pad) {                           // cout_pad is a multiple of 8
          float f[8];
#pragma unroll
          for (int k = 0; k < 8; k++) f[k] = sT[sc0 + 8 * h + k][sr];
          const uint4 pk = ys_pack<bf16_t>(f);
          const long dst = d.wd_off + ((long)ci * d.taps + tapf) * d.cout_pad + co;
          *(uint4*)(wd_all + dst) = pk;
          if (wd8_all) {
            float g[8];
            ys_unpack<bf16_t>(pk, g);
            unsigned w0 = 0, w1 = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) { w0 |= (unsigned)ys_f32_to_e4m3_dev(g[k] * sc) << (8 * k); w1 |= (unsigned)ys_f32_to_e4m3_dev(g[4 + k] * sc) << (8 * k); }
            *(uint2*)(wd8_all + dst) = make_uint2(w0, w1);
          }
        }
      }
    }
    return;
  }
  {
    const long i = (blk - nbF - nbT) * 256 + tid;
    if (i >= total_p) return;
    int lo = 0, hi = np - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (pdesc[mid].nd_start <= i) lo = mid; else hi = mid - 1; }
    const PrepDesc d = pdesc[lo];
    const long e = i - d.nd_start;
    int co, ci, tap;
    ys_phase_wd_index(e, d.cin_real, d.cout_pad, ci, tap, co);
    const bf16_t tv = Elem<bf16_t>::from_f(co < d.cout && ci < d.cin_real ? params[d.w_off + ((long)co * d.taps + tap) * d.cin_real + ci] : 0.f);
    wd_all[d.wd_off + e] = tv;
    if (wd8_all) { const float aw = amax_w[d.layer]; wd8_all[d.wd_off + e] = ys_f32_to_e4m3_dev(Elem<bf16_t>::to_f(tv) * (aw > 0.f ? YS_E4M3_MAX / aw : 1.0f)); }
  }
}
}  // namespace

int prep_weights(ys_model* m) {
  if (!m->weights_dirty) return YS_OK;
  const long total = std::max(m->prep_nf, m->prep_nd);
  if (m->f8) YS_TRY(ys_f8_weight_amax_launch(m->ctx->stream, m->params, m->f8_layers, m->n_prep, m->amax_w));
  if (m->dtype == YS_BF16 && m->prep_fast) {
    const long nbF = ys_cdiv(m->prep_nf / 8, 256), nbT = m->prep_tiles, nbP = ys_cdiv(m->prep_nd_phase, 256);
    YS_LAUNCH(weight_prep_fast_kernel, (unsigned)(nbF + nbT + nbP), 256, m->ctx->stream, (const float*)m->params, (const PrepDesc*)m->prep_dev, m->n_prep, m->prep_nf / 8,
              (const PrepDesc*)m->prep_tile_dev, m->n_prep_tile, nbF, nbT, (const PrepDesc*)m->prep_phase_dev, m->n_prep_phase, m->prep_nd_phase,
              (bf16_t*)m->wf_all, (bf16_t*)m->wd_all, (const float*)m->amax_w, m->wf8_all, m->wd8_all);
  } else if (m->dtype == YS_BF16)
    YS_LAUNCH((weight_prep_all_kernel<bf16_t>), ys_cdiv(total, 256), 256, m->ctx->stream, (const float*)m->params, (const PrepDesc*)m->prep_dev, m->n_prep, m->prep_nf, m->prep_nd, (bf16_t*)m->wf_all, (bf16_t*)m->wd_all, (const float*)m->amax_w, m->wf8_all, m->wd8_all);
  else
    YS_LAUNCH((weight_prep_all_kernel<float>), ys_cdiv(total, 256), 256, m->ctx->stream, (const float*)m->params, (const PrepDesc*)m->prep_dev, m->n_prep, m->prep_nf, m->prep_nd, (float*)m->wf_all, (float*)m->wd_all, (const float*)nullptr, (unsigned char*)nullptr, (unsigned char*)nullptr);
  m->weights_dirty = false;
  return YS_OK;
}

static void dev_free_tracked(ys_model* m, void* p) {
  if (!p) return;
  for (size_t i = 0; i < m->allocs.size(); i++) if (m->allocs[i] == p) { m->allocs.erase(m->allocs.begin() + i); break; }
  hipFree(p);
}

// Ground-truth workspace for `gcap` labels PER IMAGE (the reference pads every image to the batch's largest label count,
// Loss.cs:363-390, without a cap): raw label staging, padded GT arrays and the [B][gcap][A] assignment matrices.
int alloc_label_ws(ys_model* m, int gcap) {
  const int B = m->maxB;
  void* old[] = {m->lab_bidx, m->lab_cls, m->lab_box, m->gt_count, m->gt_box, m->gt_cls, m->ov, m->align, m->mpos, m->pos_align, m->pos_ov, m->kp_dev};
  if (m->lab_bidx) YS_CHECK_HIP(hipStreamSynchronize(m->ctx->stream));
  for (void* p : old) dev_free_tracked(m, p);
  m->lab_bidx = m->lab_cls = m->lab_box = nullptr; m->gt_count = nullptr; m->gt_box = nullptr; m->gt_cls = nullptr;
  m->ov = m->align = nullptr; m->mpos = nullptr; m->pos_align = m->pos_ov = nullptr; m->kp_dev = nullptr;
  m->gcap = gcap;
  m->max_labels = gcap * B;
  const size_t GA = (size_t)B * gcap * m->A;
  YS_TRY(dev_alloc(m, (void**)&m->lab_bidx, (size_t)m->max_labels * 4));
  YS_TRY(dev_alloc(m, (void**)&m->lab_cls, (size_t)m->max_labels * 4));
  YS_TRY(dev_alloc(m, (void**)&m->lab_box, (size_t)m->max_labels * 20));   // 4 floats per label, 5 for oriented boxes
  YS_TRY(dev_alloc(m, (void**)&m->gt_count, (size_t)B * 4));
  YS_TRY(dev_alloc(m, (void**)&m->gt_box, (size_t)B * gcap * 20));        // xyxy, or xywh + angle (OBB)
  YS_TRY(dev_alloc(m, (void**)&m->gt_cls, (size_t)B * gcap * 12));  // gt_cls + gt_valid + gt_src
  YS_TRY(dev_alloc(m, (void**)&m->ov, GA * 4));
  YS_TRY(dev_alloc(m, (void**)&m->align, GA * 4));
  YS_TRY(dev_alloc(m, (void**)&m->mpos, GA));
  YS_TRY(dev_alloc(m, (void**)&m->pos_align, (size_t)B * gcap * 4));
  YS_TRY(dev_alloc(m, (void**)&m->pos_ov, (size_t)B * gcap * 4));
  if (m->xkind == 3) YS_TRY(dev_alloc(m, (void**)&m->kp_dev, (size_t)m->max_labels * m->nm * 4));
  return YS_OK;
}

// fp8 mode: which convolutions may run the fp8 kernel, the e4m3 weight shadows and the amax / scale slots (recipe: f8.hip)
static int alloc_f8(ys_model* m, const std::vector<PrepDesc>& pd) {
  hipStream_t st = m->ctx->stream;
  std::vector<F8Layer> layers(pd.size());
  for (size_t i = 0; i < pd.size(); i++) { layers[i].w_off = pd[i].w_off; layers[i].count = (long)pd[i].cout * pd[i].taps * pd[i].cin_real; }
  std::vector<F8Conv> fc(m->convs.size());
  size_t q8_bytes = 0;
  for (auto& c : m->convs) {
    F8Conv& f = fc[c.idx];
    f.layer = c.prep_idx >= 0 ? c.prep_idx : 0;
    const bool dense = !c.first && !c.dw && !c.ct && c.bn;       // the plain biased head outputs feed the loss directly: kept in bf16
    c.f8_fwd = dense && c.cin_pad % 32 == 0 && c.cin == c.cin_pad;
    c.f8_bwd = dense && c.cout % 32 == 0 && c.cout_ld == c.cout;
    if (c.f8_fwd) q8_bytes = std::max(q8_bytes, (size_t)m->maxB * c.Hin * c.Win * c.cin_pad);
    if (c.f8_bwd) q8_bytes = std::max(q8_bytes, (size_t)m->maxB * c.Hout * c.Wout * c.cout_ld);
  }
  if (q8_bytes) YS_TRY(dev_alloc(m, (void**)&m->q8, q8_bytes));
  m->n_f8_convs = (int)fc.size();
  YS_TRY(dev_alloc(m, (void**)&m->wf8_all, (size_t)m->n_wf_pending));
  YS_TRY(dev_alloc(m, (void**)&m->wd8_all, (size_t)m->n_wd_pending));
  YS_TRY(dev_alloc(m, (void**)&m->amax_w, pd.size() * 4));
  YS_TRY(dev_alloc(m, (void**)&m->amax_act, fc.size() * YS_AMAX_WAYS * 4));
  YS_TRY(dev_alloc(m, (void**)&m->amax_dy, fc.size() * YS_AMAX_WAYS * 4));
  YS_TRY(dev_alloc(m, (void**)&m->f8_scales, fc.size() * 16));
  YS_TRY(dev_alloc(m, (void**)&m->f8_layers, layers.size() * sizeof(F8Layer)));
  YS_TRY(dev_alloc(m, (void**)&m->f8_convs, fc.size() * sizeof(F8Conv)));
  YS_CHECK_HIP(hipMemcpyAsync(m->f8_layers, layers.data(), layers.size() * sizeof(F8Layer), hipMemcpyHostToDevice, st));
  YS_CHECK_HIP(hipMemcpyAsync(m->f8_convs, fc.data(), fc.size() * sizeof(F8Conv), hipMemcpyHostToDevice, st));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  return YS_OK;
}

// model.0 of a whole-model handle on the bf16 path, when the stem kernels take its shape (conv_stem.hip: 3x3; conv_stem6.hip: Yolov5u's 6x6): what both stem routes ask for
static const ConvL* stem_unit(const ys_model* m) {
  if (!m->stem_on || m->is_block || m->is_head || m->dtype != YS_BF16 || m->convs.empty()) return nullptr;
  const ConvL& c = m->convs[0];
  if (!c.first || !c.bn || c.dw || c.ct || c.has_res || c.in.buf != m->in_buf) return nullptr;
  return (ys_stem_eligible(m->dtype, c.cin, c.cout, c.k, c.s) && c.pad == 1) || ys_stem6_eligible(m->dtype, c.cin, c.cout, c.k, c.s, c.pad) ? &c : nullptr;
}
// ... with its own weight-gradient partial region (deferred split reduction)
bool stem_direct(const ys_model* m) {
  const ConvL* c = stem_unit(m);
  if (!c || c->wgp_off < 0) return false;
  const Buf& ob = m->bufs[c->out.buf];
  return (ob.ldc & 3) == 0 && (c->out.coff & 3) == 0;
}
// model.0's BatchNorm backward can run inside its weight-gradient kernel (conv_stem.hip, FUSE): the unit has no dgrad, so nothing else reads its dy.  Decided at
// creation (no dy buffer is allocated for the unit then); a step whose forward did not read the fp32 image (ys_model_forward_u8) takes the separate pass.
bool stem_bnb_planned(const ys_model* m) {
  const ConvL* c = m->stem_bnb_fuse ? stem_unit(m) : nullptr;
  if (!c || c->k != 3 || c->pool_next || c->cout_ld != c->cout || c->cout != 16) return false;   // 16 channels: the width the fused kernel is built and measured for (conv_stem.hip)
  const Buf& ob = m->bufs[c->out.buf];
  return (ob.ldc & 7) == 0 && (c->out.coff & 7) == 0 && ob.rows_per_b == (long)c->Hout * c->Wout;
}

int allocate(ys_model* m) {
  const int B = m->maxB;
  for (auto& b : m->bufs) {
    const size_t bytes = (size_t)B * b.rows_per_b * b.ldc * m->es;
    YS_TRY(dev_alloc(m, &b.act, bytes));
    if (b.need_grad) YS_TRY(dev_alloc(m, &b.grad, bytes));
  }
  YS_TRY(dev_alloc(m, (void**)&m->params, (size_t)m->n_params * 4));
  YS_TRY(dev_alloc(m, (void**)&m->grads, (size_t)m->n_params * 4));
  YS_TRY(dev_alloc(m, (void**)&m->adam_m, (size_t)m->n_params * 4));
  YS_TRY(dev_alloc(m, (void**)&m->adam_v, (size_t)m->n_params * 4));
  YS_TRY(dev_alloc(m, (void**)&m->state, (size_t)m->n_state * 4));
  long nf = 0, nd = 0, ny = 0, nch = 0, dy_max = 0, stat_max = 0, amax = 0;
  std::vector<PrepDesc> pd;
  for (auto& c : m->convs) {
    const int taps = c.k * c.k;
    if (c.dw) {   // depthwise: fp32 master weights are used directly
      const long M = (long)B * c.Hout * c.Wout;
      c.y_off = ny; ny += M * c.cout;
      c.ch_off = nch; nch += 6L * ((c.cout + 3) / 4 * 4);
      dy_max = std::max(dy_max, M * c.cout_ld);
      stat_max = std::max(stat_max, 2048L * 2 * c.cout_ld);
      stat_max = std::max(stat_max, 1024L * 9 * c.cout);   // depthwise weight-gradient partials (ys_dwconv_wgrad_blocks <= 1024)
      continue;
    }
    c.wf_off = nf;
    c.wd_off = nd;
    c.prep_idx = (int)pd.size();
    for (int ph = 0; ph < (c.ct ? 4 : 1); ph++) {   // ConvTranspose: one 1x1 weight matrix per output phase
      PrepDesc d{}; d.w_off = c.w_off + (long)ph * c.cout * c.cin; d.wf_off = nf; d.wd_off = nd; d.cout = c.cout; d.taps = taps;
      d.cin_real = c.cin; d.cin_pad = c.cin_pad; d.cout_pad = c.cout_ld; d.has_wd = c.first ? 0 : 1;
      d.phase = (!c.ct && ys_conv_dgrad_uses_phases(m->dtype, c.k, c.s)) ? 1 : 0;
      d.nf_start = nf; d.nd_start = nd;
      nf += (long)c.cout * taps * c.cin_pad;
      if (!c.first) nd += (long)c.cin_pad * taps * c.cout_ld;   // cin_pad > cin (Pose towers): zero rows -> zero input-gradient pad channels
      pd.push_back(d);
    }
    const long M = (long)B * c.Hout * c.Wout;
    if (c.bn) { c.y_off = ny; ny += M * c.cout; }
    c.ch_off = nch; nch += 6L * ((c.cout + 3) / 4 * 4);   // 16-byte aligned coefficient vectors
    dy_max = std::max(dy_max, M * c.cout_ld);
    stat_max = std::max(stat_max, 2L * ys_cdiv(M, 64) * 2 * c.cout);   // conv epilogue partials (smallest pixel tile, ragged 2-D tiles)
    stat_max = std::max(stat_max, 2048L * 2 * c.cout_ld);   // channel-reduction partials (<= 2048 workgroups)
  }
  for (auto& op : m->ops) if (op.type == OP_MAXPOOL) { op.aux_off = amax; amax += (long)B * op.H * op.W * op.in.C; }
  long nattn = 0;
  for (auto& op : m->ops) if (op.type == OP_ATTN) { op.aux_off = nattn; nattn += 2L * B * op.heads * (long)(op.H * op.W) * (op.H * op.W); }
  m->n_attn = nattn;
  YS_TRY(dev_alloc(m, (void**)&m->attn_ws, (size_t)nattn * 4));
  m->n_wf = nf; m->n_wd = nd; m->n_y = ny; m->n_chan = nch; m->n_dy = dy_max; m->n_stat = stat_max; m->n_argmax = amax;
  m->prep_nf = nf; m->prep_nd = nd; m->n_prep = (int)pd.size();
  YS_TRY(dev_alloc(m, &m->wf_all, (size_t)nf * m->es));
  YS_TRY(dev_alloc(m, &m->wd_all, (size_t)nd * m->es));
  YS_TRY(dev_alloc(m, (void**)&m->prep_dev, pd.size() * sizeof(PrepDesc)));
  YS_CHECK_HIP(hipMemcpyAsync(m->prep_dev, pd.data(), pd.size() * sizeof(PrepDesc), hipMemcpyHostToDevice, m->ctx->stream));
  {
    // weight_prep_fast_kernel's tables (bf16): the plain layers' transpose tiles and the phase-major layers' elements, each as a compact prefix
    std::vector<PrepDesc> pt, pp;
    long tiles = 0, pe = 0;
    bool ok = m->dtype == YS_BF16;
    for (size_t i = 0; i < pd.size(); i++) {
      PrepDesc d = pd[i];
      d.layer = (int)i;
      if ((d.cin_pad & 7) || (d.cout_pad & 7) || (d.nf_start & 7) || (d.wf_off & 7) || (d.wd_off & 7)) ok = false;
      if (!d.has_wd) continue;
      if (d.phase) { d.nd_start = pe; pe += (long)d.cin_pad * d.taps * d.cout_pad; pp.push_back(d); }
      else {
        d.tiles_ci = ys_cdiv(d.cin_pad, 64); d.tiles_co = ys_cdiv(d.cout_pad, 64); d.tile_start = tiles;
        tiles += (long)d.taps * d.tiles_ci * d.tiles_co; pt.push_back(d);
      }
    }
    if ((nf & 7) || tiles + ys_cdiv(nf / 8, 256) + ys_cdiv(pe, 256) >= (1L << 31)) ok = false;
    m->prep_fast = ok;      // (the element-per-thread kernel stays for fp32 and for tables that miss the 8-element alignment; bit-identity of the two was a round-5 test, profiles/README.md)
    if (m->prep_fast) {
      m->n_prep_tile = (int)pt.size(); m->prep_tiles = tiles; m->n_prep_phase = (int)pp.size(); m->prep_nd_phase = pe;
      if (pt.empty()) pt.push_back(PrepDesc{});
      if (pp.empty()) pp.push_back(PrepDesc{});
      YS_TRY(dev_alloc(m, (void**)&m->prep_tile_dev, pt.size() * sizeof(PrepDesc)));
      YS_TRY(dev_alloc(m, (void**)&m->prep_phase_dev, pp.size() * sizeof(PrepDesc)));
      YS_CHECK_HIP(hipMemcpyAsync(m->prep_tile_dev, pt.data(), pt.size() * sizeof(PrepDesc), hipMemcpyHostToDevice, m->ctx->stream));
      YS_CHECK_HIP(hipMemcpyAsync(m->prep_phase_dev, pp.data(), pp.size() * sizeof(PrepDesc), hipMemcpyHostToDevice, m->ctx->stream));
      YS_CHECK_HIP(hipStreamSynchronize(m->ctx->stream));   // pt / pp are host temporaries
    }
  }
  YS_CHECK_HIP(hipStreamSynchronize(m->ctx->stream));   // pd is a host temporary
  m->n_wf_pending = nf; m->n_wd_pending = nd;
  if (m->f8) YS_TRY(alloc_f8(m, pd));
  YS_TRY(dev_alloc(m, &m->y_all, (size_t)ny * m->es));
  YS_TRY(dev_alloc(m, &m->dy_scratch, (size_t)dy_max * m->es));
  // measured on MI355X (YOLOv8n B=64): +1.4 % step throughput, but both streams' kernels fill the CUs' LDS, so they mostly
  // time-slice and every per-kernel duration inflates; off by default (YS_OVERLAP=1 enables it)
  // Round 3: on by default.  With the split reduction deferred to one launch per segment the weight-gradient kernels are independent
  // of everything until the segment ends, and both chains are latency-bound: measured 10.50 -> 10.30 ms/step (+2 %) on config 2
  // (round 2, before the deferral: +1.4 %).  Co-running kernels time-slice the CUs, so PER-KERNEL durations inflate (conv class +7 %):
  // bench.py switches the overlap off (ys_model_set_overlap) for its per-kernel profile steps.  YS_OVERLAP=0 disables it.
  m->overlap = (YS_OPT_INT("OVERLAP", 1) != 0);
  m->overlap_built = m->overlap;
  m->stem_on = (YS_OPT_INT("STEM_DIRECT", 1) != 0);
  m->stem_bnb_fuse = (YS_OPT_INT("STEM_BNB_FUSE", 1) != 0);   // YS_STEM_BNB_FUSE=0: model.0's BatchNorm backward is a pass of its own (the fused form's reference)
  if (m->overlap) {
    // lowest priority: the weight gradients are off the critical path (the optimizer is their only reader), and a priority class of
    // its own is a hardware queue of its own -- streams of one class share a handful of queues in creation order, and with the main
    // stream and this one on the SAME queue nothing overlaps (seen with an eagerly initialised RCCL communicator, whose streams
    // shifted the assignment: 11.6 instead of 10.2 ms/step).
    {
      int least = 0, greatest = 0;
      if (hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && least != greatest)
        YS_CHECK_HIP(hipStreamCreateWithPriority(&m->st2, hipStreamNonBlocking, least));     // (round 6: the HIGHEST priority instead: 8.61 / 8.61 / 8.63 -> 8.65 / 8.65 / 8.66 ms)
      else
        YS_CHECK_HIP(hipStreamCreateWithFlags(&m->st2, hipStreamNonBlocking));
    }
    // (rounds 3-5: a ring of four dy_max-sized buffers guarded by events; round 6: one buffer per unit, sized for that unit -- sum of the BN outputs, 1.9 GB for
    // YOLOv8n at B = 64, ~10 GB for YOLOv8x at 1280 x 1280 x 16)
    for (auto& c : m->convs) {
      if (!c.bn || c.dw || c.ct || c.dy_own) continue;
      if (c.idx == 0 && stem_bnb_planned(m)) continue;      // its dy is formed inside its weight-gradient kernel
      YS_TRY(dev_alloc(m, &c.dy_own, (size_t)B * c.Hout * c.Wout * c.cout_ld * m->es));
    }
    for (hipEvent_t& ev : m->ev_hand) YS_CHECK_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    YS_CHECK_HIP(hipEventCreateWithFlags(&m->ev_join, hipEventDisableTiming));
  }
  for (int k = 0; k < ys_model::NSEG; k++) {
    YS_CHECK_HIP(hipEventCreateWithFlags(&m->ev_seg_m[k], hipEventDisableTiming));
    YS_CHECK_HIP(hipEventCreateWithFlags(&m->ev_seg_w[k], hipEventDisableTiming));
  }
  {
    // grouped head stages: every unit keeps its own statistics rows (conv -> grouped finalize) and its own dy (BN backward -> wgrad / dgrad)
    long gst = 0;
    for (auto& c : m->convs) {
      if (c.group < 0) continue;
      const long M = (long)B * c.Hout * c.Wout;
      c.gstat_off = gst; gst += (2L * ys_cdiv(M, 64) * 2 * c.cout_ld + 63) / 64 * 64;
      if (c.bn && !c.dy_own) YS_TRY(dev_alloc(m, &c.dy_own, (size_t)M * c.cout_ld * m->es));
    }
    if (gst) YS_TRY(dev_alloc(m, (void**)&m->stat_group, (size_t)gst * 4));
  }
  YS_TRY(dev_alloc(m, (void**)&m->chan, (size_t)nch * 4));
  YS_TRY(dev_alloc(m, (void**)&m->stat_partial, (size_t)stat_max * 4));
  // statistics accumulators of the BatchNorm units (round 5, ys_kernels.h ys_stat_acc_add).  Off in fp8 mode (its apply pass also writes the e4m3 image)
  // and by BN_ATOMIC=0 (A/B switch against the row + bn_finalize form)
  m->bn_atomic = YS_OPT_INT("BN_ATOMIC", 1) != 0 && !m->f8;
  if (m->bn_atomic) {
    long off = 0;
    for (auto& c : m->convs) if (c.bn && !c.dw && !c.ct) { c.acc_off = off; off += (long)YS_STAT_SHARDS * c.cout * 2; }
    m->n_stat_acc = off;
    if (off > 0) YS_TRY(dev_alloc(m, (void**)&m->stat_acc_all, (size_t)off * 8));
    else m->bn_atomic = false;
  }
  // (BN-backward sums through exact integer accumulators + a finalize inside the apply pass -- BNB_ATOMIC, round 5: identical results, 51 launches fewer, NOT faster
  // (8.94-8.97 against 8.83-8.94 ms) -- was deleted in round 6; the record is in profiles/README.md round 5.)
  // (Two experiments lived here through round 4 and are gone: side-stream "head lanes" for the P4 / P5 towers -- 10.52-10.55 ms/step against 9.98-10.01 without,
  // a side-stream kernel that takes CU slots turns the persistent P3 kernels' equal tile shares into a tail -- and the last-arriver "ticket" BatchNorm finalize inside
  // the producing convolution, +0.9 ms/step: DESIGN.md 6b / 6d.)
  YS_TRY(dev_alloc(m, (void**)&m->argmax, (size_t)amax));
  // wgrad partial workspace: a shared scratch (max over layers of splits * |W|: ConvTranspose phases, immediate reduction) followed by
  // one region per convolution, so that the split reduction of a whole backward segment can run as ONE launch after it
  m->defer_wgred = true;
  m->sppf_fuse = (YS_OPT_INT("SPPF_FUSE", 1) != 0);       // YS_SPPF_FUSE=0: three pool launches per SPPF, forward and backward
  m->bnred_on = (YS_OPT_INT("BNRED", 1) != 0);           // YS_BNRED=0: every BN backward runs its own reduction pass
  long wgp = 0, wgp_regions = 0;
  std::vector<long> need(m->convs.size(), 0);
  for (auto& c : m->convs) {
    if (c.dw) continue;
    const Buf& ob = m->bufs[c.out.buf];     // the view geometry the launch will see (the blocked-GEMM plan depends on it): a BN unit's dy is dense, a plain one's the output view
    const WgradArgs a = c.bn ? wgrad_args(m, c, B, c.cout, 0, (long)c.Hout * c.Wout) : wgrad_args(m, c, B, ob.ldc, c.out.coff, ob.rows_per_b, c.ct ? 0 : -1);
    int sp = ys_wgrad_splits(a, m->dtype);
    if (c.k == 6 && &c == stem_unit(m)) sp = std::max(sp, ys_stem6_wgrad_splits(B, c.Hin, c.Win));   // the 6x6 stem kernel leaves one slab per workgroup (the generic route keeps its own count)
    need[c.idx] = (long)sp * c.cout * c.k * c.k * c.cin_pad;
    wgp = std::max(wgp, need[c.idx]);
    if (m->defer_wgred && !c.ct) { c.wgp_splits = sp; wgp_regions += (need[c.idx] + 63) / 64 * 64; }
  }
  {
    long off = (wgp + 63) / 64 * 64;
    // descriptor order = backward-segment order, so that a backward_range call reduces one contiguous run of descriptors.  Within a segment Proto's units
    // come LAST: the one2one pass of an End2End Segment backward launches no weight gradient for them, so it reduces the prefix [red_first[0], red_proto0)
    // only -- their descriptors and partial regions still hold the previous step's values, and the reduction accumulates.  A prefix keeps every blk0 of
    // the full run, so the two reductions of a step share one uploaded table.
    for (int seg = 0; seg < ys_model::NSEG; seg++) {
      m->red_first[seg] = (int)m->red_host.size();
      for (auto& c : m->convs) {
        if (c.seg != seg || c.dw || c.ct || !m->defer_wgred) continue;
        c.wgp_off = off; off += (need[c.idx] + 63) / 64 * 64;
      }
      for (int last = 0; last < 2; last++) {
        if (seg == 0 && last == 1) m->red_proto0 = (int)m->red_host.size();
        for (auto& c : m->convs) {
          if (c.seg != seg || c.dw || c.ct || !m->defer_wgred || (int)c.proto != last) continue;
          c.red_slot = (int)m->red_host.size();
          m->red_host.push_back(WgRedDesc{});
        }
      }
    }
    m->red_first[ys_model::NSEG] = (int)m->red_host.size();
    m->n_wgp = off;
  }
  YS_TRY(dev_alloc(m, (void**)&m->wg_partial, (size_t)m->n_wgp * 4));
  if (!m->red_host.empty()) YS_TRY(dev_alloc(m, (void**)&m->red_dev, m->red_host.size() * sizeof(WgRedDesc)));
  const ys_model_desc& d = m->d;
  YS_TRY(dev_alloc(m, (void**)&m->img_dev, (size_t)B * std::max(3, m->blk_c1) * d.height * d.width * 4));
  YS_TRY(dev_alloc(m, (void**)&m->pred, (size_t)B * (m->cls ? d.nc : (4 + d.nc + m->nm) * m->A) * 4));   // Classify: eval probabilities [B][nc]
  if (m->cls) {
    YS_TRY(dev_alloc(m, (void**)&m->cls_rows, (size_t)2 * B * 4));
    YS_TRY(dev_alloc(m, (void**)&m->cls_lab, (size_t)B * 4));
  }
  m->n_out_stage = std::max((long)B * m->A * std::max(std::max(m->ld_pd, m->ld_ps), 4 + d.nc + m->nm), (long)B * m->mh * m->mw * std::max(m->ld_pr, 1));
  if (m->is_block) { const Buf& ob = m->bufs[m->blk_out]; m->n_out_stage = std::max(m->n_out_stage, (long)B * ob.rows_per_b * ob.ldc); }
  if (m->cls) m->n_out_stage = std::max(m->n_out_stage, (long)B * m->ld_cls);
  if (m->segment) YS_TRY(dev_alloc(m, (void**)&m->masks_dev, (size_t)B * m->mh * m->mw * 4));
  if (m->segment || m->xkind == 3) {   // v8SegmentationLoss / v8PoseLoss: foreground list + partials (Pose: per workgroup)
    YS_TRY(dev_alloc(m, (void**)&m->seg_cnt, (size_t)B * 4));
    YS_TRY(dev_alloc(m, (void**)&m->seg_off, (size_t)(B + 1) * 4));
    YS_TRY(dev_alloc(m, (void**)&m->seg_list, (size_t)B * m->A * 4));
    if (m->segment) YS_TRY(dev_alloc(m, (void**)&m->seg_ent, (size_t)B * m->A * 8 * 4));
    YS_TRY(dev_alloc(m, (void**)&m->seg_part, (size_t)(m->segment ? (long)B * m->A : 2L * ys_loss_pose_grid(B, m->A)) * 4));
  }
  YS_TRY(dev_alloc(m, (void**)&m->out_stage, (size_t)m->n_out_stage * 4));
  // loss workspace (label-capacity dependent part: alloc_label_ws; grown on demand by ys_loss_detect / ys_model_reserve_labels)
  YS_TRY(alloc_label_ws(m, d.max_labels > 0 ? d.max_labels : 64));
  YS_TRY(dev_alloc(m, (void**)&m->pbox, (size_t)B * m->A * 20));
  YS_TRY(dev_alloc(m, (void**)&m->fg_gt, (size_t)B * m->A * 4));
  YS_TRY(dev_alloc(m, (void**)&m->tnorm, (size_t)B * m->A * 4));
  YS_TRY(dev_alloc(m, (void**)&m->loss_partial, ys_loss_partial_floats(B, m->A) * 4));
  YS_TRY(dev_alloc(m, (void**)&m->scalars, 64 * 4 + 64 * 8 * 8));     // 64 float scalars + the criterion's sharded integer accumulators (loss.hip LOSS_ACC: [64][8] u64)
  return YS_OK;
}

WgradArgs wgrad_args(const ys_model* m, const ConvL& c, int B, int dy_ldc, int dy_coff, long dy_bstride, int phase) {
  const Buf& ib = m->bufs[c.in.buf];
  WgradArgs a{};
  a.B = B; a.Hin = c.Hin; a.Win = c.Win; a.Cin = c.cin_pad; a.Hout = c.Hout; a.Wout = c.Wout; a.Cout = c.cout;
  a.KH = a.KW = c.k; a.stride = c.s; a.pad = c.pad;               // (a ConvTranspose unit is recorded with k = 1, s = 1: its phases are 1x1 GEMMs)
  a.in_ldc = ib.ldc; a.in_coff = c.in.coff; a.in_bstride = ib.rows_per_b;
  a.dy_ldc = dy_ldc; a.dy_coff = dy_coff; a.dy_bstride = dy_bstride;
  if (phase >= 0) { a.Hout = c.Hin; a.Wout = c.Win; a.dy_rh = 4 * c.Win; a.dy_rw = 2; a.dy_r0 = (long)(phase >> 1) * 2 * c.Win + (phase & 1); }
  a.M = (int)((long)B * a.Hout * a.Wout);
  return a;
}

// Fused BN-backward reduction, host side.  For every BN Conv unit L find, per output channel, the FIRST op in forward order that
// reads it: that op's backward is the last writer of the channel's gradient dz.  When all of L's channels are completed by the
// dgrad launches of plain convolutions (reading them as their input view, not as a residual) whose kernels carry the fused
// epilogue (ys_conv_bnred_rows), those launches produce L's sums and L's backward skips chan_reduce_kernel.
static ConvArgs dgrad_plan_args(ys_model* m, const ConvL& c, int B, bool f8) {
  const Buf& ob = m->bufs[c.out.buf];
  ConvArgs a = c.bn ? dgrad_args(m, c, B, m->dy_scratch, c.cout, 0, (long)c.Hout * c.Wout)
                    : dgrad_args(m, c, B, view_ptr(m, ob.grad, ob, c.out_rowoff), ob.ldc, c.out.coff, ob.rows_per_b);
  if (f8 && m->f8 && c.f8_bwd) {
    f8_dgrad_operands(m, c, a); a.q8 = m->q8;
    if (c.bn && m->q8 && c.cout_ld == c.cout && ys_conv_wants_x8(a)) a.x8 = m->q8;
  }
  return a;
}
int plan_bnred(ys_model* m, int B) {
  if (m->bnred_B == B) return YS_OK;
  m->bnred_B = B;
  for (auto& c : m->convs) { c.feeds.clear(); c.red_src.clear(); c.red_ok = false; c.red_seen = 0; }
  // fp8 mode: a producer is fused only when its consumers' dgrads carry the fused epilogue under BOTH routings (the scale-less
  // first step runs the bf16 kernels, later steps the fp8 ones): conv_gemm_kernel<e5m2> has the variant, conv_p2_kernel<F8> does not
  if (!m->bnred_on || m->dtype != YS_BF16) return YS_OK;
  const int epl = m->epl;
  // first reader per (buffer, channel): op index and kind (0 = input of a plain convolution, 1 = residual / unsupported reader)
  std::vector<std::vector<int>> fop(m->bufs.size()), fkind(m->bufs.size());
  for (size_t b = 0; b < m->bufs.size(); b++) { fop[b].assign(m->bufs[b].ldc, -1); fkind[b].assign(m->bufs[b].ldc, 1); }
  auto touch = [&](const View& v, int op, int kind) {
    for (int ch = v.coff; ch < v.coff + v.C; ch++) {
      if (fop[v.buf][ch] == -1) { fop[v.buf][ch] = op; fkind[v.buf][ch] = kind; }
      else if (fop[v.buf][ch] == op) fkind[v.buf][ch] = 1;      // read twice by the same op (input and residual): not fusable
    }
  };
  for (size_t oi = 0; oi < m->ops.size(); oi++) {
    const Op& op = m->ops[oi];
    if (op.type == OP_CONV) {
      const ConvL& x = m->convs[op.conv];
      touch(x.in, (int)oi, (x.dw || x.ct || x.first) ? 1 : 0);
      if (x.has_res) touch(x.res, (int)oi, 1);
    } else {
      touch(op.in, (int)oi, 1);
    }
  }
  // candidate feeds
  for (auto& l : m->convs) {
    if (!l.bn || l.ct || l.cout_ld != l.cout) continue;
    bool ok = true;
    std::vector<ConvL::RedSrc> srcs;
    std::vector<std::pair<int, ConvL::RedFeed>> add;           // (consumer conv, feed)
    int ch = l.out.coff;
    while (ok && ch < l.out.coff + l.out.C) {
      const int op = fop[l.out.buf][ch];
      if (op < 0 || fkind[l.out.buf][ch] != 0) { ok = false; break; }
      int e = ch;
      while (e < l.out.coff + l.out.C && fop[l.out.buf][e] == op && fkind[l.out.buf][e] == 0) e++;
      const ConvL& x = m->convs[m->ops[op].conv];
      ConvL::RedFeed f{};
      f.prod = l.idx; f.c0 = ch - x.in.coff; f.c1 = e - x.in.coff; f.yc0 = ch - l.out.coff;
      if (f.c0 % epl || f.c1 % epl || f.yc0 % epl || x.Hin != l.Hout || x.Win != l.Wout) { ok = false; break; }
      add.push_back({x.idx, f});
      ch = e;
    }
    if (!ok || add.empty() || (int)add.size() > YS_BNRED_MAXSEG) continue;
    for (auto& pr : add) m->convs[pr.first].feeds.push_back(pr.second);
    l.red_ok = true;                                           // provisional: consumers are checked below
  }
  // consumers: segment capacity and kernel support; a failing consumer disqualifies the producers it would have served
  bool changed = true;
  while (changed) {
    changed = false;
    for (auto& x : m->convs) {
      if (x.feeds.empty()) continue;
      int rows = 0;
      if ((int)x.feeds.size() <= YS_BNRED_MAXSEG) {
        ConvArgs a = dgrad_plan_args(m, x, B, false);
        rows = ys_conv_bnred_rows(a, m->dtype);
        if (rows > 0 && m->f8) { ConvArgs a8 = dgrad_plan_args(m, x, B, true); const int r8 = ys_conv_bnred_rows(a8, m->dtype); rows = r8 > 0 ? std::max(rows, r8) : 0; }
      }
      for (auto& f : x.feeds) f.rows_cap = rows;
      if (rows == 0) {
        for (auto& f : x.feeds) m->convs[f.prod].red_ok = false;
        x.feeds.clear();
        changed = true;
      }
    }
    for (auto& x : m->convs) {                                  // drop feeds of disqualified producers
      const size_t n0 = x.feeds.size();
      x.feeds.erase(std::remove_if(x.feeds.begin(), x.feeds.end(), [&](const ConvL::RedFeed& f) { return !m->convs[f.prod].red_ok; }), x.feeds.end());
      if (x.feeds.size() != n0) changed = true;
    }
  }
  // partial-row regions and the producers' source lists
  long off = 0;
  for (auto& x : m->convs)
    for (size_t k = 0; k < x.feeds.size(); k++) {
      ConvL::RedFeed& f = x.feeds[k];
      f.part_off = off; off += (long)f.rows_cap * 2 * m->convs[f.prod].cout;
      m->convs[f.prod].red_src.push_back(ConvL::RedSrc{x.idx, (int)k});
    }
  for (auto& l : m->convs) {
    std::sort(l.red_src.begin(), l.red_src.end(), [&](const ConvL::RedSrc& p, const ConvL::RedSrc& q) {
      return m->convs[p.cons].feeds[p.feed].yc0 < m->convs[q.cons].feeds[q.feed].yc0; });
    if (l.red_src.empty()) l.red_ok = false;
  }
  if (off > m->n_bnred) {
    if (m->bnred_part) { YS_CHECK_HIP(hipStreamSynchronize(m->ctx->stream)); dev_free_tracked(m, m->bnred_part); m->bnred_part = nullptr; }
    YS_TRY(dev_alloc(m, (void**)&m->bnred_part, (size_t)off * 4));
    m->n_bnred = off;
  }
  if (YS_OPT_INT("BNRED_LOG", 0) != 0) {        // plan report (tests/test_bnred.py reads the count)
    int nf = 0, nb = 0;
    for (auto& l : m->convs) { if (l.bn) nb++; if (l.red_ok) nf++; }
    fprintf(stderr, "[ys] fused BN-backward reduction: %d of %d BN conv units (B=%d, %.1f MB of partial rows)\n", nf, nb, B, off * 4.0 / 1e6);
    for (auto& l : m->convs) if (l.bn && !l.red_ok) fprintf(stderr, "[ys]   not fused: %s\n", l.name.c_str());
  }
  return YS_OK;
}

}  // namespace ysm
