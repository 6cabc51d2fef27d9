// ops_augment.hip -- the training input's entry points of the C ABI (augment.hip), the ones a host calls every step with device pointers (on_device != 0) and
// the tests with host arrays: Mosaic4 + RandomPerspective + flips + Normalize + collate (Data/Augment.cs:158-274, 315-695, 860-966; Data/YoloDataset.cs:102-151;
// Data/YoloDataLoader.cs:18-44), the LetterBox (close-mosaic) branch (Data/YoloDataset.cs:378-429; Data/Augment.cs:698-778, 860-966), ColorJitter, OBB labels, and the classification input (Data/ClassificationDataset.cs:90-131; augment_cls.hip).
#include "ops_stage.h"

namespace {
int aug_reserve_ws(ys_ctx* ctx, int batch) { return ys_ctx_reserve_ws(ctx, &ctx->aug_ws, &ctx->aug_ws_bytes, ys_aug_ws_bytes(batch), "ys_augment"); }

// the part of the arena the sources name (what a host-pointer call uploads)
size_t aug_arena_bytes(const ys_aug_src* srcs, int n_src) {
  size_t bytes = 0;
  for (int k = 0; k < n_src; k++) {
    const ys_aug_src& sr = srcs[k];
    if (sr.img_off >= 0 && sr.h > 0 && sr.w > 0) { const size_t e = (size_t)sr.img_off + (size_t)3 * sr.h * sr.w; bytes = e > bytes ? e : bytes; }
    if (sr.mask_off >= 0 && sr.mh > 0 && sr.mw > 0) { const size_t e = (size_t)sr.mask_off + (size_t)sr.mh * sr.mw; bytes = e > bytes ? e : bytes; }
  }
  return bytes;
}
// the checks a host-resident Mosaic item table allows (include/yolosharp_hip.h); n_src < 0: unknown, only src >= 0 is checked
int aug_check_items(const char* fn, const ys_aug_item* items, int batch, const ys_aug_src* srcs, int n_src, int s, int perspective) {
  for (int b = 0; b < batch; b++) {
    const ys_aug_item& it = items[b];
    for (int i = 0; i < 4; i++)
      if (n_src < 0) YS_REQUIRE(it.src[i] >= 0, "%s: item %d: src[%d] = %d is negative", fn, b, i, it.src[i]);
      else YS_REQUIRE(it.src[i] >= 0 && it.src[i] < n_src, "%s: item %d: src[%d] = %d is outside [0, %d)", fn, b, i, it.src[i], n_src);
    YS_REQUIRE(it.xc >= 0 && it.xc <= 2 * s && it.yc >= 0 && it.yc <= 2 * s, "%s: item %d: centre (%d, %d) is outside [0, %d]", fn, b, it.xc, it.yc, 2 * s);
    int mx = 0;
    for (int i = 0; i < 4; i++) mx = it.src[i] > mx ? it.src[i] : mx;
    for (int i = 0; i < 4; i++)
      YS_REQUIRE(srcs[it.src[i]].h > 0 && srcs[it.src[i]].w > 0 && srcs[it.src[i]].img_off >= 0, "%s: source %d has no image", fn, it.src[i]);
    YS_REQUIRE(ys_aug_item_ok_host(&it, srcs, mx + 1, s, perspective), "%s: item %d: M is singular", fn, b);
  }
  return YS_OK;
}
// ... and a LetterBox one: src[0] alone
int aug_check_letterbox_items(const char* fn, const ys_aug_item* items, int batch, const ys_aug_src* srcs, int n_src) {
  for (int b = 0; b < batch; b++) {
    const int k = items[b].src[0];
    YS_REQUIRE(k >= 0 && k < n_src, "%s: item %d: src[0] = %d is outside [0, %d)", fn, b, k, n_src);
    YS_REQUIRE(ys_aug_letterbox_src_host(&items[b], srcs, n_src) == k, "%s: source %d has no image", fn, k);
  }
  return YS_OK;
}
// the checks a host-resident jitter table allows: every row valid (YS_ERR_INVALID_ARG); allow_contrast = 0: no row runs contrast (YS_ERR_UNSUPPORTED).
// *any_contrast (may be NULL) = some row runs it
int aug_check_jitter(const char* fn, const ys_aug_jitter* rows, int batch, int allow_contrast, int* any_contrast) {
  int any = 0;
  for (int b = 0; b < batch; b++) {
    const ys_aug_jitter& J = rows[b];
    const int state = ys_aug_jitter_state_host(&J);
    YS_REQUIRE(state != 0, "%s: jitter row %d is invalid: order (%d, %d, %d, %d) must hold ids in {-1, 0..3} with none twice, factors (%g, %g, %g) must be "
               "finite and >= 0, hue %g in [-0.5, 0.5]", fn, b, J.order[0], J.order[1], J.order[2], J.order[3], (double)J.factor[0], (double)J.factor[1],
               (double)J.factor[2], (double)J.factor[3]);
    if (state == 2 && !allow_contrast) {
      ys_set_error("%s: jitter row %d runs contrast: the fused entries have no image mean (ys_color_jitter does)", fn, b);
      return YS_ERR_UNSUPPORTED;
    }
    any |= state == 2;
  }
  if (any_contrast) *any_contrast = any;
  return YS_OK;
}

// ---- the image side of Mosaic and LetterBox, with and without jitter
// the tables of one call, on the host or on the device
struct AugImageIO {
  const uint8_t* arena; const ys_aug_src* srcs; const ys_aug_item* items; const ys_aug_jitter* jitter;
  float *images, *masks;
};
int aug_image_args(const char* fn, ys_ctx* ctx, const AugImageIO& io, int n_src, int batch, int imgsz) {
  YS_REQUIRE(ctx && io.arena && io.srcs && io.items && io.images, "%s: null argument", fn);
  YS_REQUIRE(batch > 0 && batch <= 65535 && n_src > 0, "%s: bad shape batch=%d (1..65535) n_src=%d", fn, batch, n_src);
  YS_REQUIRE(imgsz >= 2 && imgsz % 2 == 0 && imgsz <= 16384, "%s: imgsz %d must be even and in [2, 16384]", fn, imgsz);
  return YS_OK;
}
// check_items: the checks the host-resident item table allows; launch(io): the kernels on device pointers -- the two parts that differ.  r: the mask ratio
template <class Check, class Launch>
int aug_images(const char* fn, const char* timer_name, ys_ctx* ctx, const AugImageIO& h, int n_src, int batch, int on_device, int imgsz, int r, Check check_items,
               Launch launch) {
  hipStream_t st = ctx->stream;
  YsTimer timer(ctx, timer_name);
  if (on_device) return launch(h);
  YS_TRY(check_items());
  if (h.jitter) YS_TRY(aug_check_jitter(fn, h.jitter, batch, 0, nullptr));
  const size_t arena_bytes = aug_arena_bytes(h.srcs, n_src), src_bytes = (size_t)n_src * sizeof(ys_aug_src), item_bytes = (size_t)batch * sizeof(ys_aug_item);
  const size_t n_img = (size_t)batch * 3 * imgsz * imgsz, n_msk = h.masks ? (size_t)batch * (imgsz / r) * (imgsz / r) : 0;
  DevBuf da, ds, di, dj, dimg, dm;
  YS_TRY(da.alloc(arena_bytes)); YS_TRY(ds.alloc(src_bytes)); YS_TRY(di.alloc(item_bytes));
  YS_TRY(dimg.alloc(n_img * 4)); YS_TRY(dm.alloc(n_msk * 4));
  YS_TRY(h2d(st, da.p, h.arena, arena_bytes));
  YS_TRY(h2d(st, ds.p, h.srcs, src_bytes));
  YS_TRY(h2d(st, di.p, h.items, item_bytes));
  if (h.jitter) {
    YS_TRY(dj.alloc((size_t)batch * sizeof(ys_aug_jitter)));
    YS_TRY(h2d(st, dj.p, h.jitter, (size_t)batch * sizeof(ys_aug_jitter)));
  }
  const AugImageIO d{da.as<uint8_t>(), ds.as<ys_aug_src>(), di.as<ys_aug_item>(), h.jitter ? dj.as<ys_aug_jitter>() : nullptr, dimg.as<float>(),
                     h.masks ? dm.as<float>() : nullptr};
  YS_TRY(launch(d));
  YS_TRY(d2h(st, h.images, dimg.p, n_img * 4));
  if (h.masks) YS_TRY(d2h(st, h.masks, dm.p, n_msk * 4));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  return YS_OK;
}

int aug_mosaic_impl(const char* fn, ys_ctx* ctx, const uint8_t* arena, const ys_aug_src* srcs, int n_src, const ys_aug_item* items, int batch, int on_device,
                    int imgsz, int mask_ratio, int perspective, const ys_aug_jitter* jitter, float* images, float* masks) {
  const AugImageIO io{arena, srcs, items, jitter, images, masks};
  YS_TRY(aug_image_args(fn, ctx, io, n_src, batch, imgsz));
  if (masks) YS_REQUIRE(mask_ratio >= 1 && imgsz % mask_ratio == 0 && 2 * imgsz / mask_ratio >= 2, "%s: mask_ratio %d does not divide imgsz %d", fn, mask_ratio, imgsz);
  const int r = masks ? mask_ratio : 1, persp = perspective != 0;
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  YS_TRY(aug_reserve_ws(ctx, batch));
  return aug_images(fn, "augment", ctx, io, n_src, batch, on_device, imgsz, r, [&] { return aug_check_items(fn, items, batch, srcs, n_src, imgsz, persp); },
                    [&](const AugImageIO& a) {
                      return ys_aug_mosaic_launch(ctx->stream, a.arena, a.srcs, n_src, a.items, batch, imgsz, r, persp, a.jitter, ctx->aug_ws, a.images, a.masks);
                    });
}

int aug_letterbox_impl(const char* fn, ys_ctx* ctx, const uint8_t* arena, const ys_aug_src* srcs, int n_src, const ys_aug_item* items, int batch,
                       int on_device, int imgsz, int mask_ratio, const ys_aug_jitter* jitter, float* images, float* masks) {
  const AugImageIO io{arena, srcs, items, jitter, images, masks};
  YS_TRY(aug_image_args(fn, ctx, io, n_src, batch, imgsz));
  if (masks) YS_REQUIRE(mask_ratio >= 1 && imgsz % mask_ratio == 0, "%s: mask_ratio %d does not divide imgsz %d", fn, mask_ratio, imgsz);
  const int r = masks ? mask_ratio : 1;
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  return aug_images(fn, "augment_letterbox", ctx, io, n_src, batch, on_device, imgsz, r, [&] { return aug_check_letterbox_items(fn, items, batch, srcs, n_src); },
                    [&](const AugImageIO& a) { return ys_aug_letterbox_launch(ctx->stream, a.arena, a.srcs, n_src, a.items, batch, imgsz, r, a.jitter, a.images, a.masks); });
}

// ---- the label side: ys_augment_labels / ys_augment_letterbox_labels (corners == NULL) and their _obb forms (corners [n, 4, 2] in place of the keypoints,
//      out_bboxes [capacity, 5], flags 0)
// the tables of one call, on the host or on the device.  extra: the per-label table beside the boxes, K keypoints of 3 floats or 4 corners of 2
struct AugLabelIO {
  const ys_aug_src* srcs; const int32_t* lab_off; const float *cls, *boxes, *extra; const ys_aug_item* items;
  float *batch_idx, *out_cls, *bboxes, *keypoints; int32_t* count;
  int K, obb;
};
// flags_known: the box-flip switches the entry accepts
int aug_label_args(const char* fn, ys_ctx* ctx, const float* keypoints, int kpt_num, int kpt_dim, const float* corners, int batch, int imgsz, int flags,
                   int flags_known, AugLabelIO& io) {
  YS_REQUIRE(ctx && io.srcs && io.lab_off && io.cls && io.boxes && io.items && io.batch_idx && io.out_cls && io.bboxes && io.count && (!io.obb || corners),
             "%s: null argument", fn);
  YS_REQUIRE(imgsz >= 2 && imgsz % 2 == 0 && imgsz <= 16384, "%s: imgsz %d must be even and in [2, 16384]", fn, imgsz);
  YS_REQUIRE((keypoints != nullptr) == (io.keypoints != nullptr), "%s: keypoints and out_keypoints go together", fn);
  if (keypoints) {
    YS_REQUIRE(kpt_dim == 3, "%s: kpt_dim %d: only (x, y, visibility) keypoints are supported (apply_keypoints reads column 2)", fn, kpt_dim);
    YS_REQUIRE(kpt_num > 0, "%s: kpt_num %d", fn, kpt_num);
  }
  if (io.obb) YS_REQUIRE(flags == 0, "%s: flags 0x%x: the box-flip switches have nothing to act on, flags must be 0", fn, flags);
  else YS_REQUIRE((flags & ~flags_known) == 0, "%s: unknown flags 0x%x", fn, flags);
  io.K = keypoints ? kpt_num : 0;
  io.extra = io.obb ? corners : keypoints;
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  return aug_reserve_ws(ctx, batch);
}
// the host-pointer call: the n_src sources' tables and their n_lab labels to the device, launch(io, n_src) on them, the capacity output rows back
template <class Launch>
int aug_labels_staged(hipStream_t st, const AugLabelIO& h, int n_src, size_t n_lab, int batch, int capacity, Launch launch) {
  const size_t cap = (size_t)capacity, xf = h.obb ? 8 : (size_t)h.K * 3, bw = h.obb ? 5 : 4;      // floats of an `extra` row; the width of an output box row
  const size_t src_bytes = (size_t)n_src * sizeof(ys_aug_src), off_bytes = (size_t)(n_src + 1) * 4, item_bytes = (size_t)batch * sizeof(ys_aug_item);
  DevBuf ds, dl, dc, db, dk, di, obi, ocl, obx, okp, ocn;
  YS_TRY(ds.alloc(src_bytes)); YS_TRY(dl.alloc(off_bytes)); YS_TRY(dc.alloc(n_lab * 4)); YS_TRY(db.alloc(n_lab * 16));
  YS_TRY(dk.alloc(n_lab * xf * 4)); YS_TRY(di.alloc(item_bytes));
  YS_TRY(obi.alloc(cap * 4)); YS_TRY(ocl.alloc(cap * 4)); YS_TRY(obx.alloc(cap * bw * 4)); YS_TRY(okp.alloc(cap * h.K * 12)); YS_TRY(ocn.alloc(4));
  YS_TRY(h2d(st, ds.p, h.srcs, src_bytes));
  YS_TRY(h2d(st, dl.p, h.lab_off, off_bytes));
  if (n_lab) {
    YS_TRY(h2d(st, dc.p, h.cls, n_lab * 4));
    YS_TRY(h2d(st, db.p, h.boxes, n_lab * 16));
    if (xf) YS_TRY(h2d(st, dk.p, h.extra, n_lab * xf * 4));
  }
  YS_TRY(h2d(st, di.p, h.items, item_bytes));
  const AugLabelIO d{ds.as<ys_aug_src>(), dl.as<int32_t>(), dc.as<float>(), db.as<float>(), xf ? dk.as<float>() : nullptr, di.as<ys_aug_item>(),
                     obi.as<float>(), ocl.as<float>(), obx.as<float>(), h.K ? okp.as<float>() : nullptr, ocn.as<int32_t>(), h.K, h.obb};
  YS_TRY(launch(d, n_src));
  YS_TRY(d2h(st, h.batch_idx, obi.p, cap * 4));
  YS_TRY(d2h(st, h.out_cls, ocl.p, cap * 4));
  YS_TRY(d2h(st, h.bboxes, obx.p, cap * bw * 4));
  if (h.K) YS_TRY(d2h(st, h.keypoints, okp.p, cap * h.K * 12));
  YS_TRY(d2h(st, h.count, ocn.p, 4));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  return YS_OK;
}

int aug_labels_impl(const char* fn, ys_ctx* ctx, const float* keypoints, int kpt_num, int kpt_dim, const float* corners, int batch, int on_device, int imgsz,
                    int perspective, int flags, int capacity, AugLabelIO io) {
  YS_REQUIRE(batch > 0 && batch <= 65535 && capacity > 0, "%s: bad shape batch=%d (1..65535) capacity=%d", fn, batch, capacity);
  YS_TRY(aug_label_args(fn, ctx, keypoints, kpt_num, kpt_dim, corners, batch, imgsz, flags, YS_AUG_SORT_FLIPPED, io));
  hipStream_t st = ctx->stream;
  const int persp = perspective != 0;
  YsTimer timer(ctx, "augment_labels");
  auto launch = [&](const AugLabelIO& a, int n_src) {
    return ys_aug_labels_launch(st, a.srcs, n_src, a.lab_off, a.cls, a.boxes, a.extra, a.K, a.items, batch, imgsz, persp, flags, capacity, ctx->aug_ws, a.batch_idx,
                                a.out_cls, a.bboxes, a.keypoints, a.count, a.obb);
  };
  // the source count is not part of the signature: lab_off has one entry per source and one more, device items are the caller's responsibility
  if (on_device) return launch(io, 0x7fffffff);
  YS_TRY(aug_check_items(fn, io.items, batch, io.srcs, -1, imgsz, persp));
  int n_src = 0;
  for (int b = 0; b < batch; b++) for (int i = 0; i < 4; i++) n_src = io.items[b].src[i] + 1 > n_src ? io.items[b].src[i] + 1 : n_src;
  size_t n_lab = 0;
  for (int b = 0; b < batch; b++) {
    long sum = 0;
    for (int i = 0; i < 4; i++) {
      const int k = io.items[b].src[i];
      YS_REQUIRE(io.lab_off[k] >= 0 && io.lab_off[k + 1] >= io.lab_off[k], "%s: lab_off is not non-decreasing at source %d", fn, k);
      sum += io.lab_off[k + 1] - io.lab_off[k];
      n_lab = (size_t)io.lab_off[k + 1] > n_lab ? (size_t)io.lab_off[k + 1] : n_lab;
    }
    YS_REQUIRE(sum <= capacity, "%s: item %d carries %ld labels over its four tiles, capacity is %d", fn, b, sum, capacity);
  }
  return aug_labels_staged(st, io, n_src, n_lab, batch, capacity, launch);
}

int aug_letterbox_labels_impl(const char* fn, ys_ctx* ctx, int n_src, const float* keypoints, int kpt_num, int kpt_dim, const float* corners, int batch,
                              int on_device, int imgsz, int flags, int capacity, AugLabelIO io) {
  YS_REQUIRE(batch > 0 && batch <= 65535 && capacity > 0 && n_src > 0, "%s: bad shape batch=%d (1..65535) capacity=%d n_src=%d", fn, batch, capacity, n_src);
  YS_TRY(aug_label_args(fn, ctx, keypoints, kpt_num, kpt_dim, corners, batch, imgsz, flags, YS_AUG_SORT_FLIPPED | YS_AUG_FLIP_KEEP_SIZE, io));
  hipStream_t st = ctx->stream;
  YsTimer timer(ctx, "augment_letterbox_labels");
  auto launch = [&](const AugLabelIO& a, int ns) {
    return ys_aug_letterbox_labels_launch(st, a.srcs, ns, a.lab_off, a.cls, a.boxes, a.extra, a.K, a.items, batch, imgsz, flags, capacity, ctx->aug_ws, a.batch_idx,
                                          a.out_cls, a.bboxes, a.keypoints, a.count, a.obb);
  };
  if (on_device) return launch(io, n_src);
  YS_TRY(aug_check_letterbox_items(fn, io.items, batch, io.srcs, n_src));
  for (int k = 0; k < n_src; k++)
    YS_REQUIRE(io.lab_off[k] >= 0 && io.lab_off[k + 1] >= io.lab_off[k], "%s: lab_off is not non-decreasing at source %d", fn, k);
  long total = 0;
  for (int b = 0; b < batch; b++) total += io.lab_off[io.items[b].src[0] + 1] - io.lab_off[io.items[b].src[0]];
  YS_REQUIRE(total <= capacity, "%s: the batch carries %ld labels, capacity is %d", fn, total, capacity);
  return aug_labels_staged(st, io, n_src, (size_t)io.lab_off[n_src], batch, capacity, launch);
}
}  // namespace

extern "C" int ys_augment_mosaic(ys_ctx* ctx, const uint8_t* arena, const ys_aug_src* srcs, int n_src, const ys_aug_item* items, int batch,
                                 int on_device, int imgsz, int mask_ratio, int perspective, float* images, float* masks) {
  return aug_mosaic_impl("ys_augment_mosaic", ctx, arena, srcs, n_src, items, batch, on_device, imgsz, mask_ratio, perspective, nullptr, images, masks);
}

// the same with the ColorJitter (RandomHSV, Data/Augment.cs:968-987) rows of the batch in the warp kernel's epilogue; jitter == NULL is the entry above
extern "C" int ys_augment_mosaic_jitter(ys_ctx* ctx, const uint8_t* arena, const ys_aug_src* srcs, int n_src, const ys_aug_item* items, int batch,
                                        int on_device, int imgsz, int mask_ratio, int perspective, const ys_aug_jitter* jitter, float* images,
                                        float* masks) {
  return aug_mosaic_impl("ys_augment_mosaic_jitter", ctx, arena, srcs, n_src, items, batch, on_device, imgsz, mask_ratio, perspective, jitter, images, masks);
}

extern "C" int ys_augment_letterbox(ys_ctx* ctx, const uint8_t* arena, const ys_aug_src* srcs, int n_src, const ys_aug_item* items, int batch,
                                    int on_device, int imgsz, int mask_ratio, float* images, float* masks) {
  return aug_letterbox_impl("ys_augment_letterbox", ctx, arena, srcs, n_src, items, batch, on_device, imgsz, mask_ratio, nullptr, images, masks);
}

// the same with the batch's ColorJitter rows in the image kernel's epilogue; jitter == NULL is the entry above
extern "C" int ys_augment_letterbox_jitter(ys_ctx* ctx, const uint8_t* arena, const ys_aug_src* srcs, int n_src, const ys_aug_item* items, int batch,
                                           int on_device, int imgsz, int mask_ratio, const ys_aug_jitter* jitter, float* images, float* masks) {
  return aug_letterbox_impl("ys_augment_letterbox_jitter", ctx, arena, srcs, n_src, items, batch, on_device, imgsz, mask_ratio, jitter, images, masks);
}

extern "C" int ys_augment_labels(ys_ctx* ctx, const ys_aug_src* srcs, const int32_t* lab_off, const float* cls, const float* boxes,
                                 const float* keypoints, int kpt_num, int kpt_dim, const ys_aug_item* items, int batch, int on_device,
                                 int imgsz, int perspective, int flags, int capacity, float* out_batch_idx, float* out_cls, float* out_bboxes,
                                 float* out_keypoints, int32_t* out_count) {
  return aug_labels_impl("ys_augment_labels", ctx, keypoints, kpt_num, kpt_dim, nullptr, batch, on_device, imgsz, perspective, flags, capacity,
                         AugLabelIO{srcs, lab_off, cls, boxes, nullptr, items, out_batch_idx, out_cls, out_bboxes, out_keypoints, out_count, 0, 0});
}

// OBB corner labels (Data/YoloDataset.cs:110-129, 216-244): the corners through the chain, the minimum-area rectangle, rows of 5
extern "C" int ys_augment_labels_obb(ys_ctx* ctx, const ys_aug_src* srcs, const int32_t* lab_off, const float* cls, const float* boxes,
                                     const float* corners, const ys_aug_item* items, int batch, int on_device, int imgsz, int perspective, int flags,
                                     int capacity, float* out_batch_idx, float* out_cls, float* out_bboxes, int32_t* out_count) {
  return aug_labels_impl("ys_augment_labels_obb", ctx, nullptr, 0, 3, corners, batch, on_device, imgsz, perspective, flags, capacity,
                         AugLabelIO{srcs, lab_off, cls, boxes, nullptr, items, out_batch_idx, out_cls, out_bboxes, nullptr, out_count, 0, 1});
}

extern "C" int ys_augment_letterbox_labels(ys_ctx* ctx, const ys_aug_src* srcs, int n_src, const int32_t* lab_off, const float* cls, const float* boxes,
                                           const float* keypoints, int kpt_num, int kpt_dim, const ys_aug_item* items, int batch, int on_device,
                                           int imgsz, int flags, int capacity, float* out_batch_idx, float* out_cls, float* out_bboxes,
                                           float* out_keypoints, int32_t* out_count) {
  return aug_letterbox_labels_impl("ys_augment_letterbox_labels", ctx, n_src, keypoints, kpt_num, kpt_dim, nullptr, batch, on_device, imgsz, flags, capacity,
                                   AugLabelIO{srcs, lab_off, cls, boxes, nullptr, items, out_batch_idx, out_cls, out_bboxes, out_keypoints, out_count, 0, 0});
}

extern "C" int ys_augment_letterbox_labels_obb(ys_ctx* ctx, const ys_aug_src* srcs, int n_src, const int32_t* lab_off, const float* cls, const float* boxes,
                                               const float* corners, const ys_aug_item* items, int batch, int on_device, int imgsz, int flags, int capacity,
                                               float* out_batch_idx, float* out_cls, float* out_bboxes, int32_t* out_count) {
  return aug_letterbox_labels_impl("ys_augment_letterbox_labels_obb", ctx, n_src, nullptr, 0, 3, corners, batch, on_device, imgsz, flags, capacity,
                                   AugLabelIO{srcs, lab_off, cls, boxes, nullptr, items, out_batch_idx, out_cls, out_bboxes, nullptr, out_count, 0, 1});
}

// the rectangle on its own: corners [n, 4, 2] -> out [n, 5] = cx, cy, w, h in the corners' units, angle in radians; n == 0 does nothing
extern "C" int ys_xyxyxyxy2xywhr(ys_ctx* ctx, const float* corners, int n, int on_device, float* out) {
  YS_REQUIRE(ctx && n >= 0 && (n == 0 || (corners && out)), "ys_xyxyxyxy2xywhr: null argument or n = %d < 0", n);
  if (n == 0) return YS_OK;
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  YsTimer timer(ctx, "xyxyxyxy2xywhr");
  if (on_device) return ys_xyxyxyxy2xywhr_launch(st, corners, n, out);
  DevBuf dc, dout;
  YS_TRY(dc.alloc((size_t)n * 32)); YS_TRY(dout.alloc((size_t)n * 20));
  YS_TRY(h2d(st, dc.p, corners, (size_t)n * 32));
  YS_TRY(ys_xyxyxyxy2xywhr_launch(st, (const float*)dc.p, n, (float*)dout.p));
  YS_TRY(d2h(st, out, dout.p, (size_t)n * 20));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  return YS_OK;
}

// ---- the classification input (augment_cls.hip; Data/ClassificationDataset.cs:90-131): crop / resize / flips / erase / ColorJitter / mul(1 / 255) as one
//      gather, and the class ids.  The contrast reduction's per-image sums live in the augmenter's workspace, zeroed on the stream each call.
//      aa != NULL (ys_augment_classify_aa): the AutoAugment / RandAugment slots between the flips and the erase, on uint8 images staged in the context's
//      second workspace (AaWs), whose statistics rows are zeroed on the stream each call.
namespace {
// the context's AutoAugment workspace: statistics rows | image A | image B (each image B * 3 * h * w bytes, 16-byte aligned)
struct AaWs { void* stats; unsigned char *a, *b; size_t stats_bytes; };
int aa_reserve_ws(ys_ctx* ctx, int batch, int h, int w, AaWs* ws) {
  const size_t sb = (ys_aa_stats_bytes(batch) + 15) & ~(size_t)15, ib = ((size_t)batch * 3 * h * w + 15) & ~(size_t)15;
  YS_TRY(ys_ctx_reserve_ws(ctx, &ctx->aa_ws, &ctx->aa_ws_bytes, sb + 2 * ib, "ys_auto_augment"));
  ws->stats = ctx->aa_ws; ws->a = (unsigned char*)ctx->aa_ws + sb; ws->b = ws->a + ib; ws->stats_bytes = sb;
  return YS_OK;
}
// the checks a host-resident ys_aa_row table allows; *stats_mask bit k = some row's slot k needs the statistics launch
int aa_check_rows(const char* fn, const ys_aa_row* rows, int batch, int* stats_mask) {
  int mask = 0;
  for (int b = 0; b < batch; b++) {
    const ys_aa_row& r = rows[b];
    YS_REQUIRE(ys_aa_row_ok_host(&r), "%s: aa row %d is invalid: ops (%d, %d) must be in -1 .. 13, args (%g, %g) and theta finite, Posterize bits in 0 .. 8", fn, b,
               r.op[0], r.op[1], (double)r.arg[0], (double)r.arg[1]);
    for (int k = 0; k < 2; k++) mask |= ys_aa_row_needs_stats_host(&r, k) << k;
  }
  *stats_mask = mask;
  return YS_OK;
}

int aug_classify_impl(const char* fn, ys_ctx* ctx, const uint8_t* arena, const ys_aug_src* srcs, int n_src, const float* src_cls, const ys_cls_item* items,
                      int batch, int on_device, int imgsz, const ys_aa_row* aa, const ys_aug_jitter* jitter, float* images, float* out_cls) {
  YS_REQUIRE(ctx && arena && srcs && src_cls && items && images && out_cls, "%s: null argument", fn);
  YS_REQUIRE(batch > 0 && batch <= 65535 && n_src > 0, "%s: bad shape batch=%d (1..65535) n_src=%d", fn, batch, n_src);
  YS_REQUIRE(imgsz >= 1 && imgsz <= 16384, "%s: imgsz %d must be in [1, 16384]", fn, imgsz);
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  YS_TRY(aug_reserve_ws(ctx, batch));
  AaWs aws{};
  if (aa) YS_TRY(aa_reserve_ws(ctx, batch, imgsz, imgsz, &aws));
  YsTimer timer(ctx, "augment_classify");
  if (on_device) {                                         // the host cannot read the rows: the reductions run and leave at once where a row needs none
    if (jitter) YS_CHECK_HIP(hipMemsetAsync(ctx->aug_ws, 0, (size_t)batch * 8, st));
    if (!aa) return ys_aug_classify_launch(st, arena, srcs, n_src, src_cls, items, batch, imgsz, jitter, 1, ctx->aug_ws, images, out_cls);
    YS_CHECK_HIP(hipMemsetAsync(aws.stats, 0, aws.stats_bytes, st));
    return ys_aug_classify_aa_launch(st, arena, srcs, n_src, src_cls, items, batch, imgsz, aa, 3, aws.stats, aws.a, aws.b, jitter, 1, ctx->aug_ws, images, out_cls);
  }
  for (int b = 0; b < batch; b++) {
    const ys_cls_item& it = items[b];
    YS_REQUIRE(ys_aug_cls_item_ok_host(&it, srcs, n_src, imgsz), "%s: item %d is invalid: src %d of %d, crop (top %d, left %d, %d x %d), resized %d x %d, window "
               "(%d, %d) + %d, flips (%d, %d), erase (y %d, x %d, %d x %d)", fn, b, it.src, n_src, it.top, it.left, it.ch, it.cw, it.oh, it.ow, it.oy, it.ox, imgsz,
               it.flip_lr, it.flip_ud, it.er_y, it.er_x, it.er_h, it.er_w);
  }
  int contrast = 0, stats_mask = 0;
  if (aa) YS_TRY(aa_check_rows(fn, aa, batch, &stats_mask));
  if (jitter) YS_TRY(aug_check_jitter(fn, jitter, batch, 1, &contrast));
  const size_t arena_bytes = aug_arena_bytes(srcs, n_src), src_bytes = (size_t)n_src * sizeof(ys_aug_src), item_bytes = (size_t)batch * sizeof(ys_cls_item);
  const size_t jit_bytes = (size_t)batch * sizeof(ys_aug_jitter), n_img = (size_t)batch * 3 * imgsz * imgsz;
  DevBuf da, ds, dc, di, dj, daa, dimg, dcls;
  YS_TRY(da.alloc(arena_bytes)); YS_TRY(ds.alloc(src_bytes)); YS_TRY(dc.alloc((size_t)n_src * 4)); YS_TRY(di.alloc(item_bytes));
  YS_TRY(dimg.alloc(n_img * 4)); YS_TRY(dcls.alloc((size_t)batch * 4));
  YS_TRY(h2d(st, da.p, arena, arena_bytes));
  YS_TRY(h2d(st, ds.p, srcs, src_bytes));
  YS_TRY(h2d(st, dc.p, src_cls, (size_t)n_src * 4));
  YS_TRY(h2d(st, di.p, items, item_bytes));
  if (jitter) {
    YS_TRY(dj.alloc(jit_bytes));
    YS_TRY(h2d(st, dj.p, jitter, jit_bytes));
  }
  if (contrast) YS_CHECK_HIP(hipMemsetAsync(ctx->aug_ws, 0, (size_t)batch * 8, st));
  if (aa) {
    YS_TRY(daa.alloc((size_t)batch * sizeof(ys_aa_row)));
    YS_TRY(h2d(st, daa.p, aa, (size_t)batch * sizeof(ys_aa_row)));
    if (stats_mask) YS_CHECK_HIP(hipMemsetAsync(aws.stats, 0, aws.stats_bytes, st));
    YS_TRY(ys_aug_classify_aa_launch(st, da.as<unsigned char>(), ds.as<ys_aug_src>(), n_src, dc.as<float>(), di.as<ys_cls_item>(), batch, imgsz,
                                     daa.as<ys_aa_row>(), stats_mask, aws.stats, aws.a, aws.b, jitter ? dj.as<ys_aug_jitter>() : nullptr, contrast, ctx->aug_ws,
                                     dimg.as<float>(), dcls.as<float>()));
  } else {
    YS_TRY(ys_aug_classify_launch(st, da.as<unsigned char>(), ds.as<ys_aug_src>(), n_src, dc.as<float>(), di.as<ys_cls_item>(), batch, imgsz,
                                  jitter ? dj.as<ys_aug_jitter>() : nullptr, contrast, ctx->aug_ws, dimg.as<float>(), dcls.as<float>()));
  }
  YS_TRY(d2h(st, images, dimg.p, n_img * 4));
  YS_TRY(d2h(st, out_cls, dcls.p, (size_t)batch * 4));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  return YS_OK;
}
}  // namespace

extern "C" int ys_augment_classify(ys_ctx* ctx, const uint8_t* arena, const ys_aug_src* srcs, int n_src, const float* src_cls, const ys_cls_item* items,
                                   int batch, int on_device, int imgsz, const ys_aug_jitter* jitter, float* images, float* out_cls) {
  return aug_classify_impl("ys_augment_classify", ctx, arena, srcs, n_src, src_cls, items, batch, on_device, imgsz, nullptr, jitter, images, out_cls);
}

// the same with the AutoAugment / RandAugment rows of the batch; aa == NULL is the entry above
extern "C" int ys_augment_classify_aa(ys_ctx* ctx, const uint8_t* arena, const ys_aug_src* srcs, int n_src, const float* src_cls, const ys_cls_item* items,
                                      int batch, int on_device, int imgsz, const ys_aa_row* aa, const ys_aug_jitter* jitter, float* images, float* out_cls) {
  return aug_classify_impl("ys_augment_classify_aa", ctx, arena, srcs, n_src, src_cls, items, batch, on_device, imgsz, aa, jitter, images, out_cls);
}

// ---- the two slots on their own (augment_aa.hip): uint8 [B, 3, H, W] -> uint8, any H x W.  in and out must not overlap
extern "C" int ys_auto_augment_ops(ys_ctx* ctx, const uint8_t* in, int B, int H, int W, const ys_aa_row* rows, int on_device, uint8_t* out) {
  const char* fn = "ys_auto_augment_ops";
  YS_REQUIRE(ctx && in && rows && out, "%s: null argument", fn);
  YS_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && H <= 16384 && W <= 16384, "%s: bad shape batch=%d (1..65535) h=%d w=%d (1..16384)", fn, B, H, W);
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  AaWs aws{};
  YS_TRY(aa_reserve_ws(ctx, B, H, W, &aws));
  YsTimer timer(ctx, "auto_augment_ops");
  if (on_device) {
    YS_CHECK_HIP(hipMemsetAsync(aws.stats, 0, aws.stats_bytes, st));
    return ys_aa_slots_launch(st, in, aws.a, out, rows, B, H, W, 3, aws.stats);
  }
  int stats_mask = 0;
  YS_TRY(aa_check_rows(fn, rows, B, &stats_mask));
  const size_t n_px = (size_t)B * 3 * H * W;
  DevBuf drows;
  YS_TRY(drows.alloc((size_t)B * sizeof(ys_aa_row)));
  YS_TRY(h2d(st, aws.b, in, n_px));                        // image B of the workspace holds the input, and then the output
  YS_TRY(h2d(st, drows.p, rows, (size_t)B * sizeof(ys_aa_row)));
  if (stats_mask) YS_CHECK_HIP(hipMemsetAsync(aws.stats, 0, aws.stats_bytes, st));
  YS_TRY(ys_aa_slots_launch(st, aws.b, aws.a, aws.b, drows.as<ys_aa_row>(), B, H, W, stats_mask, aws.stats));
  YS_TRY(d2h(st, out, aws.b, n_px));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  return YS_OK;
}

// ---- ColorJitter on its own (augment.hip; Data/Augment.cs:968-987, Data/ClassificationDataset.cs:122): all four ops, uint8 or fp32 * (1 / 255.0f) out
extern "C" int ys_color_jitter(ys_ctx* ctx, const uint8_t* src, const ys_aug_jitter* jitter, int batch, int h, int w, int on_device, void* dst,
                               int dst_is_float) {
  YS_REQUIRE(ctx && src && jitter && dst, "ys_color_jitter: null argument");
  YS_REQUIRE(batch > 0 && batch <= 65535 && h > 0 && w > 0 && h <= 16384 && w <= 16384, "ys_color_jitter: bad shape batch=%d (1..65535) h=%d w=%d (1..16384)",
             batch, h, w);
  YS_CHECK_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  YS_TRY(aug_reserve_ws(ctx, batch));                      // the per-image gray sums live in the augmenter's workspace (8 bytes per image)
  YsTimer timer(ctx, "color_jitter");
  const long long n = (long long)h * w;
  if (on_device) {                                         // the host cannot read the rows: the reduction runs and leaves at once where a row has no contrast
    YS_CHECK_HIP(hipMemsetAsync(ctx->aug_ws, 0, (size_t)batch * 8, st));
    return ys_color_jitter_launch(st, src, jitter, batch, n, 1, ctx->aug_ws, dst, dst_is_float != 0);
  }
  int contrast = 0;
  YS_TRY(aug_check_jitter("ys_color_jitter", jitter, batch, 1, &contrast));
  const size_t n_px = (size_t)batch * 3 * (size_t)n, out_bytes = n_px * (dst_is_float ? 4 : 1);
  DevBuf dsrc, dj, dout;
  YS_TRY(dsrc.alloc(n_px)); YS_TRY(dj.alloc((size_t)batch * sizeof(ys_aug_jitter))); YS_TRY(dout.alloc(out_bytes));
  YS_TRY(h2d(st, dsrc.p, src, n_px));
  YS_TRY(h2d(st, dj.p, jitter, (size_t)batch * sizeof(ys_aug_jitter)));
  if (contrast) YS_CHECK_HIP(hipMemsetAsync(ctx->aug_ws, 0, (size_t)batch * 8, st));
  YS_TRY(ys_color_jitter_launch(st, (const unsigned char*)dsrc.p, (const ys_aug_jitter*)dj.p, batch, n, contrast, ctx->aug_ws, dout.p, dst_is_float != 0));
  YS_TRY(d2h(st, dst, dout.p, out_bytes));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  return YS_OK;
}
