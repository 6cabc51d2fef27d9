// augment.hip -- the training input on the device: Mosaic4 + RandomPerspective + FlipLR / FlipUD + Normalize + collate
// of the reference's default training pipeline (ImageProcessType.Mosiac, Data/YoloDataset.cs:57-151) as three kernels; RandomHSV (:86) as their epilogue.
//
//   aug_prep_kernel          one thread per output image: the four tile rectangles of Augment.Mosaic._mosaic4 (Data/Augment.cs:184-203,
//                            mask rectangles :207-209) and the inverse of the forward matrix, in double (the reference inverts in fp32 with
//                            torch.linalg.inv, :409 / :486; parity is judged against a float64 restatement; a deviation, see below).  The mask inverse is
//                            S_inv * M_inv * S -- the inverse of M_mask = S_inv * M * S (:371-376) without a second inversion.
//   aug_mosaic_warp_kernel   Mosaic4 + WarpAffine/PerspectiveWithGridSample (:395-538) + flips (:879, :936) + mul(1/255) (YoloDataset.cs:140)
//                            in one pass: a gather from the four source images with a streaming fp32 NCHW write.  The 2s x 2s canvas never
//                            exists: canvas pixel (Y, X) is 114 or a pixel of the tile whose quadrant (X >= xc, Y >= yc) it lies in.
//                            aug_mask_warp_kernel is the same for the overlap-encoded instance-id masks ([B, s/r, s/r] fp32, what
//                            ys_loss_segment reads): BILINEAR on the id bytes like the reference (:383-388), border 0.
//   aug_labels_kernel        one workgroup per image: the label filter of _mosaic4 (:238-256), apply_bboxes (:546-568), clip_boxes + area > 0
//                            (:681-692), apply_keypoints (:581-601), clip_keypoints (Utils/Ops.cs:166-183), the flips' label arithmetic
//                            (:890-891, :905, :945-946, :955), box_convert(xyxy -> cxcywh), Normalize (Data/Struct.cs:99-121) and the collate
//                            (Data/YoloDataLoader.cs:18-44) into compacted rows: a scan over the workgroup, then an exclusive scan over the B
//                            counts.  No floating-point atomics: the output is a pure function of the input.
//
// Sampling restated exactly: src = M_inv (x, y, 1) / w; valid = 0 <= src <= in - 1 on both axes (else 114 / 0); the value is
// grid_sample(bilinear, border, align_corners = false) at grid = src / (in - 1) * 2 - 1, i.e. at the position src * in / (in - 1) - 0.5 (NOT src),
// clamp(0, 255), truncation to a byte.
// DEVIATION in precision, on purpose: the inverse stays in double and the source position and the blend are evaluated in double PER PIXEL (an fp32
// inverse and fp32 pixel arithmetic would be the cheaper kernel).  That is what keeps the result closer to a float64 restatement than the reference's own
// fp32 is (see aug_blend_u8), and it has a price: measured at B = 64 / 640 px the kernel reaches 17 % of the HBM rate -- it is bound by its instruction
// stream, about 5x above the HBM estimate of its bytes (DESIGN.md "Training input on the device").
//
// Scope (include/yolosharp_hip.h lists the same): kpt_dim = 3 only (apply_keypoints reads column 2); OBB corner labels
// (xyxyxyxy2xywhr, host code in the reference) are the <true> instances of the two label kernels, see "OBB corner labels" below; RandomHSV (torchvision ColorJitter on the bytes) runs in the epilogue of the two image kernels, see "ColorJitter" below; of the no-mosaic branches the close-mosaic one (LetterBox) is built below,
// the `rand > p` one of Augment.Mosaic is not (it yields images of unequal sizes).  Deviations: a label-free
// sample is still warped (RandomPerspective.Apply returns the unwarped canvas, :666-669); where the reference's mask slice would run past the
// source mask (it throws) the kernel reads 0.
#include "ys_internal.h"
#include "ys_kernels.h"
#include "aug_jitter.h"
#include <cmath>

#define AUG_T 256

// tile i of _mosaic4 (:184-203): canvas rectangle [x1a, x2a) x [y1a, y2a), source origin (x1b, y1b)
__host__ __device__ inline void aug_tile_rect(int i, int xc, int yc, int h, int w, int s, int* x1a, int* y1a, int* x2a, int* y2a, int* x1b, int* y1b) {
  const int s2 = 2 * s;
  if (i == 0) {
    *x1a = xc - w > 0 ? xc - w : 0; *y1a = yc - h > 0 ? yc - h : 0; *x2a = xc; *y2a = yc;
    *x1b = w - (*x2a - *x1a); *y1b = h - (*y2a - *y1a);
  } else if (i == 1) {
    *x1a = xc; *y1a = yc - h > 0 ? yc - h : 0; *x2a = xc + w < s2 ? xc + w : s2; *y2a = yc;
    *x1b = 0; *y1b = h - (*y2a - *y1a);
  } else if (i == 2) {
    *x1a = xc - w > 0 ? xc - w : 0; *y1a = yc; *x2a = xc; *y2a = yc + h < s2 ? yc + h : s2;
    *x1b = w - (*x2a - *x1a); *y1b = 0;
  } else {
    *x1a = xc; *y1a = yc; *x2a = xc + w < s2 ? xc + w : s2; *y2a = yc + h < s2 ? yc + h : s2;
    *x1b = 0; *y1b = 0;
  }
}

// o = m^-1 by cofactors in double; false for a singular (or non-finite) matrix
__host__ __device__ inline bool aug_invert3(const double* m, double* o) {
  const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
  const double det = m[0] * c00 + m[1] * c01 + m[2] * c02;
  // singular = the three terms of the expansion cancel (or vanish): |det| against the sum of their magnitudes, which carries the matrix's own scale --
  // a translation of thousands of pixels does not turn a sound matrix into a "singular" one
  const double t0 = m[0] * c00, t1 = m[1] * c01, t2 = m[2] * c02;
  const double mag = (t0 < 0 ? -t0 : t0) + (t1 < 0 ? -t1 : t1) + (t2 < 0 ? -t2 : t2);
  const double ad = det < 0 ? -det : det;
  if (!(ad > 1e-12 * mag) || !(ad < 1e300)) return false;
  const double r = 1.0 / det;
  o[0] = c00 * r; o[1] = (m[2] * m[7] - m[1] * m[8]) * r; o[2] = (m[1] * m[5] - m[2] * m[4]) * r;
  o[3] = c01 * r; o[4] = (m[0] * m[8] - m[2] * m[6]) * r; o[5] = (m[2] * m[3] - m[0] * m[5]) * r;
  o[6] = c02 * r; o[7] = (m[1] * m[6] - m[0] * m[7]) * r; o[8] = (m[0] * m[4] - m[1] * m[3]) * r;
  return true;
}

// the matrix the warp inverts: M itself (perspective form, :364) or its first two rows over (0, 0, 1) (affine form, :368, :479-486)
__host__ __device__ inline void aug_warp_matrix(const float* M, int perspective, double* m) {
  for (int i = 0; i < 9; i++) m[i] = (double)M[i];
  if (!perspective) { m[6] = 0.0; m[7] = 0.0; m[8] = 1.0; }
}

// an item the kernels can run: sources in range, centre inside the canvas, invertible matrix
__host__ __device__ inline int aug_item_ok(const ys_aug_item& it, const ys_aug_src* srcs, int n_src, int s, int perspective) {
  for (int i = 0; i < 4; i++) {
    if (it.src[i] < 0 || it.src[i] >= n_src) return 0;
    const ys_aug_src& sr = srcs[it.src[i]];
    if (sr.h < 1 || sr.w < 1 || sr.img_off < 0) return 0;
  }
  if (it.xc < 0 || it.xc > 2 * s || it.yc < 0 || it.yc > 2 * s) return 0;
  double m[9], o[9];
  aug_warp_matrix(it.M, perspective, m);
  return aug_invert3(m, o) ? 1 : 0;
}

__global__ void __launch_bounds__(64)
aug_prep_kernel(const ys_aug_src* __restrict__ srcs, int n_src, const ys_aug_item* __restrict__ items, int B, int s, int r, int perspective,
                AugParams* __restrict__ params) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const ys_aug_item it = items[b];
  AugParams P;
  P.valid = aug_item_ok(it, srcs, n_src, s, perspective);
  P.xc = it.xc; P.yc = it.yc; P.flip_lr = it.flip_lr != 0; P.flip_ud = it.flip_ud != 0;
  P.pad_ = 0;
  for (int i = 0; i < 9; i++) { P.inv[i] = (i % 4 == 0) ? 1.0 : 0.0; P.minv[i] = P.inv[i]; }
  for (int i = 0; i < 4; i++) {
    AugTile& t = P.t[i];
    t.img_off = 0; t.mask_off = -1; t.h = 0; t.w = 0; t.mh = 0; t.mw = 0; t.padw = 0; t.padh = 0;     // a refused item: every canvas pixel is 114, nothing is read
    t.mx1a = t.my1a = t.mx2a = t.my2a = t.mx1b = t.my1b = 0;
  }
  if (P.valid) {
    double m[9];
    aug_warp_matrix(it.M, perspective, m);
    aug_invert3(m, P.inv);
    const double rr = (double)r;
    for (int i = 0; i < 9; i++) P.minv[i] = P.inv[i];
    P.minv[2] /= rr; P.minv[5] /= rr; P.minv[6] *= rr; P.minv[7] *= rr;                                // S_inv * M_inv * S, S = diag(r, r, 1)
    for (int i = 0; i < 4; i++) {
      const ys_aug_src sr = srcs[it.src[i]];
      AugTile& t = P.t[i];
      int x1a, y1a, x2a, y2a, x1b, y1b;
      aug_tile_rect(i, it.xc, it.yc, sr.h, sr.w, s, &x1a, &y1a, &x2a, &y2a, &x1b, &y1b);
      t.img_off = sr.img_off; t.mask_off = sr.mask_off; t.h = sr.h; t.w = sr.w; t.mh = sr.mh; t.mw = sr.mw;
      t.padw = x1a - x1b; t.padh = y1a - y1b;
      t.mx1a = x1a / r; t.my1a = y1a / r; t.mx2a = x2a / r; t.my2a = y2a / r; t.mx1b = x1b / r; t.my1b = y1b / r;
    }
  }
  params[b] = P;
}

// source position of output pixel (x, y): inv * (x, y, 1), divided by w in the perspective form (in the affine form w is exactly 1)
__device__ __forceinline__ void aug_src_pos(const double* inv, int perspective, int x, int y, double* sx, double* sy) {
  const double dx = (double)x, dy = (double)y;
  double X = fma(inv[0], dx, fma(inv[1], dy, inv[2]));
  double Y = fma(inv[3], dx, fma(inv[4], dy, inv[5]));
  if (perspective) {
    const double W = fma(inv[6], dx, fma(inv[7], dy, inv[8]));
    X /= W; Y /= W;
  }
  *sx = X; *sy = Y;
}

// grid_sample's bilinear set-up on an in x in input at source position (X, Y) (valid, i.e. inside [0, in - 1]): the four corner indices
// (clamped: a corner past the edge has weight 0) and the two fractions, in double
__device__ __forceinline__ void aug_bilinear(double X, double Y, int in, int* x0, int* y0, int* x1, int* y1, double* wx, double* wy) {
  const double k = (double)in / (double)(in - 1);
  double ix = X * k - 0.5, iy = Y * k - 0.5;
  const double hi = (double)(in - 1);
  ix = ix < 0.0 ? 0.0 : (ix > hi ? hi : ix);
  iy = iy < 0.0 ? 0.0 : (iy > hi ? hi : iy);
  const double fx = floor(ix), fy = floor(iy);
  *wx = ix - fx; *wy = iy - fy;
  *x0 = (int)fx; *y0 = (int)fy;
  *x1 = *x0 + 1 < in ? *x0 + 1 : in - 1;
  *y1 = *y0 + 1 < in ? *y0 + 1 : in - 1;
}

// the blend, clamp(0, 255) and the truncation to uint8 (:454, :529).  ATen sums nw * (1-wy)(1-wx) + ne * (1-wy) wx + sw * wy (1-wx) + se * wy wx; four
// rounded weights need not sum to 1, so that form returns 113.99999 -> 113 for some pixels of a constant 114 region, and WHICH pixels depends on the
// last bits of the weights (the float32 and float64 restatements disagree on 2-10 % of the bytes of an image with large fill regions for this reason
// alone).  The nested interpolation in double is exact on constant regions and within 1e-13 levels of the real value elsewhere: the kernel adds no
// truncation flips of its own to those of whatever it is compared with.
__device__ __forceinline__ float aug_blend_u8(float a, float b, float c, float d, double wx, double wy) {
  const double top = (double)a + wx * ((double)b - (double)a), bot = (double)c + wx * ((double)d - (double)c);
  double v = top + wy * (bot - top);
  v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);
  return (float)(int)v;
}

// the four tiles' geometry as wave-uniform scalars; a canvas pixel picks its tile with two comparisons and three selects per field
// (passed as SCALARS: selects between the fields of a struct in memory are turned into an indexed load by hipcc, which then parks the struct in LDS)
#define AUG_T4_PARAMS int w0, int w1, int w2, int w3, int h0, int h1, int h2, int h3, long long off0, long long off1, long long off2, long long off3, int xc, int yc
#define AUG_T4_ARGS w0, w1, w2, w3, h0, h1, h2, h3, off0, off1, off2, off3, xc, yc

__device__ __forceinline__ void aug_canvas_fetch(const unsigned char* __restrict__ arena, AUG_T4_PARAMS, int X, int Y, float* v) {
  const bool right = X >= xc, bottom = Y >= yc;
  const int w = right ? (bottom ? w3 : w1) : (bottom ? w2 : w0);
  const int h = right ? (bottom ? h3 : h1) : (bottom ? h2 : h0);
  const long long off = right ? (bottom ? off3 : off1) : (bottom ? off2 : off0);
  // tile 0 / 2: x1a = max(xc - w, 0), x1b = w - (xc - x1a) -> source column X - xc + w; tile 1 / 3: X - xc.  Inside the rectangle <=> 0 <= column < w
  const int px = X - xc + (right ? 0 : w), py = Y - yc + (bottom ? 0 : h);
  if ((unsigned)px < (unsigned)w && (unsigned)py < (unsigned)h) {
    const long long plane = (long long)h * w;
    const unsigned char* p = arena + off + (long long)py * w + px;
    v[0] = (float)p[0]; v[1] = (float)p[plane]; v[2] = (float)p[2 * plane];
  } else {
    v[0] = 114.0f; v[1] = 114.0f; v[2] = 114.0f;
  }
}

// ColorJitter (RandomHSV): AugPx, aug_jitter_state, the aug_jit_* ops and aug_jitter_quad live in aug_jitter.h (augment_cls.hip runs them too)

// one output pixel (logical coordinates after the flips): three channels as bytes in fp32
__device__ __forceinline__ AugPx aug_pixel(const unsigned char* __restrict__ arena, AUG_T4_PARAMS, const double* __restrict__ inv, int perspective, int in,
                                           bool live, int lx, int ly) {
  float b0 = 114.0f, b1 = 114.0f, b2 = 114.0f;
  double X, Y;
  aug_src_pos(inv, perspective, lx, ly, &X, &Y);
  const double hi = (double)(in - 1);
  if (live && X >= 0.0 && X <= hi && Y >= 0.0 && Y <= hi) {
    int xa, ya, xb, yb; double wx, wy;
    aug_bilinear(X, Y, in, &xa, &ya, &xb, &yb, &wx, &wy);
    float nw[3], ne[3], sw[3], se[3];
    aug_canvas_fetch(arena, AUG_T4_ARGS, xa, ya, nw);
    aug_canvas_fetch(arena, AUG_T4_ARGS, xb, ya, ne);
    aug_canvas_fetch(arena, AUG_T4_ARGS, xa, yb, sw);
    aug_canvas_fetch(arena, AUG_T4_ARGS, xb, yb, se);
    b0 = aug_blend_u8(nw[0], ne[0], sw[0], se[0], wx, wy);
    b1 = aug_blend_u8(nw[1], ne[1], sw[1], se[1], wx, wy);
    b2 = aug_blend_u8(nw[2], ne[2], sw[2], se[2], wx, wy);
  }
  AugPx r; r.c0 = b0; r.c1 = b1; r.c2 = b2;
  return r;
}

// one thread: 4 consecutive x of one output row, three channels -> three 16-byte stores (vec: s % 4 == 0, rows 16-byte aligned)
__global__ void __launch_bounds__(AUG_T)
aug_mosaic_warp_kernel(const unsigned char* __restrict__ arena, const AugParams* __restrict__ params, const ys_aug_jitter* __restrict__ jitter, int s,
                       int perspective, int vec, float* __restrict__ images) {
  const AugParams& P = params[blockIdx.z];
  // the image's jitter row (wave-uniform; NULL = none).  A row that is invalid or asks for contrast (the mean needs the whole image first) refuses
  // the image like a refused item: all 114, not jittered
  const ys_aug_jitter* __restrict__ J = jitter ? jitter + blockIdx.z : nullptr;
  const int jstate = J ? aug_jitter_state(*J) : 1;
  const bool refused = jstate != 1;
  const int qpr = (s + 3) >> 2;
  const unsigned i = blockIdx.x * AUG_T + threadIdx.x;
  if (i >= (unsigned)qpr * (unsigned)s) return;
  const int y = (int)(i / (unsigned)qpr), x0 = (int)(i - (unsigned)y * (unsigned)qpr) * 4;
  const int w0 = P.t[0].w, w1 = P.t[1].w, w2 = P.t[2].w, w3 = P.t[3].w, h0 = P.t[0].h, h1 = P.t[1].h, h2 = P.t[2].h, h3 = P.t[3].h;
  const long long off0 = P.t[0].img_off, off1 = P.t[1].img_off, off2 = P.t[2].img_off, off3 = P.t[3].img_off;
  const int xc = P.xc, yc = P.yc;
  const double* __restrict__ inv = P.inv;                 // wave-uniform: scalar loads
  const int in = 2 * s;
  // the flips are folded into the output coordinate: out[y][x] = warped[ly][lx]
  const int ly = P.flip_ud ? s - 1 - y : y;
  const int lx0 = P.flip_lr ? s - 1 - x0 : x0, dx = P.flip_lr ? -1 : 1;
  AugPx p0 = aug_pixel(arena, AUG_T4_ARGS, inv, perspective, in, !refused && x0 < s, lx0, ly);
  AugPx p1 = aug_pixel(arena, AUG_T4_ARGS, inv, perspective, in, !refused && x0 + 1 < s, lx0 + dx, ly);
  AugPx p2 = aug_pixel(arena, AUG_T4_ARGS, inv, perspective, in, !refused && x0 + 2 < s, lx0 + 2 * dx, ly);
  AugPx p3 = aug_pixel(arena, AUG_T4_ARGS, inv, perspective, in, !refused && x0 + 3 < s, lx0 + 3 * dx, ly);
  if (J && !refused) aug_jitter_quad(J, 0.0f, false, p0, p1, p2, p3);
  const float q = 1 / 255.0f;                             // mul(1 / 255.0f), YoloDataset.cs:140: a multiply, bit-exact per byte
  p0.c0 *= q; p0.c1 *= q; p0.c2 *= q; p1.c0 *= q; p1.c1 *= q; p1.c2 *= q; p2.c0 *= q; p2.c1 *= q; p2.c2 *= q; p3.c0 *= q; p3.c1 *= q; p3.c2 *= q;
  const long long plane = (long long)s * s;
  float* dst = images + (long long)blockIdx.z * 3 * plane + (long long)y * s + x0;
  if (vec) {
    ys_st16(dst, make_uint4(ys_f2u(p0.c0), ys_f2u(p1.c0), ys_f2u(p2.c0), ys_f2u(p3.c0)));
    ys_st16(dst + plane, make_uint4(ys_f2u(p0.c1), ys_f2u(p1.c1), ys_f2u(p2.c1), ys_f2u(p3.c1)));
    ys_st16(dst + 2 * plane, make_uint4(ys_f2u(p0.c2), ys_f2u(p1.c2), ys_f2u(p2.c2), ys_f2u(p3.c2)));
  } else {
    if (x0 < s) { dst[0] = p0.c0; dst[plane] = p0.c1; dst[2 * plane] = p0.c2; }
    if (x0 + 1 < s) { dst[1] = p1.c0; dst[plane + 1] = p1.c1; dst[2 * plane + 1] = p1.c2; }
    if (x0 + 2 < s) { dst[2] = p2.c0; dst[plane + 2] = p2.c1; dst[2 * plane + 2] = p2.c2; }
    if (x0 + 3 < s) { dst[3] = p3.c0; dst[plane + 3] = p3.c1; dst[2 * plane + 3] = p3.c2; }
  }
}

// mask canvas pixel (Y, X) of the (2s / r)^2 id canvas: 0, or the byte of the tile whose rectangle (bounds / r, :207-209) holds it
__device__ inline float aug_mask_fetch(const unsigned char* __restrict__ arena, const AugParams& P, int r, int X, int Y) {
  const int q = (Y >= P.yc / r ? 2 : 0) + (X >= P.xc / r ? 1 : 0);
  const AugTile& t = P.t[q];
  if (t.mask_off < 0 || X < t.mx1a || X >= t.mx2a || Y < t.my1a || Y >= t.my2a) return 0.0f;
  const int px = X - t.mx1a + t.mx1b, py = Y - t.my1a + t.my1b;
  if (px >= t.mw || py >= t.mh) return 0.0f;              // past the source mask: the reference's slice assignment throws here
  return (float)arena[t.mask_off + (long long)py * t.mw + px];
}

__global__ void __launch_bounds__(AUG_T)
aug_mask_warp_kernel(const unsigned char* __restrict__ arena, const AugParams* __restrict__ params, int s, int r, int perspective,
                     float* __restrict__ masks) {
  const AugParams& P = params[blockIdx.z];
  const int ms = s / r, in = 2 * s / r;
  const unsigned i = blockIdx.x * AUG_T + threadIdx.x;
  if (i >= (unsigned)ms * (unsigned)ms) return;
  const int y = (int)(i / (unsigned)ms), x = (int)(i - (unsigned)y * (unsigned)ms);
  const int lx = P.flip_lr ? ms - 1 - x : x, ly = P.flip_ud ? ms - 1 - y : y;
  const double* __restrict__ inv = P.minv;
  double X, Y;
  aug_src_pos(inv, perspective, lx, ly, &X, &Y);
  const double hi = (double)(in - 1);
  float v = 0.0f;
  if (X >= 0.0 && X <= hi && Y >= 0.0 && Y <= hi) {
    int xa, ya, xb, yb; double wx, wy;
    aug_bilinear(X, Y, in, &xa, &ya, &xb, &yb, &wx, &wy);
    v = aug_blend_u8(aug_mask_fetch(arena, P, r, xa, ya), aug_mask_fetch(arena, P, r, xb, ya), aug_mask_fetch(arena, P, r, xa, yb),
                     aug_mask_fetch(arena, P, r, xb, yb), wx, wy);
  }
  masks[(long long)blockIdx.z * ms * ms + i] = v;
}

// ---------------------------------------------------------------------------------------------------------------- labels
struct AugLabelOut { float cls, box[4]; };

// label l of tile (padw, padh) through the two filters and the matrix; returns the keep decision, fills the cxcywh / s row
__device__ inline bool aug_label_box(const float* __restrict__ boxes, int l, float padw, float padh, const float* M, int s, int perspective, int flip_lr,
                                     int flip_ud, int sort_flipped, float* out) {
  const float S2 = (float)(2 * s), S = (float)s;
  float x1 = boxes[4 * l + 0] + padw, y1 = boxes[4 * l + 1] + padh, x2 = boxes[4 * l + 2] + padw, y2 = boxes[4 * l + 3] + padh;
  const float org_area = (x2 - x1) * (y2 - y1);
  x1 = fminf(fmaxf(x1, 0.0f), S2); y1 = fminf(fmaxf(y1, 0.0f), S2); x2 = fminf(fmaxf(x2, 0.0f), S2); y2 = fminf(fmaxf(y2, 0.0f), S2);
  const float area = (x2 - x1) * (y2 - y1);
  bool keep = area > 0.0f && area > 0.7f * org_area;                              // :245
  // apply_bboxes (:557-566): corners x1y1, x2y2, x1y2, x2y1 through M, divide only when perspective > 0, min / max
  const float cx[4] = {x1, x2, x1, x2}, cy[4] = {y1, y2, y2, y1};
  float xmin = 0.f, xmax = 0.f, ymin = 0.f, ymax = 0.f;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    float px = (cx[k] * M[0] + cy[k] * M[1]) + M[2], py = (cx[k] * M[3] + cy[k] * M[4]) + M[5];
    if (perspective) { const float pw = (cx[k] * M[6] + cy[k] * M[7]) + M[8]; px /= pw; py /= pw; }
    xmin = k == 0 ? px : fminf(xmin, px); xmax = k == 0 ? px : fmaxf(xmax, px);
    ymin = k == 0 ? py : fminf(ymin, py); ymax = k == 0 ? py : fmaxf(ymax, py);
  }
  xmin = fminf(fmaxf(xmin, 0.0f), S); ymin = fminf(fmaxf(ymin, 0.0f), S); xmax = fminf(fmaxf(xmax, 0.0f), S); ymax = fminf(fmaxf(ymax, 0.0f), S);
  keep = keep && (xmax - xmin) * (ymax - ymin) > 0.0f;                            // :683-684
  // FlipLR / FlipUD as written (:890-891, :945-946): columns 0 and 2 (1 and 3) become s - x, NOT swapped -> a flipped box has x1 > x2
  if (flip_lr) { xmin = S - xmin; xmax = S - xmax; }
  if (flip_ud) { ymin = S - ymin; ymax = S - ymax; }
  if (sort_flipped) {
    const float a = fminf(xmin, xmax), b = fmaxf(xmin, xmax), c = fminf(ymin, ymax), d = fmaxf(ymin, ymax);
    xmin = a; xmax = b; ymin = c; ymax = d;
  }
  const float inv = 1.0f / S;                                                     // Normalize: mul by 1f / w (Struct.cs:107-110)
  out[0] = ((xmin + xmax) / 2.0f) * inv; out[1] = ((ymin + ymax) / 2.0f) * inv; out[2] = (xmax - xmin) * inv; out[3] = (ymax - ymin) * inv;
  return keep;
}

// keypoints [K][3] of label l: + pad, apply_keypoints (always divides; visibility 0 outside [0, s]), clip_keypoints, flips, / s
__device__ inline void aug_label_kpts(const float* __restrict__ kin, int K, float padw, float padh, const float* M, int s, int flip_lr, int flip_ud,
                                      float* __restrict__ kout) {
  const float S = (float)s, inv = 1.0f / S;
  for (int k = 0; k < K; k++) {
    const float x = kin[3 * k] + padw, y = kin[3 * k + 1] + padh;
    float vis = kin[3 * k + 2];
    const float pw = (x * M[6] + y * M[7]) + M[8];
    float px = ((x * M[0] + y * M[1]) + M[2]) / pw, py = ((x * M[3] + y * M[4]) + M[5]) / pw;
    if (px < 0.0f || py < 0.0f || px > S || py > S) vis = 0.0f;                   // :597-598 and Ops.cs:173-178: the same test twice
    px = fminf(fmaxf(px, 0.0f), S); py = fminf(fmaxf(py, 0.0f), S);
    if (flip_lr) px = S - px;
    if (flip_ud) py = S - py;
    kout[3 * k] = px * inv; kout[3 * k + 1] = py * inv; kout[3 * k + 2] = vis;
  }
}

// ---------------------------------------------------------------------------------------------------------------- OBB corner labels
// xyxyxyxy2xywhr (Utils/Ops.cs:44-54) is OpenCV MinAreaRect of a label's four corners, host code in the reference (YoloDataset.GetTensor, :110-129).
// Here: the enclosing rectangle of minimum area of four points, without a hull and without indexed private arrays.  The minimum-area rectangle has a
// side collinear with a hull edge; every hull edge is one of the 6 point pairs; the bounding rectangle along any OTHER pair's direction still encloses
// the points -- so the minimum over the 6 pair directions is the answer.  Zero-length pairs are skipped.  6 directions x 3 projections (the points are
// taken relative to point 0), unrolled, everything in registers.
//   pair order: (0,1) (1,2) (2,3) (3,0) (0,2) (1,3); the FIRST strict minimum of the area wins: the row is a pure function of the input.
//   canonical form (OpenCV >= 4.5.1's documented one; the reference pins OpenCvSharp 4.11): a pair's direction is folded by quarter turns -- exact: swaps
//   and sign changes -- into u = (ux >= 0, uy > 0); angle = atan2(uy, ux) in (0, pi/2], w = the extent along u, h = the extent along its normal.  An
//   axis-aligned rectangle is angle = pi/2 with (w, h) = (y extent, x extent), never angle = 0.  A rectangle has one such representative.
//   precision: the inputs are fp32, everything from the differences to atan2 is double, the five results are rounded to fp32 once.  Products of two
//   fp32 values are exact in double, so exactly collinear points on a border (the clipped case) give an extent of exactly 0, whole-number inputs give
//   exact areas (ties between the parallel edges of a rectangle are exact ties, whatever corner the list starts at), and the rounding of the
//   direction never decides between two candidates that differ by more than 1e-15 relative.  One thread per label: the cost is nothing.
//   degenerate inputs, finite rows: four identical points give (x, y, 0, 0, 0).  Exactly collinear points (two distinct points included) give
//   w = the span, h = 0 and the line's OWN direction folded by half turns into (0, pi]: the one kind of row whose angle can exceed pi/2 (a line in
//   the second quadrant; a horizontal one is pi).  A quarter-turn fold cannot name such a segment with w as its span -- (span, 0, angle - pi/2) is
//   the segment turned by 90 degrees -- and the row must describe the points it encloses.  DEVIATION: OpenCV leaves the raw atan2 of the line, in
//   (-pi, pi], there.
// UNPINNED: OpenCV is not available to the tests; the choice among geometrically different rectangles of EQUAL area (an acute triangle: all three
// edges tie exactly; many quads clipped to the image) is this file's pair order, not pinned against the reference binary.
struct AugRect { double area, w, h, cx, cy, ang; };

// the candidate along the pair a -> b (coordinates relative to point 0, which is the origin; 1..3 the other points)
__device__ __forceinline__ void aug_rect_pair(double ax, double ay, double bx, double by, double x1, double y1, double x2, double y2, double x3, double y3,
                                              bool& any, AugRect& best) {
  double ux = bx - ax, uy = by - ay;
  if (ux == 0.0 && uy == 0.0) return;
  if (uy < 0.0 || (uy == 0.0 && ux < 0.0)) { ux = -ux; uy = -uy; }                   // the upper half plane, +x axis included
  if (uy == 0.0) { uy = ux; ux = 0.0; }                                              // +x axis: a quarter turn forward -> pi/2
  else if (ux < 0.0) { const double t = ux; ux = uy; uy = -t; }                      // second quadrant: a quarter turn back
  // projections on u and on n = (-uy, ux), unnormalised; point 0 projects to (0, 0)
  const double t1 = x1 * ux + y1 * uy, t2 = x2 * ux + y2 * uy, t3 = x3 * ux + y3 * uy;
  const double m1 = y1 * ux - x1 * uy, m2 = y2 * ux - x2 * uy, m3 = y3 * ux - x3 * uy;
  const double tlo = fmin(fmin(0.0, t1), fmin(t2, t3)), thi = fmax(fmax(0.0, t1), fmax(t2, t3));
  const double mlo = fmin(fmin(0.0, m1), fmin(m2, m3)), mhi = fmax(fmax(0.0, m1), fmax(m2, m3));
  const double len2 = ux * ux + uy * uy;
  const double area = ((thi - tlo) * (mhi - mlo)) / len2;
  if (any && !(area < best.area)) return;
  const double len = sqrt(len2), tc = (tlo + thi) / 2.0, mc = (mlo + mhi) / 2.0;
  any = true;
  best.area = area; best.w = (thi - tlo) / len; best.h = (mhi - mlo) / len;
  best.cx = (tc * ux - mc * uy) / len2; best.cy = (tc * uy + mc * ux) / len2;
  best.ang = atan2(uy, ux);
}

// c = x0 y0 x1 y1 x2 y2 x3 y3 (constant indices only) -> out = cx, cy, w, h (the units of c), angle (radians)
__device__ inline void aug_min_area_rect(const float* c, float* out) {
  const double ox = (double)c[0], oy = (double)c[1];
  const double x1 = (double)c[2] - ox, y1 = (double)c[3] - oy, x2 = (double)c[4] - ox, y2 = (double)c[5] - oy, x3 = (double)c[6] - ox, y3 = (double)c[7] - oy;
  bool any = false;
  AugRect r;
  r.area = 0.0; r.w = 0.0; r.h = 0.0; r.cx = 0.0; r.cy = 0.0; r.ang = 0.0;           // four identical points
  aug_rect_pair(0.0, 0.0, x1, y1, x1, y1, x2, y2, x3, y3, any, r);
  aug_rect_pair(x1, y1, x2, y2, x1, y1, x2, y2, x3, y3, any, r);
  aug_rect_pair(x2, y2, x3, y3, x1, y1, x2, y2, x3, y3, any, r);
  aug_rect_pair(x3, y3, 0.0, 0.0, x1, y1, x2, y2, x3, y3, any, r);
  aug_rect_pair(0.0, 0.0, x2, y2, x1, y1, x2, y2, x3, y3, any, r);
  aug_rect_pair(x1, y1, x3, y3, x1, y1, x2, y2, x3, y3, any, r);
  if (r.w == 0.0 && r.h != 0.0) { r.w = r.h; r.h = 0.0; r.ang += 1.5707963267948966; }   // exactly collinear along the normal: w = the span, the line's direction
  out[0] = (float)(ox + r.cx); out[1] = (float)(oy + r.cy); out[2] = (float)r.w; out[3] = (float)r.h; out[4] = (float)r.ang;
}

// corners [4][2] of one label -> the criterion's row (cx / s, cy / s, w / s, h / s, angle), fp32 in the reference's order: + pad; warp (the Mosaic
// branch): apply_obb_corners (Augment.cs:604-635: (x, y, 1) . M^T, divided by the third component only when perspective > 0 -- apply_keypoints always
// divides) and clip_obb_corners (Utils/Ops.cs:191-199: clamp to [0, s]); FlipLR x <- s - x, FlipUD y <- s - y (:908-911, :958-961); the rectangle;
// columns 0-3 DIVIDED by s (YoloDataset.cs:121: a division, not mul(1 / s)).  _mosaic4 does not clip the corners to the canvas (:253-256).
__device__ inline void aug_label_obb(const float* __restrict__ cin, float padw, float padh, bool warp, const float* M, int s, int perspective, int flip_lr,
                                     int flip_ud, float* out) {
  const float S = (float)s;
  float c[8];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    float x = cin[2 * k] + padw, y = cin[2 * k + 1] + padh;
    if (warp) {
      float px = (x * M[0] + y * M[1]) + M[2], py = (x * M[3] + y * M[4]) + M[5];
      if (perspective) { const float pw = (x * M[6] + y * M[7]) + M[8]; px /= pw; py /= pw; }
      x = fminf(fmaxf(px, 0.0f), S); y = fminf(fmaxf(py, 0.0f), S);
    }
    if (flip_lr) x = S - x;
    if (flip_ud) y = S - y;
    c[2 * k] = x; c[2 * k + 1] = y;
  }
  aug_min_area_rect(c, out);
  out[0] = out[0] / S; out[1] = out[1] / S; out[2] = out[2] / S; out[3] = out[3] / S;
}

// ys_xyxyxyxy2xywhr: the operator on its own, one thread per row, pixels in, pixels and radians out
__global__ void __launch_bounds__(AUG_T)
aug_xyxyxyxy2xywhr_kernel(const float* __restrict__ corners, int n, float* __restrict__ out) {
  const int i = blockIdx.x * AUG_T + threadIdx.x;
  if (i >= n) return;
  float c[8], r[5];
#pragma unroll
  for (int k = 0; k < 8; k++) c[k] = corners[8 * (long long)i + k];
  aug_min_area_rect(c, r);
#pragma unroll
  for (int k = 0; k < 5; k++) out[5 * (long long)i + k] = r[k];
}

// offs[b] = counts[0] + ... + counts[b - 1], offs[B] = the total: one workgroup, chunks of AUG_T with a carry (Hillis-Steele in LDS, fixed order)
__global__ void __launch_bounds__(AUG_T)
aug_count_scan_kernel(const int* __restrict__ counts, int B, int* __restrict__ offs) {
  __shared__ int s_scan[AUG_T];
  const int tid = threadIdx.x;
  int carry = 0;
  for (int k0 = 0; k0 < B; k0 += AUG_T) {
    const int k = k0 + tid;
    const int c = k < B ? counts[k] : 0;
    s_scan[tid] = c;
    __syncthreads();
    for (int d = 1; d < AUG_T; d <<= 1) {
      const int v = tid >= d ? s_scan[tid - d] : 0;
      __syncthreads();
      s_scan[tid] += v;
      __syncthreads();
    }
    if (k < B) offs[k] = carry + s_scan[tid] - c;
    carry += s_scan[AUG_T - 1];
    __syncthreads();
  }
  if (tid == 0) offs[B] = carry;
}

// pass 0: counts[b] = kept labels of image b.  pass 1: rows [base(b), base(b) + counts[b]) with base = the exclusive scan of counts (counts[B + b], written by aug_count_scan_kernel between the passes), the tail
// [total, capacity) = (batch_idx -1, zeros), *out_count = total (a total above capacity is reported as it is; rows past capacity are not written).
// OBB: kpts holds the labels' corners [n][4][2] instead, o_box has 5 columns (aug_label_obb) and o_kpt is NULL; `boxes` alone decides what is kept.
template <bool OBB>
__global__ void __launch_bounds__(AUG_T)
aug_labels_kernel(const ys_aug_src* __restrict__ srcs, int n_src, const int* __restrict__ lab_off, const float* __restrict__ cls,
                  const float* __restrict__ boxes, const float* __restrict__ kpts, int K, const ys_aug_item* __restrict__ items, int B, int s,
                  int perspective, int flags, int capacity, int pass, int* __restrict__ counts, float* __restrict__ o_bidx, float* __restrict__ o_cls,
                  float* __restrict__ o_box, float* __restrict__ o_kpt, int* __restrict__ o_count) {
  __shared__ int s_scan[AUG_T];
  __shared__ int s_n[4], s_first[4], s_padw[4], s_padh[4];
  __shared__ int s_base, s_total;
  const int b = blockIdx.x, tid = threadIdx.x;
  const ys_aug_item it = items[b];
  if (tid < 4) {
    int n = 0, first = 0, padw = 0, padh = 0;
    if (aug_item_ok(it, srcs, n_src, s, perspective)) {
      const int sr = it.src[tid];
      first = lab_off[sr]; n = lab_off[sr + 1] - first;
      int x1a, y1a, x2a, y2a, x1b, y1b;
      aug_tile_rect(tid, it.xc, it.yc, srcs[sr].h, srcs[sr].w, s, &x1a, &y1a, &x2a, &y2a, &x1b, &y1b);
      padw = x1a - x1b; padh = y1a - y1b;
    }
    s_n[tid] = n > 0 ? n : 0; s_first[tid] = first; s_padw[tid] = padw; s_padh[tid] = padh;
  }
  if (tid == 0 && pass == 1) { s_base = counts[B + b]; s_total = counts[2 * B]; }      // aug_count_scan_kernel's offsets
  __syncthreads();
  const int c0 = s_n[0], c1 = c0 + s_n[1], c2 = c1 + s_n[2], n_img = c2 + s_n[3];
  float M[9];
#pragma unroll
  for (int k = 0; k < 9; k++) M[k] = it.M[k];
  int done = 0;                                                                    // kept labels of the chunks before this one
  for (int j0 = 0; j0 < n_img; j0 += AUG_T) {
    const int j = j0 + tid;
    bool keep = false;
    int l = 0, t = 0;
    float row[4] = {0.f, 0.f, 0.f, 0.f};
    if (j < n_img) {
      t = j < c0 ? 0 : (j < c1 ? 1 : (j < c2 ? 2 : 3));
      l = s_first[t] + j - (t == 0 ? 0 : (t == 1 ? c0 : (t == 2 ? c1 : c2)));
      keep = aug_label_box(boxes, l, (float)s_padw[t], (float)s_padh[t], M, s, perspective, it.flip_lr != 0, it.flip_ud != 0,
                           (flags & YS_AUG_SORT_FLIPPED) != 0, row);
    }
    // inclusive scan of the keep flags over the workgroup (Hillis-Steele in LDS: a fixed order, 8 steps)
    s_scan[tid] = keep ? 1 : 0;
    __syncthreads();
    for (int d = 1; d < AUG_T; d <<= 1) {
      const int v = tid >= d ? s_scan[tid - d] : 0;
      __syncthreads();
      s_scan[tid] += v;
      __syncthreads();
    }
    const int rank = done + s_scan[tid] - 1;
    const int chunk = s_scan[AUG_T - 1];
    if (pass == 1 && keep) {
      const long long rowi = (long long)s_base + rank;
      if (rowi < capacity) {
        o_bidx[rowi] = (float)b; o_cls[rowi] = cls[l];
        if constexpr (OBB) {
          float r5[5];
          aug_label_obb(kpts + 8 * (long long)l, (float)s_padw[t], (float)s_padh[t], true, M, s, perspective, it.flip_lr != 0, it.flip_ud != 0, r5);
#pragma unroll
          for (int k = 0; k < 5; k++) o_box[5 * rowi + k] = r5[k];
        } else {
          o_box[4 * rowi] = row[0]; o_box[4 * rowi + 1] = row[1]; o_box[4 * rowi + 2] = row[2]; o_box[4 * rowi + 3] = row[3];
          if (o_kpt) aug_label_kpts(kpts + (long long)l * K * 3, K, (float)s_padw[t], (float)s_padh[t], M, s, it.flip_lr != 0, it.flip_ud != 0,
                                    o_kpt + rowi * K * 3);
        }
      }
    }
    done += chunk;
    __syncthreads();
  }
  if (pass == 0) {
    if (tid == 0) counts[b] = done;
    return;
  }
  if (b == 0 && tid == 0) *o_count = s_total;
  for (long long rowi = (long long)s_total + (long long)b * AUG_T + tid; rowi < capacity; rowi += (long long)B * AUG_T) {
    o_bidx[rowi] = -1.0f; o_cls[rowi] = 0.0f;
    if constexpr (OBB) {
#pragma unroll
      for (int k = 0; k < 5; k++) o_box[5 * rowi + k] = 0.f;
    } else {
      o_box[4 * rowi] = 0.f; o_box[4 * rowi + 1] = 0.f; o_box[4 * rowi + 2] = 0.f; o_box[4 * rowi + 3] = 0.f;
      if (o_kpt) for (int k = 0; k < K * 3; k++) o_kpt[rowi * K * 3 + k] = 0.f;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- LetterBox branch
// The close-mosaic training input (YoloDataset.CloseMosaic(true), Data/YoloDataset.cs:378-429; also ImageProcessType.Letterbox, :70-74):
// LetterBox(s, s, mask_ratio) (Data/Augment.cs:698-778) + FlipLR / FlipUD (:860-966) + mul(1/255) + collate, on src[0] of an item alone.
//
//   aug_letterbox_kernel<3>       LetterboxImage (:756-777) of the image: nearest resize (the rule of letterbox_kernel, elementwise.hip) into the
//                                 window [pad_u, pad_u + new_h) x [pad_l, pad_l + new_w), 114 elsewhere, flips folded into the output coordinate,
//                                 byte * (1 / 255.0f): a pure gather, nothing is blended, so the output is bit-exact against a restatement.
//                                 ratio == 1 -- the loader has resized the long side to s -- takes no division and reads a quad's four
//                                 consecutive source bytes as aligned words, at any arena offset and row width.
//   aug_letterbox_kernel<1>       the same on the [mh, mw] id mask with ITS OWN ratio and pads for an (s / r)^2 output (:725), fill 0, whole ids.
//                                 The reference computes them from the mask's size, not as the image's pads / r: mask and image can sit a fraction
//                                 of a cell apart (kept).
//   aug_letterbox_count_kernel, aug_letterbox_labels_kernel
//                                 every label of the source, in order (this branch has no thresholds); offsets = aug_count_scan_kernel over the
//                                 sources' label counts.  The reference carries cxcywh here (bbox_format = cxcywh, YoloDataset.cs:303): the
//                                 pixel xyxy table becomes cx = (x1 + x2) / 2, w = x2 - x1 (torchvision box_convert) -- a deviation of a few fp32
//                                 roundings -- then + (pad_l, pad_u, 0, 0) (:735-738; keypoints + (pad_l, pad_u), :741-744), NEITHER scaled by
//                                 ratio (kept: exact whenever ratio == 1), the flips, mul(1f / s) (Struct.cs:106-115).
//                                 QUIRK kept by default: FlipLR / FlipUD test bbox_format != xywh, true for cxcywh, and rewrite columns 0 AND 2
//                                 (1 AND 3) as s - value (:888-892, :943-947): a flipped box's width becomes s - w.  YS_AUG_FLIP_KEEP_SIZE leaves
//                                 columns 2 / 3 alone.  Keypoints: x <- s - x / y <- s - y, no left / right index swap (the reference has none).
struct AugLbGeom { int new_w, new_h, pad_l, pad_u; };

// LetterboxImage's geometry (:761-770) of an h x w plane on an out x out canvas, in the reference's fp32 arithmetic
__host__ __device__ inline AugLbGeom aug_letterbox_geom(int h, int w, int out) {
  const float ratio_w = (float)out / (float)w, ratio_h = (float)out / (float)h;
  const float ratio = ratio_w < ratio_h ? ratio_w : ratio_h;
  AugLbGeom g;
  g.new_w = (int)((float)w * ratio); g.new_h = (int)((float)h * ratio);
  g.new_w = g.new_w < 0 ? 0 : (g.new_w > out ? out : g.new_w);      // fp32 cannot leave [0, out] for sizes below 2^24; the clamp keeps the window inside
  g.new_h = g.new_h < 0 ? 0 : (g.new_h > out ? out : g.new_h);      // the output whatever the table holds
  g.pad_l = (out - g.new_w) / 2; g.pad_u = (out - g.new_h) / 2;
  return g;
}

// the source a LetterBox item names (src[0]; the other fields but the flips are ignored), or -1: outside the table, or a source without an image
__host__ __device__ inline int aug_letterbox_src(const ys_aug_item& it, const ys_aug_src* srcs, int n_src) {
  const int k = it.src[0];
  if (k < 0 || k >= n_src) return -1;
  const ys_aug_src& sr = srcs[k];
  return (sr.h < 1 || sr.w < 1 || sr.img_off < 0) ? -1 : k;
}

// one thread: 4 consecutive x of one output row, C planes -> C 16-byte stores (vec: s % 4 == 0, base 16-byte aligned), else scalar stores.
// C = 3: the image [B, 3, s, s]; C = 1: the id mask [B, s, s] with s = imgsz / mask_ratio.
template <int C>
__global__ void __launch_bounds__(AUG_T)
aug_letterbox_kernel(const unsigned char* __restrict__ arena, const ys_aug_src* __restrict__ srcs, int n_src, const ys_aug_item* __restrict__ items,
                     const ys_aug_jitter* __restrict__ jitter, int s, int vec, float* __restrict__ out) {
  const int qpr = (s + 3) >> 2;
  const unsigned i = blockIdx.x * AUG_T + threadIdx.x;
  if (i >= (unsigned)qpr * (unsigned)s) return;
  const int y = (int)(i / (unsigned)qpr), x0 = (int)(i - (unsigned)y * (unsigned)qpr) * 4;
  // wave-uniform: the item, its source and the window
  const ys_aug_item& it = items[blockIdx.z];
  // the image's jitter row (C == 3 only; NULL = none): an invalid row or one that asks for contrast refuses the image like a source outside the table
  const ys_aug_jitter* __restrict__ J = (C == 3 && jitter) ? jitter + blockIdx.z : nullptr;
  const int k = (J && aug_jitter_state(*J) != 1) ? -1 : aug_letterbox_src(it, srcs, n_src);
  int h = 0, w = 0;
  long long off = -1;
  if (k >= 0) {
    const ys_aug_src& sr = srcs[k];
    if (C == 3) { h = sr.h; w = sr.w; off = sr.img_off; }
    else if (sr.mask_off >= 0 && sr.mh >= 1 && sr.mw >= 1) { h = sr.mh; w = sr.mw; off = sr.mask_off; }
  }
  AugLbGeom g;
  g.new_w = g.new_h = g.pad_l = g.pad_u = 0;               // a refused item, a source without a mask: the window is empty, nothing is read
  // ratio == 1 (the loader has resized the long side to s): s / (float)s is exactly 1 and the other ratio is >= 1, so new = (h, w) -- no division, and
  // the nearest rule is the identity.  A wave-uniform branch.
  const bool ident = off >= 0 && ((w == s && h <= s) || (h == s && w <= s));
  if (ident) { g.new_w = w; g.new_h = h; g.pad_l = (s - w) / 2; g.pad_u = (s - h) / 2; }
  else if (off >= 0) g = aug_letterbox_geom(h, w, s);
  const bool flr = it.flip_lr != 0, fud = it.flip_ud != 0;
  const float q = 1 / 255.0f;                             // mul(1 / 255.0f), YoloDataset.cs:140: a multiply, bit-exact per byte; ids stay whole
  const float fill = C == 3 ? 114.0f : 0.0f;
  // the flips are folded into the output coordinate: out[y][x] = letterboxed[ly][lx]
  const int ry = (fud ? s - 1 - y : y) - g.pad_u;
  const bool row_in = (unsigned)ry < (unsigned)g.new_h;
  float v[C][4];
#pragma unroll
  for (int j = 0; j < 4; j++)
#pragma unroll
    for (int c = 0; c < C; c++) v[c][j] = fill;
  if (row_in) {
    // ATen's nearest rule, fp32: src = min(floor(dst * (float)in / out), in - 1)
    float sy = 1.0f, sx = 1.0f;
    if (!ident) { sy = (float)h / (float)g.new_h; sx = (float)w / (float)g.new_w; }
    int iy = (int)floorf((float)ry * sy);
    iy = iy < h - 1 ? iy : h - 1;
    const long long plane = (long long)h * w;
    const unsigned char* __restrict__ row = arena + off + (long long)iy * w;
    const int rx0 = (flr ? s - 1 - x0 : x0) - g.pad_l;     // source column of output x0; the quad's columns run down from it when flipped
    const int lo = flr ? rx0 - 3 : rx0;
    if (ident && x0 + 3 < s && lo >= 0 && lo + 3 < w) {
      // the whole quad lies in the window and its four source bytes are consecutive, at any alignment: the one or two ALIGNED words that hold them
      // (each holds at least one byte of the source, so neither can leave its page), shifted together
#pragma unroll
      for (int c = 0; c < C; c++) {
        const unsigned char* __restrict__ p = row + c * plane + lo;
        const unsigned sh = (unsigned)((unsigned long long)p & 3);
        const unsigned* __restrict__ wp = (const unsigned*)(p - sh);
        const unsigned w0 = wp[0], w1 = sh ? wp[1] : 0u;
        unsigned px = (unsigned)((((unsigned long long)w1 << 32) | w0) >> (8 * sh));
        if (flr) px = __builtin_bswap32(px);
        v[c][0] = (float)(px & 255u); v[c][1] = (float)((px >> 8) & 255u);
        v[c][2] = (float)((px >> 16) & 255u); v[c][3] = (float)(px >> 24);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int rx = flr ? rx0 - j : rx0 + j;
        if (x0 + j < s && (unsigned)rx < (unsigned)g.new_w) {
          int ix = (int)floorf((float)rx * sx);
          ix = ix < w - 1 ? ix : w - 1;
#pragma unroll
          for (int c = 0; c < C; c++) v[c][j] = (float)row[c * plane + ix];
        }
      }
    }
  }
  if constexpr (C == 3) {                                  // the bytes (the 114 of the padding included) through the row's ops, then mul(1 / 255.0f)
    if (J && k >= 0) {
      AugPx p0 = {v[0][0], v[1][0], v[2][0]}, p1 = {v[0][1], v[1][1], v[2][1]}, p2 = {v[0][2], v[1][2], v[2][2]}, p3 = {v[0][3], v[1][3], v[2][3]};
      aug_jitter_quad(J, 0.0f, false, p0, p1, p2, p3);
      v[0][0] = p0.c0; v[1][0] = p0.c1; v[2][0] = p0.c2; v[0][1] = p1.c0; v[1][1] = p1.c1; v[2][1] = p1.c2;
      v[0][2] = p2.c0; v[1][2] = p2.c1; v[2][2] = p2.c2; v[0][3] = p3.c0; v[1][3] = p3.c1; v[2][3] = p3.c2;
    }
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
      for (int c = 0; c < C; c++) v[c][j] *= q;
  }
  const long long oplane = (long long)s * s;
  float* dst = out + (long long)blockIdx.z * C * oplane + (long long)y * s + x0;
  if (vec) {
#pragma unroll
    for (int c = 0; c < C; c++) ys_st16(dst + c * oplane, make_uint4(ys_f2u(v[c][0]), ys_f2u(v[c][1]), ys_f2u(v[c][2]), ys_f2u(v[c][3])));
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (x0 + j < s)
#pragma unroll
        for (int c = 0; c < C; c++) dst[c * oplane + j] = v[c][j];
  }
}

// counts[b] = the label count of image b's source (0 for a refused item)
__global__ void __launch_bounds__(AUG_T)
aug_letterbox_count_kernel(const ys_aug_src* __restrict__ srcs, int n_src, const int* __restrict__ lab_off, const ys_aug_item* __restrict__ items, int B,
                           int* __restrict__ counts) {
  const int b = blockIdx.x * AUG_T + threadIdx.x;
  if (b >= B) return;
  const int k = aug_letterbox_src(items[b], srcs, n_src);
  const int n = k >= 0 ? lab_off[k + 1] - lab_off[k] : 0;
  counts[b] = n > 0 ? n : 0;
}

// one workgroup per image: rows [offs[b], offs[b + 1]) = the source's labels in order; the tail [total, capacity) = (batch_idx -1, zeros);
// *o_count = total (a total above capacity is reported as it is; rows past capacity are not written).
// OBB: kpts holds the corners [n][4][2], o_box has 5 columns, o_kpt is NULL: corners + (pad_l, pad_u), not scaled by ratio like the boxes (:746-749),
// nothing clipped (a corner may lie outside [0, s]), the flips (:825-828), aug_label_obb's rectangle and division.
template <bool OBB>
__global__ void __launch_bounds__(AUG_T)
aug_letterbox_labels_kernel(const ys_aug_src* __restrict__ srcs, int n_src, const int* __restrict__ lab_off, const float* __restrict__ cls,
                            const float* __restrict__ boxes, const float* __restrict__ kpts, int K, const ys_aug_item* __restrict__ items, int B, int s,
                            int flags, int capacity, const int* __restrict__ offs, float* __restrict__ o_bidx, float* __restrict__ o_cls,
                            float* __restrict__ o_box, float* __restrict__ o_kpt, int* __restrict__ o_count) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const ys_aug_item& it = items[b];
  const int base = offs[b], n = offs[b + 1] - base, total = offs[B];
  const int k = aug_letterbox_src(it, srcs, n_src);
  if (k >= 0 && n > 0) {
    const AugLbGeom g = aug_letterbox_geom(srcs[k].h, srcs[k].w, s);
    const int first = lab_off[k];
    const float S = (float)s, inv = 1.0f / S, pl = (float)g.pad_l, pu = (float)g.pad_u;
    const bool flr = it.flip_lr != 0, fud = it.flip_ud != 0, keep_size = (flags & YS_AUG_FLIP_KEEP_SIZE) != 0;
    for (int j = tid; j < n; j += AUG_T) {
      const long long rowi = (long long)base + j;
      if (rowi >= capacity) break;
      const int l = first + j;
      if constexpr (OBB) {
        float r5[5];
        aug_label_obb(kpts + 8 * (long long)l, pl, pu, false, nullptr, s, 0, flr, fud, r5);
        o_bidx[rowi] = (float)b; o_cls[rowi] = cls[l];
#pragma unroll
        for (int p = 0; p < 5; p++) o_box[5 * rowi + p] = r5[p];
        continue;
      }
      const float x1 = boxes[4 * l], y1 = boxes[4 * l + 1], x2 = boxes[4 * l + 2], y2 = boxes[4 * l + 3];
      float cx = (x1 + x2) / 2.0f + pl, cy = (y1 + y2) / 2.0f + pu, bw = x2 - x1, bh = y2 - y1;
      if (flr) { cx = S - cx; if (!keep_size) bw = S - bw; }
      if (fud) { cy = S - cy; if (!keep_size) bh = S - bh; }
      o_bidx[rowi] = (float)b; o_cls[rowi] = cls[l];
      o_box[4 * rowi] = cx * inv; o_box[4 * rowi + 1] = cy * inv; o_box[4 * rowi + 2] = bw * inv; o_box[4 * rowi + 3] = bh * inv;
      if (o_kpt) {
        const float* __restrict__ kin = kpts + (long long)l * K * 3;
        float* __restrict__ kout = o_kpt + rowi * K * 3;
        for (int p = 0; p < K; p++) {
          float px = kin[3 * p] + pl, py = kin[3 * p + 1] + pu;
          if (flr) px = S - px;
          if (fud) py = S - py;
          kout[3 * p] = px * inv; kout[3 * p + 1] = py * inv; kout[3 * p + 2] = kin[3 * p + 2];
        }
      }
    }
  }
  if (b == 0 && tid == 0) *o_count = total;
  for (long long rowi = (long long)total + (long long)b * AUG_T + tid; rowi < capacity; rowi += (long long)B * AUG_T) {
    o_bidx[rowi] = -1.0f; o_cls[rowi] = 0.0f;
    if constexpr (OBB) {
#pragma unroll
      for (int p = 0; p < 5; p++) o_box[5 * rowi + p] = 0.f;
      continue;
    }
    o_box[4 * rowi] = 0.f; o_box[4 * rowi + 1] = 0.f; o_box[4 * rowi + 2] = 0.f; o_box[4 * rowi + 3] = 0.f;
    if (o_kpt) for (int p = 0; p < K * 3; p++) o_kpt[rowi * K * 3 + p] = 0.f;
  }
}

// ---------------------------------------------------------------------------------------------------------------- ColorJitter on its own
// ys_color_jitter: all four ops on uint8 planes [B, 3, n] (n = h * w; the ops are per pixel, so a thread takes four consecutive pixels of the
// flattened plane).  vec: n % 4 == 0 and aligned bases -> one word per plane in, one word (uint8) or 16 bytes (fp32) per plane out.
__device__ __forceinline__ void aug_cj_load(const unsigned char* __restrict__ src, long long n, long long i4, int vec, AugPx& p0, AugPx& p1, AugPx& p2,
                                            AugPx& p3) {
  float v[3][4];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const unsigned char* __restrict__ p = src + c * n + i4;
    if (vec) {
      const unsigned px = *(const unsigned*)p;
      v[c][0] = (float)(px & 255u); v[c][1] = (float)((px >> 8) & 255u); v[c][2] = (float)((px >> 16) & 255u); v[c][3] = (float)(px >> 24);
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++) v[c][j] = i4 + j < n ? (float)p[j] : 0.0f;
    }
  }
  p0.c0 = v[0][0]; p0.c1 = v[1][0]; p0.c2 = v[2][0]; p1.c0 = v[0][1]; p1.c1 = v[1][1]; p1.c2 = v[2][1];
  p2.c0 = v[0][2]; p2.c1 = v[1][2]; p2.c2 = v[2][2]; p3.c0 = v[0][3]; p3.c1 = v[1][3]; p3.c2 = v[2][3];
}

// contrast, launch 1 of 2: sums[b] += the gray bytes of image b in its state in front of the contrast op (the ops ahead of it are replayed).
// Integer atomics: any order gives the same sum.  Images whose row does not run contrast leave at once.
__global__ void __launch_bounds__(AUG_T)
aug_cj_gray_sum_kernel(const unsigned char* __restrict__ src, const ys_aug_jitter* __restrict__ jitter, long long n, int vec,
                       unsigned long long* __restrict__ sums) {
  __shared__ unsigned s_red[AUG_T];
  const ys_aug_jitter* __restrict__ J = jitter + blockIdx.z;
  if (aug_jitter_state(*J) != 2) return;                   // wave-uniform, block-uniform
  const long long i4 = ((long long)blockIdx.x * AUG_T + threadIdx.x) * 4;
  unsigned sum = 0;
  if (i4 < n) {
    AugPx p0, p1, p2, p3;
    aug_cj_load(src + (long long)blockIdx.z * 3 * n, n, i4, vec, p0, p1, p2, p3);
    aug_jitter_quad(J, 0.0f, true, p0, p1, p2, p3);
    sum = (unsigned)aug_jit_gray(p0);
    if (i4 + 1 < n) sum += (unsigned)aug_jit_gray(p1);
    if (i4 + 2 < n) sum += (unsigned)aug_jit_gray(p2);
    if (i4 + 3 < n) sum += (unsigned)aug_jit_gray(p3);
  }
  s_red[threadIdx.x] = sum;
  __syncthreads();
  for (int d = AUG_T / 2; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d) s_red[threadIdx.x] += s_red[threadIdx.x + d];
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicAdd(&sums[blockIdx.z], (unsigned long long)s_red[0]);
}

// launch 2 of 2 (the only one for rows without contrast): every op in the row's order; mean = (float)sum / (float)n -- for n <= 65536 the sum is an
// exact fp32 integer and this is torch.mean's value; above that torch's own fp32 summation order decides its last bit (the one deviation).
// An invalid row gives the all-114 image, like a refused item of the fused entries.
__global__ void __launch_bounds__(AUG_T)
aug_cj_apply_kernel(const unsigned char* __restrict__ src, const ys_aug_jitter* __restrict__ jitter, long long n, int vec,
                    const unsigned long long* __restrict__ sums, void* __restrict__ dst, int dst_is_float) {
  const long long i4 = ((long long)blockIdx.x * AUG_T + threadIdx.x) * 4;
  if (i4 >= n) return;
  const ys_aug_jitter* __restrict__ J = jitter + blockIdx.z;
  const int state = aug_jitter_state(*J);                  // wave-uniform
  AugPx p0, p1, p2, p3;
  if (state == 0) {
    p0.c0 = p0.c1 = p0.c2 = 114.0f; p1 = p0; p2 = p0; p3 = p0;
  } else {
    aug_cj_load(src + (long long)blockIdx.z * 3 * n, n, i4, vec, p0, p1, p2, p3);
    const float mean = state == 2 ? (float)sums[blockIdx.z] / (float)n : 0.0f;
    aug_jitter_quad(J, mean, false, p0, p1, p2, p3);
  }
  const float v[3][4] = {{p0.c0, p1.c0, p2.c0, p3.c0}, {p0.c1, p1.c1, p2.c1, p3.c1}, {p0.c2, p1.c2, p2.c2, p3.c2}};
  const long long base = (long long)blockIdx.z * 3 * n + i4;
  if (dst_is_float) {
    const float q = 1 / 255.0f;
    float* __restrict__ o = (float*)dst + base;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      if (vec) ys_st16(o + c * n, make_uint4(ys_f2u(v[c][0] * q), ys_f2u(v[c][1] * q), ys_f2u(v[c][2] * q), ys_f2u(v[c][3] * q)));
      else
#pragma unroll
        for (int j = 0; j < 4; j++) if (i4 + j < n) o[c * n + j] = v[c][j] * q;
    }
  } else {
    unsigned char* __restrict__ o = (unsigned char*)dst + base;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      if (vec) *(unsigned*)(o + c * n) = (unsigned)v[c][0] | ((unsigned)v[c][1] << 8) | ((unsigned)v[c][2] << 16) | ((unsigned)v[c][3] << 24);
      else
#pragma unroll
        for (int j = 0; j < 4; j++) if (i4 + j < n) o[c * n + j] = (unsigned char)v[c][j];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- launchers
size_t ys_aug_ws_bytes(int B) { return (size_t)B * sizeof(AugParams) + ((size_t)2 * B + 1) * sizeof(int) + 64; }   // params | counts [B] | offsets [B + 1]

int ys_aug_item_ok_host(const ys_aug_item* it, const ys_aug_src* srcs, int n_src, int s, int perspective) {
  return aug_item_ok(*it, srcs, n_src, s, perspective);
}

int ys_aug_mosaic_launch(hipStream_t st, const unsigned char* arena, const ys_aug_src* srcs, int n_src, const ys_aug_item* items, int B, int s,
                         int r, int perspective, const ys_aug_jitter* jitter, void* ws, float* images, float* masks) {
  AugParams* params = (AugParams*)ws;
  YS_LAUNCH(aug_prep_kernel, ys_cdiv(B, 64), 64, st, srcs, n_src, items, B, s, r, perspective, params);
  const long quads = (long)((s + 3) / 4) * s;
  YS_LAUNCH(aug_mosaic_warp_kernel, dim3(ys_cdiv(quads, AUG_T), 1, B), AUG_T, st, arena, (const AugParams*)params, jitter, s, perspective,
            (s % 4 == 0 && ((size_t)images & 15) == 0) ? 1 : 0, images);
  if (masks) {
    const long n = (long)(s / r) * (s / r);
    YS_LAUNCH(aug_mask_warp_kernel, dim3(ys_cdiv(n, AUG_T), 1, B), AUG_T, st, arena, (const AugParams*)params, s, r, perspective, masks);
  }
  return YS_OK;
}

int ys_aug_labels_launch(hipStream_t st, const ys_aug_src* srcs, int n_src, const int* lab_off, const float* cls, const float* boxes,
                         const float* kpts, int K, const ys_aug_item* items, int B, int s, int perspective, int flags, int capacity, void* ws,
                         float* o_bidx, float* o_cls, float* o_box, float* o_kpt, int* o_count, int obb) {
  int* counts = (int*)((char*)ws + (size_t)B * sizeof(AugParams));
  for (int pass = 0; pass < 2; pass++) {
    if (pass == 1) YS_LAUNCH(aug_count_scan_kernel, 1, AUG_T, st, (const int*)counts, B, counts + B);
    if (obb) YS_LAUNCH((aug_labels_kernel<true>), B, AUG_T, st, srcs, n_src, lab_off, cls, boxes, kpts, 0, items, B, s, perspective, flags, capacity, pass, counts,
                       o_bidx, o_cls, o_box, (float*)nullptr, o_count);
    else YS_LAUNCH((aug_labels_kernel<false>), B, AUG_T, st, srcs, n_src, lab_off, cls, boxes, kpts, K, items, B, s, perspective, flags, capacity, pass, counts,
                   o_bidx, o_cls, o_box, o_kpt, o_count);
  }
  return YS_OK;
}

int ys_xyxyxyxy2xywhr_launch(hipStream_t st, const float* corners, int n, float* out) {
  YS_LAUNCH(aug_xyxyxyxy2xywhr_kernel, ys_cdiv(n, AUG_T), AUG_T, st, corners, n, out);
  return YS_OK;
}

int ys_aug_letterbox_src_host(const ys_aug_item* it, const ys_aug_src* srcs, int n_src) { return aug_letterbox_src(*it, srcs, n_src); }

int ys_aug_letterbox_launch(hipStream_t st, const unsigned char* arena, const ys_aug_src* srcs, int n_src, const ys_aug_item* items, int B, int s,
                            int r, const ys_aug_jitter* jitter, float* images, float* masks) {
  const long quads = (long)((s + 3) / 4) * s;
  YS_LAUNCH((aug_letterbox_kernel<3>), dim3(ys_cdiv(quads, AUG_T), 1, B), AUG_T, st, arena, srcs, n_src, items, jitter, s,
            (s % 4 == 0 && ((size_t)images & 15) == 0) ? 1 : 0, images);
  if (masks) {
    const int ms = s / r;
    const long mquads = (long)((ms + 3) / 4) * ms;
    YS_LAUNCH((aug_letterbox_kernel<1>), dim3(ys_cdiv(mquads, AUG_T), 1, B), AUG_T, st, arena, srcs, n_src, items, (const ys_aug_jitter*)nullptr, ms,
              (ms % 4 == 0 && ((size_t)masks & 15) == 0) ? 1 : 0, masks);
  }
  return YS_OK;
}

int ys_aug_letterbox_labels_launch(hipStream_t st, const ys_aug_src* srcs, int n_src, const int* lab_off, const float* cls, const float* boxes,
                                   const float* kpts, int K, const ys_aug_item* items, int B, int s, int flags, int capacity, void* ws, float* o_bidx,
                                   float* o_cls, float* o_box, float* o_kpt, int* o_count, int obb) {
  int* counts = (int*)((char*)ws + (size_t)B * sizeof(AugParams));            // the workspace layout of ys_aug_ws_bytes: counts [B] | offsets [B + 1]
  YS_LAUNCH(aug_letterbox_count_kernel, ys_cdiv(B, AUG_T), AUG_T, st, srcs, n_src, lab_off, items, B, counts);
  YS_LAUNCH(aug_count_scan_kernel, 1, AUG_T, st, (const int*)counts, B, counts + B);
  if (obb) YS_LAUNCH((aug_letterbox_labels_kernel<true>), B, AUG_T, st, srcs, n_src, lab_off, cls, boxes, kpts, 0, items, B, s, flags, capacity,
                     (const int*)(counts + B), o_bidx, o_cls, o_box, (float*)nullptr, o_count);
  else YS_LAUNCH((aug_letterbox_labels_kernel<false>), B, AUG_T, st, srcs, n_src, lab_off, cls, boxes, kpts, K, items, B, s, flags, capacity,
                 (const int*)(counts + B), o_bidx, o_cls, o_box, o_kpt, o_count);
  return YS_OK;
}

int ys_aug_jitter_state_host(const ys_aug_jitter* row) { return aug_jitter_state(*row); }

// sums: B zeroed 64-bit counters (read and written only where a row runs contrast); with_contrast = 0 skips the reduction (the caller knows the rows)
int ys_color_jitter_launch(hipStream_t st, const unsigned char* src, const ys_aug_jitter* jitter, int B, long long n, int with_contrast, void* sums,
                           void* dst, int dst_is_float) {
  const int vec = (n % 4 == 0 && ((size_t)src & 3) == 0 && ((size_t)dst & (dst_is_float ? 15 : 3)) == 0) ? 1 : 0;
  const dim3 grid(ys_cdiv((n + 3) / 4, AUG_T), 1, B);
  if (with_contrast) YS_LAUNCH(aug_cj_gray_sum_kernel, grid, AUG_T, st, src, jitter, n, vec, (unsigned long long*)sums);
  YS_LAUNCH(aug_cj_apply_kernel, grid, AUG_T, st, src, jitter, n, vec, (const unsigned long long*)sums, dst, dst_is_float);
  return YS_OK;
}
