// elementwise.hip -- HBM-bound NHWC kernels around the convolutions (gfx950).
//   input pack / unpack, LetterBox resize                           (Detector.cs:33-41, Data/Augment.cs:698-857)
//   MaxPool2d(5,1,2) chain of SPPF                                   (Modules/Block.cs:236-285)
//   Upsample(x2, nearest) + Concat as channel-slice writes           (Models/Yolo.cs:70-75, Convs.cs:435-448)
//   Detect._inference decode                                         (Modules/Head.cs:204-223, Block.cs:40-45)
//   AdamW step                                                       (YoloBaseTaskModel.cs:144-153, Amp.cs:355-372)
// (The BatchNorm + SiLU training passes are batchnorm.hip.)
// All tensors are [rows][ldc] views with a channel offset; one thread moves 16 bytes (8 bf16 / 4 f32).
#include "ys_internal.h"
#include "ys_kernels.h"
#include <cstdlib>

#define EW_THREADS 256

// ------------------------------------------------------------------ input pack / unpack
// one thread per pixel: C planar reads (coalesced across threads), one packed row of cpad channels written with 16-byte stores
template <class T, class SRC>
__global__ void __launch_bounds__(EW_THREADS)
pack_input_kernel(const SRC* __restrict__ x, int B, int C, int h, int w, int H, int W, int cpad, float div, float padv,
                  T* __restrict__ y) {
  constexpr int EPL = Elem<T>::EPL;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long HW = (long)H * W;
  if (i >= (long)B * HW) return;
  long b; int py, px;
  if ((long)B * HW < (1L << 31)) {                        // 32-bit index arithmetic (two 64-bit divisions are ~160 VALU instructions)
    const unsigned iu = (unsigned)i, hw = (unsigned)HW, bu = iu / hw, pu = iu - bu * hw;
    b = bu; py = (int)(pu / (unsigned)W); px = (int)(pu - (unsigned)py * (unsigned)W);
  } else {
    b = i / HW; const long p = i - b * HW;
    py = (int)(p / W); px = (int)(p - (long)py * W);
  }
  const bool in = py < h && px < w;                       // bottom / right padding (Detector.cs:33-41)
  const bool unit = div == 1.0f;                          // fp32 images in [0,1]: no division at all
  for (int c0 = 0; c0 < cpad; c0 += EPL) {
    float f[EPL];
#pragma unroll
    for (int e = 0; e < EPL; e++) {
      const int c = c0 + e;
      float v = 0.f;
      if (c < C) {
        v = padv;
        if (in) { const float r = (float)x[((b * C + c) * h + py) * (long)w + px]; v = unit ? r : r / div; }
      }
      f[e] = v;
    }
    ys_st16(y + i * cpad + c0, ys_pack<T>(f));
  }
}
// fp32 image planes, C <= EPL (one 16-byte vector per pixel), W % 4 == 0: four consecutive pixels per thread -- 16-byte plane loads,
// 64 contiguous bytes written
template <class T>
__global__ void __launch_bounds__(EW_THREADS)
pack_input4_kernel(const float* __restrict__ x, long npix4, int C, long HW, T* __restrict__ y) {
  constexpr int EPL = Elem<T>::EPL;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;       // group of 4 pixels
  if (i >= npix4) return;
  const long pix = i * 4;
  const long b = pix / HW, p = pix - b * HW;
  float4 pl[EPL];
#pragma unroll
  for (int c = 0; c < EPL; c++) pl[c] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int c = 0; c < EPL; c++)
    if (c < C) pl[c] = *(const float4*)(x + (b * C + c) * HW + p);
#pragma unroll
  for (int k = 0; k < 4; k++) {
    float f[EPL];
#pragma unroll
    for (int c = 0; c < EPL; c++) f[c] = k == 0 ? pl[c].x : k == 1 ? pl[c].y : k == 2 ? pl[c].z : pl[c].w;
    ys_st16(y + (pix + k) * EPL, ys_pack<T>(f));
  }
}

int ys_pack_input_launch(hipStream_t st, int dtype, const float* x, int B, int C, int H, int W, int cpad, void* y) {
  const long n = (long)B * H * W;
  const int epl = dtype == YS_BF16 ? 8 : 4;
  if (cpad == epl && C <= epl && C <= 4 && W % 4 == 0 && ((size_t)x & 15) == 0) {   // the model's image input
    const long n4 = n / 4;
    if (dtype == YS_BF16) YS_LAUNCH((pack_input4_kernel<bf16_t>), ys_cdiv(n4, EW_THREADS), EW_THREADS, st, x, n4, C, (long)H * W, (bf16_t*)y);
    else YS_LAUNCH((pack_input4_kernel<float>), ys_cdiv(n4, EW_THREADS), EW_THREADS, st, x, n4, C, (long)H * W, (float*)y);
    return YS_OK;
  }
  if (dtype == YS_BF16) YS_LAUNCH((pack_input_kernel<bf16_t, float>), ys_cdiv(n, EW_THREADS), EW_THREADS, st, x, B, C, H, W, H, W, cpad, 1.0f, 0.0f, (bf16_t*)y);
  else YS_LAUNCH((pack_input_kernel<float, float>), ys_cdiv(n, EW_THREADS), EW_THREADS, st, x, B, C, H, W, H, W, cpad, 1.0f, 0.0f, (float*)y);
  return YS_OK;
}
// uint8 [B,C,h,w] (0..255) -> NHWC T [B,H,W,cpad]: value / 255, bottom / right padding with 114 / 255 (Detector.cs:33-41)
int ys_pack_input_u8_launch(hipStream_t st, int dtype, const unsigned char* x, int B, int C, int h, int w, int H, int W, int cpad, void* y) {
  const long n = (long)B * H * W;
  const float s = 255.0f, pv = 114.0f / 255.0f;        // true division like the reference's `/ 255.0f`
  if (dtype == YS_BF16) YS_LAUNCH((pack_input_kernel<bf16_t, unsigned char>), ys_cdiv(n, EW_THREADS), EW_THREADS, st, x, B, C, h, w, H, W, cpad, s, pv, (bf16_t*)y);
  else YS_LAUNCH((pack_input_kernel<float, unsigned char>), ys_cdiv(n, EW_THREADS), EW_THREADS, st, x, B, C, h, w, H, W, cpad, s, pv, (float*)y);
  return YS_OK;
}

// LetterBox / Rectangle (Data/Augment.cs:698-857): out[c, y, x] = in[c, src_y(y - pad_u), src_x(x - pad_l)] inside the resized
// window [pad_u, pad_u + new_h) x [pad_l, pad_l + new_w), `color` elsewhere.  The resize is
// torchvision.transforms.functional.resize(img, new_h, new_w) of TorchVision(.NET), whose default interpolation is NEAREST
// (third-party, not vendored): ATen's legacy nearest rule  src = min(floor(dst * (float)in / out), in - 1),
// evaluated here in the same fp32 arithmetic.  One thread per output pixel and plane; ET = unsigned char (images) or float (masks).
template <class ET>
__global__ void __launch_bounds__(EW_THREADS)
letterbox_kernel(const ET* __restrict__ x, int C, int h, int w, ET* __restrict__ y, int H, int W, int new_h, int new_w,
                 int pad_u, int pad_l, float color) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long n = (long)C * H * W;
  if (i >= n) return;
  const int ox = (int)(i % W);
  const int oy = (int)((i / W) % H);
  const int c = (int)(i / ((long)W * H));
  const int ry = oy - pad_u, rx = ox - pad_l;
  ET v = (ET)color;
  if (ry >= 0 && ry < new_h && rx >= 0 && rx < new_w) {
    const float sy = (float)h / (float)new_h, sx = (float)w / (float)new_w;
    int iy = (int)floorf((float)ry * sy), ix = (int)floorf((float)rx * sx);
    iy = iy < h - 1 ? iy : h - 1; ix = ix < w - 1 ? ix : w - 1;
    v = x[((long)c * h + iy) * w + ix];
  }
  y[i] = v;
}
int ys_letterbox_launch(hipStream_t st, int is_float, const void* x, int C, int h, int w, void* y, int H, int W, int new_h, int new_w,
                        int pad_u, int pad_l, float color) {
  const long n = (long)C * H * W;
  if (n <= 0) return YS_OK;
  if (is_float) YS_LAUNCH((letterbox_kernel<float>), ys_cdiv(n, EW_THREADS), EW_THREADS, st, (const float*)x, C, h, w, (float*)y, H, W, new_h, new_w, pad_u, pad_l, color);
  else YS_LAUNCH((letterbox_kernel<unsigned char>), ys_cdiv(n, EW_THREADS), EW_THREADS, st, (const unsigned char*)x, C, h, w, (unsigned char*)y, H, W, new_h, new_w, pad_u, pad_l, color);
  return YS_OK;
}

template <class T>
__global__ void __launch_bounds__(EW_THREADS)
unpack_nchw_kernel(const T* __restrict__ x, int ldc, int coff, int B, int C, long rpb, float* __restrict__ y) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long n = (long)B * C * rpb;
  if (i >= n) return;
  const long p = i % rpb;
  const long bc = i / rpb;
  const int c = (int)(bc % C);
  const long b = bc / C;
  y[i] = Elem<T>::to_f(x[(b * rpb + p) * ldc + coff + c]);
}
int ys_unpack_nchw_launch(hipStream_t st, int dtype, const void* x, int ldc, int coff, int B, int C, long rpb, float* y) {
  const long n = (long)B * C * rpb;
  if (dtype == YS_BF16) YS_LAUNCH((unpack_nchw_kernel<bf16_t>), ys_cdiv(n, EW_THREADS), EW_THREADS, st, (const bf16_t*)x, ldc, coff, B, C, rpb, y);
  else YS_LAUNCH((unpack_nchw_kernel<float>), ys_cdiv(n, EW_THREADS), EW_THREADS, st, (const float*)x, ldc, coff, B, C, rpb, y);
  return YS_OK;
}

// [B][rpb][ldc] view -> channel block of a wider NCHW tensor: y[b*y_bstride + y_off + c*rpb + p]
template <class T>
__global__ void __launch_bounds__(EW_THREADS)
unpack_nchw_strided_kernel(const T* __restrict__ x, int ldc, int coff, int B, int C, long rpb, float* __restrict__ y, long y_bstride, long y_off) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * C * rpb) return;
  const long p = i % rpb;
  const long bc = i / rpb;
  const int c = (int)(bc % C);
  const long b = bc / C;
  y[b * y_bstride + y_off + (long)c * rpb + p] = Elem<T>::to_f(x[(b * rpb + p) * ldc + coff + c]);
}
int ys_unpack_nchw_strided_launch(hipStream_t st, int dtype, const void* x, int ldc, int coff, int B, int C, long rpb, float* y,
                                  long y_bstride, long y_off) {
  const long n = (long)B * C * rpb;
  if (dtype == YS_BF16) YS_LAUNCH((unpack_nchw_strided_kernel<bf16_t>), ys_cdiv(n, EW_THREADS), EW_THREADS, st, (const bf16_t*)x, ldc, coff, B, C, rpb, y, y_bstride, y_off);
  else YS_LAUNCH((unpack_nchw_strided_kernel<float>), ys_cdiv(n, EW_THREADS), EW_THREADS, st, (const float*)x, ldc, coff, B, C, rpb, y, y_bstride, y_off);
  return YS_OK;
}

// ------------------------------------------------------------------ max-pool 5x5 s1 p2
// argmax = first maximum in (kh,kw) scan order with strict '>' (ATen max_pool2d CPU semantics)
template <class T>
__global__ void __launch_bounds__(EW_THREADS)
maxpool5_fwd_kernel(const T* __restrict__ x, int x_ldc, int x_coff, int B, int H, int W, int C, T* __restrict__ y,
                    int y_ldc, int y_coff, unsigned char* __restrict__ amax) {
  constexpr int EPL = Elem<T>::EPL;
  const int CG = C / EPL;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long n = (long)B * H * W * CG;
  if (i >= n) return;
  const int c = (int)(i % CG) * EPL;
  const long pix = i / CG;
  const int w = (int)(pix % W);
  const int h = (int)((pix / W) % H);
  const long b = pix / ((long)W * H);
  float best[EPL];
  int bi[EPL];
#pragma unroll
  for (int e = 0; e < EPL; e++) { best[e] = -INFINITY; bi[e] = 0; }
  bool first = true;
  for (int kh = 0; kh < 5; kh++) {
    const int ih = h + kh - 2;
    if (ih < 0 || ih >= H) continue;
    for (int kw = 0; kw < 5; kw++) {
      const int iw = w + kw - 2;
      if (iw < 0 || iw >= W) continue;
      float f[EPL];
      ys_unpack<T>(ys_ld16(x + ((b * H + ih) * W + iw) * x_ldc + x_coff + c), f);
#pragma unroll
      for (int e = 0; e < EPL; e++)
        if (first || f[e] > best[e]) { best[e] = f[e]; bi[e] = kh * 5 + kw; }
      first = false;
    }
  }
  ys_st16(y + pix * y_ldc + y_coff + c, ys_pack<T>(best));
  if (amax) {
#pragma unroll
    for (int e = 0; e < EPL; e++) amax[pix * C + c + e] = (unsigned char)bi[e];
  }
}
int ys_maxpool5_fwd_launch(hipStream_t st, int dtype, const void* x, int x_ldc, int x_coff, int B, int H, int W, int C,
                           void* y, int y_ldc, int y_coff, unsigned char* argmax) {
  const int epl = dtype == YS_BF16 ? 8 : 4;
  const long n = (long)B * H * W * (C / epl);
  if (dtype == YS_BF16)
    YS_LAUNCH((maxpool5_fwd_kernel<bf16_t>), ys_cdiv(n, EW_THREADS), EW_THREADS, st, (const bf16_t*)x, x_ldc, x_coff, B, H, W, C, (bf16_t*)y, y_ldc, y_coff, argmax);
  else
    YS_LAUNCH((maxpool5_fwd_kernel<float>), ys_cdiv(n, EW_THREADS), EW_THREADS, st, (const float*)x, x_ldc, x_coff, B, H, W, C, (float*)y, y_ldc, y_coff, argmax);
  return YS_OK;
}

template <class T>
__global__ void __launch_bounds__(EW_THREADS)
maxpool5_bwd_kernel(const T* __restrict__ dy, int dy_ldc, int dy_coff, int B, int H, int W, int C,
                    const unsigned char* __restrict__ amax, T* __restrict__ dx, int dx_ldc, int dx_coff, int accumulate) {
  constexpr int EPL = Elem<T>::EPL;
  const int CG = C / EPL;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long n = (long)B * H * W * CG;
  if (i >= n) return;
  const int c = (int)(i % CG) * EPL;
  const long pix = i / CG;
  const int w = (int)(pix % W);
  const int h = (int)((pix / W) % H);
  const long b = pix / ((long)W * H);
  float acc[EPL];
#pragma unroll
  for (int e = 0; e < EPL; e++) acc[e] = 0.f;
  for (int kh = 0; kh < 5; kh++) {
    const int oh = h - kh + 2;  // output whose window holds (h,w) at offset (kh,kw)
    if (oh < 0 || oh >= H) continue;
    for (int kw = 0; kw < 5; kw++) {
      const int ow = w - kw + 2;
      if (ow < 0 || ow >= W) continue;
      const long op = (b * H + oh) * W + ow;
      float g[EPL];
      ys_unpack<T>(ys_ld16(dy + op * dy_ldc + dy_coff + c), g);
      const int code = kh * 5 + kw;
#pragma unroll
      for (int e = 0; e < EPL; e++)
        if (amax[op * C + c + e] == code) acc[e] += g[e];
    }
  }
  T* dp = dx + pix * dx_ldc + dx_coff + c;
  if (accumulate) {
    float o[EPL];
    ys_unpack<T>(ys_ld16(dp), o);
#pragma unroll
    for (int e = 0; e < EPL; e++) acc[e] += o[e];
  }
  ys_st16(dp, ys_pack<T>(acc));
}
int ys_maxpool5_bwd_launch(hipStream_t st, int dtype, const void* dy, int dy_ldc, int dy_coff, int B, int H, int W,
                           int C, const unsigned char* argmax, void* dx, int dx_ldc, int dx_coff, int accumulate) {
  const int epl = dtype == YS_BF16 ? 8 : 4;
  const long n = (long)B * H * W * (C / epl);
  if (dtype == YS_BF16)
    YS_LAUNCH((maxpool5_bwd_kernel<bf16_t>), ys_cdiv(n, EW_THREADS), EW_THREADS, st, (const bf16_t*)dy, dy_ldc, dy_coff, B, H, W, C, argmax, (bf16_t*)dx, dx_ldc, dx_coff, accumulate);
  else
    YS_LAUNCH((maxpool5_bwd_kernel<float>), ys_cdiv(n, EW_THREADS), EW_THREADS, st, (const float*)dy, dy_ldc, dy_coff, B, H, W, C, argmax, (float*)dx, dx_ldc, dx_coff, accumulate);
  return YS_OK;
}

// ------------------------------------------------------------------ SPPF: the three chained 5x5 pools of one concat buffer in one launch
// A workgroup owns (image, four 16-byte units of channels: 32 bf16 or 16 f32, 64 contiguous bytes per pixel in memory): the map sits in LDS, the three pools run
// from LDS and every stage writes its concat slice (+ its argmax plane in training).  Results are those of three maxpool5_fwd_kernel launches bit for bit:
//  * the pool is separable -- a row pass keeps, per row of the window, the FIRST kw of the row maximum (strict '>'), the column pass the FIRST kh whose row maximum
//    is strictly greater: together the first maximum in (kh, kw) scan order.  Both start from -inf with the code of the first tap of the clipped window, which is
//    what "the first visited tap is always taken" gives for every non-NaN map; a NaN in the first tap is taken afterwards, as the scan does.
//  * taps outside the map are clamped to the edge instead of skipped: on the low side the clamped taps read the first in-window element early and carry its real
//    code (max(k, k0)); on the high side they repeat an element already seen, which strict '>' never takes.
// Every loop runs SPPF_NIT rounds for every thread and the barriers sit between the loops: nothing here depends on the pixel or the channel.
#define SPPF_THREADS 512
#define SPPF_MAXHW 400                  // 20 x 20: LDS 25.6 KB map + 25.6 KB row maxima + 6.4 KB row codes (backward: 25.6 KB gradient + 12.8 KB codes)
#define SPPF_CU 4                       // 16-byte units per pixel and workgroup
#define SPPF_NIT ((SPPF_MAXHW * SPPF_CU + SPPF_THREADS - 1) / SPPF_THREADS)
__device__ inline int sppf_min(int x, int y) { return x < y ? x : y; }
__device__ inline int sppf_max(int x, int y) { return x > y ? x : y; }
struct SppfArgs {
  void* buf;                            // the concat buffer (forward: activations, backward: gradients), [B][H*W][ldc]
  int ldc, coff[4];                     // slice i at channel offset coff[i]; pool i reads slice i and writes slice i + 1
  int H, W, C, nchunk;
  unsigned char* amax[3];               // argmax plane of pool i, [B*H*W][C] bytes (forward: null in eval mode)
  int acc[3];                           // backward: slice i already holds a gradient contribution (grad_mode)
};

// EPL argmax codes of one unit <-> the bytes of the plane (bf16: 8 bytes, f32: 4)
template <int EPL> __device__ inline uint2 sppf_ld_codes(const unsigned char* p) {
  if constexpr (EPL == 8) return *(const uint2*)p;
  else return make_uint2(*(const unsigned*)p, 0u);
}
template <int EPL> __device__ inline void sppf_st_codes(unsigned char* p, uint2 v) {
  if constexpr (EPL == 8) *(uint2*)p = v;
  else *(unsigned*)p = v.x;
}

template <class T>
__global__ void __launch_bounds__(SPPF_THREADS)
sppf_pool3_fwd_kernel(SppfArgs a) {
  constexpr int EPL = Elem<T>::EPL;
  T* const buf = (T*)a.buf;
  __shared__ uint4 sV[SPPF_MAXHW * SPPF_CU];        // the stage's input map
  __shared__ uint4 sR[SPPF_MAXHW * SPPF_CU];        // row maxima
  __shared__ unsigned sRI[SPPF_MAXHW * SPPF_CU];    // their kw codes, 3 bits per channel
  const int tid = threadIdx.x;
  const int chunk = (int)blockIdx.x % a.nchunk, b = (int)blockIdx.x / a.nchunk;
  const int HW = a.H * a.W, W = a.W, H = a.H;
  const int nu = sppf_min(SPPF_CU, a.C / EPL - chunk * SPPF_CU);     // units of this chunk that exist (the last chunk may be short)
  const int n = HW * SPPF_CU;
  const long prow = (long)b * HW;
#pragma unroll
  for (int it = 0; it < SPPF_NIT; it++) {
    const int idx = tid + it * SPPF_THREADS;
    const int px = idx >> 2, u = idx & 3;
    if (idx < n && u < nu) sV[idx] = ys_ld16(buf + (prow + px) * a.ldc + a.coff[0] + (chunk * SPPF_CU + u) * EPL);
  }
  __syncthreads();
  for (int s = 0; s < 3; s++) {
    // ---- row pass
#pragma unroll
    for (int it = 0; it < SPPF_NIT; it++) {
      const int idx = tid + it * SPPF_THREADS;
      const int px = idx >> 2, u = idx & 3;
      if (idx < n && u < nu) {
        const int h = px / W, w = px - h * W;
        const int kw0 = sppf_max(0, 2 - w);
        float best[EPL]; unsigned bi[EPL];
#pragma unroll
        for (int e = 0; e < EPL; e++) { best[e] = -INFINITY; bi[e] = (unsigned)kw0; }
#pragma unroll
        for (int kw = 0; kw < 5; kw++) {
          const int iw = sppf_min(sppf_max(w + kw - 2, 0), W - 1);
          const unsigned code = (unsigned)sppf_max(kw, kw0);
          float f[EPL];
          ys_unpack<T>(sV[(h * W + iw) * SPPF_CU + u], f);
#pragma unroll
          for (int e = 0; e < EPL; e++)
            if (f[e] > best[e]) { best[e] = f[e]; bi[e] = code; }
        }
        unsigned ri = 0;
#pragma unroll
        for (int e = 0; e < EPL; e++) ri |= bi[e] << (3 * e);
        sR[idx] = ys_pack<T>(best);            // exact: the maxima are storage values (or -inf)
        sRI[idx] = ri;
      }
    }
    __syncthreads();
    // ---- column pass, first-tap NaN rule, stores
    uint4 out[SPPF_NIT];
#pragma unroll
    for (int it = 0; it < SPPF_NIT; it++) {
      const int idx = tid + it * SPPF_THREADS;
      const int px = idx >> 2, u = idx & 3;
      out[it] = ys_zero16();
      if (idx < n && u < nu) {
        const int h = px / W, w = px - h * W;
        const int kh0 = sppf_max(0, 2 - h), kw0 = sppf_max(0, 2 - w);
        float best[EPL]; unsigned bw[EPL];              // bw: the winning row's code word, its kh in bits 24..26
#pragma unroll
        for (int e = 0; e < EPL; e++) { best[e] = -INFINITY; bw[e] = ((unsigned)kh0 << 24) | ((unsigned)kw0 * 0x249249u); }   // kw0 in every 3-bit field
#pragma unroll
        for (int kh = 0; kh < 5; kh++) {
          const int ih = sppf_min(sppf_max(h + kh - 2, 0), H - 1);
          const int j = (ih * W + w) * SPPF_CU + u;
          const unsigned word = sRI[j] | ((unsigned)sppf_max(kh, kh0) << 24);
          float f[EPL];
          ys_unpack<T>(sR[j], f);
#pragma unroll
          for (int e = 0; e < EPL; e++)
            if (f[e] > best[e]) { best[e] = f[e]; bw[e] = word; }
        }
        float t0[EPL];                                // the first tap of the clipped window
        ys_unpack<T>(sV[(sppf_max(h - 2, 0) * W + sppf_max(w - 2, 0)) * SPPF_CU + u], t0);
        unsigned code[EPL];
#pragma unroll
        for (int e = 0; e < EPL; e++) {
          code[e] = (bw[e] >> 24) * 5u + ((bw[e] >> (3 * e)) & 7u);
          if (t0[e] != t0[e]) { best[e] = t0[e]; code[e] = (unsigned)(kh0 * 5 + kw0); }
        }
        out[it] = ys_pack<T>(best);
        const long row = prow + px;
        const int c = (chunk * SPPF_CU + u) * EPL;
        ys_st16(buf + row * a.ldc + a.coff[s + 1] + c, out[it]);
        if (a.amax[s]) {
          uint2 pk = make_uint2(0u, 0u);
#pragma unroll
          for (int e = 0; e < EPL; e++) (e < 4 ? pk.x : pk.y) |= code[e] << (8 * (e & 3));
          sppf_st_codes<EPL>(a.amax[s] + row * a.C + c, pk);
        }
      }
    }
    __syncthreads();                                // every first-tap read of sV is done
#pragma unroll
    for (int it = 0; it < SPPF_NIT; it++) {
      const int idx = tid + it * SPPF_THREADS;
      if (idx < n && (idx & 3) < nu) sV[idx] = out[it];
    }
    __syncthreads();
  }
}

// G[slice 2] = round(scatter(G[slice 3]) + G[slice 2]), then slice 1 from that, then slice 0: the three maxpool5_bwd_kernel launches with their rounding points
// (fp32 sum of the taps in (kh, kw) order, then the old value, then one rounding to the storage type per stage).  The upstream gradient map and the stage's argmax codes sit in LDS.
template <class T>
__global__ void __launch_bounds__(SPPF_THREADS)
sppf_pool3_bwd_kernel(SppfArgs a) {
  constexpr int EPL = Elem<T>::EPL;
  T* const buf = (T*)a.buf;
  __shared__ uint4 sG[SPPF_MAXHW * SPPF_CU];        // gradient of the stage's pool output
  __shared__ uint2 sA[SPPF_MAXHW * SPPF_CU];        // its argmax codes
  const int tid = threadIdx.x;
  const int chunk = (int)blockIdx.x % a.nchunk, b = (int)blockIdx.x / a.nchunk;
  const int HW = a.H * a.W, W = a.W, H = a.H;
  const int nu = sppf_min(SPPF_CU, a.C / EPL - chunk * SPPF_CU);
  const int n = HW * SPPF_CU;
  const long prow = (long)b * HW;
#pragma unroll
  for (int it = 0; it < SPPF_NIT; it++) {
    const int idx = tid + it * SPPF_THREADS;
    const int px = idx >> 2, u = idx & 3;
    if (idx < n && u < nu) {
      const int c = (chunk * SPPF_CU + u) * EPL;
      sG[idx] = ys_ld16(buf + (prow + px) * a.ldc + a.coff[3] + c);
      sA[idx] = sppf_ld_codes<EPL>(a.amax[2] + (prow + px) * a.C + c);
    }
  }
  __syncthreads();
  for (int s = 2; s >= 0; s--) {
    uint4 out[SPPF_NIT]; uint2 an[SPPF_NIT];
#pragma unroll
    for (int it = 0; it < SPPF_NIT; it++) {
      const int idx = tid + it * SPPF_THREADS;
      const int px = idx >> 2, u = idx & 3;
      out[it] = ys_zero16(); an[it] = make_uint2(0u, 0u);
      if (idx < n && u < nu) {
        const int h = px / W, w = px - h * W;
        const int c = (chunk * SPPF_CU + u) * EPL;
        T* dp = buf + (prow + px) * a.ldc + a.coff[s] + c;
        uint4 old = ys_zero16();
        if (a.acc[s]) old = ys_ld16(dp);            // requested ahead of the taps
        if (s > 0) an[it] = sppf_ld_codes<EPL>(a.amax[s - 1] + (prow + px) * a.C + c);
        float acc[EPL];
#pragma unroll
        for (int e = 0; e < EPL; e++) acc[e] = 0.f;
#pragma unroll 1                            // (five rows of taps unrolled at once spill registers in the f32 instantiation)
        for (int kh = 0; kh < 5; kh++) {
          const int oh = h - kh + 2;                // output whose window holds (h,w) at offset (kh,kw)
          const bool okh = oh >= 0 && oh < H;
          const int ohc = sppf_min(sppf_max(oh, 0), H - 1);
#pragma unroll
          for (int kw = 0; kw < 5; kw++) {
            const int ow = w - kw + 2;
            const bool ok = okh && ow >= 0 && ow < W;
            const int j = (ohc * W + sppf_min(sppf_max(ow, 0), W - 1)) * SPPF_CU + u;
            const unsigned code = ok ? (unsigned)(kh * 5 + kw) : 255u;      // no plane holds 255: a tap outside the map adds nothing
            float g[EPL];
            ys_unpack<T>(sG[j], g);
            const uint2 am = sA[j];
#pragma unroll
            for (int e = 0; e < EPL; e++)
              if ((((e < 4 ? am.x : am.y) >> (8 * (e & 3))) & 0xffu) == code) acc[e] += g[e];
          }
        }
        if (a.acc[s]) {
          float o[EPL];
          ys_unpack<T>(old, o);
#pragma unroll
          for (int e = 0; e < EPL; e++) acc[e] += o[e];
        }
        out[it] = ys_pack<T>(acc);
        ys_st16(dp, out[it]);
      }
    }
    __syncthreads();                                // every read of this stage's map and codes is done
#pragma unroll
    for (int it = 0; it < SPPF_NIT; it++) {
      const int idx = tid + it * SPPF_THREADS;
      if (idx < n && (idx & 3) < nu) { sG[idx] = out[it]; sA[idx] = an[it]; }
    }
    __syncthreads();
  }
}

// the fused form takes maps of at most SPPF_MAXHW pixels whose slices start on 16-byte units and whose argmax planes (null = none) are aligned for the unit's
// code bytes; everything else runs the three launches
int ys_sppf_pool3_ok(int dtype, int H, int W, int C, int ldc, const int* coff, unsigned char* const* argmax) {
  const int epl = dtype == YS_BF16 ? 8 : 4;
  if ((dtype != YS_BF16 && dtype != YS_F32) || H < 1 || W < 1 || H * W > SPPF_MAXHW || C < epl || (C % epl) || (ldc % epl)) return 0;
  for (int i = 0; i < 4; i++) if (coff[i] % epl) return 0;
  for (int i = 0; argmax && i < 3; i++) if ((size_t)argmax[i] % epl) return 0;
  return 1;
}
static SppfArgs sppf_args(int dtype, void* buf, int ldc, const int* coff, int H, int W, int C) {
  SppfArgs a{};
  a.buf = buf; a.ldc = ldc; a.H = H; a.W = W; a.C = C; a.nchunk = ys_cdiv(C / (dtype == YS_BF16 ? 8 : 4), SPPF_CU);
  for (int i = 0; i < 4; i++) a.coff[i] = coff[i];
  return a;
}
int ys_sppf_pool3_fwd_launch(hipStream_t st, int dtype, void* act, int ldc, const int* coff, int B, int H, int W, int C, unsigned char* const* argmax) {
  if (!ys_sppf_pool3_ok(dtype, H, W, C, ldc, coff, argmax)) { ys_set_error("sppf pools: unsupported view"); return YS_ERR_UNSUPPORTED; }
  SppfArgs a = sppf_args(dtype, act, ldc, coff, H, W, C);
  for (int i = 0; i < 3; i++) a.amax[i] = argmax ? argmax[i] : nullptr;
  YsKprofScope prof(st, "sppf_pool3");
  if (dtype == YS_BF16) YS_LAUNCH((sppf_pool3_fwd_kernel<bf16_t>), B * a.nchunk, SPPF_THREADS, st, a);
  else YS_LAUNCH((sppf_pool3_fwd_kernel<float>), B * a.nchunk, SPPF_THREADS, st, a);
  return YS_OK;
}
int ys_sppf_pool3_bwd_launch(hipStream_t st, int dtype, void* grad, int ldc, const int* coff, int B, int H, int W, int C, unsigned char* const* argmax,
                             const int* accumulate) {
  if (!argmax || !argmax[0] || !argmax[1] || !argmax[2] || !ys_sppf_pool3_ok(dtype, H, W, C, ldc, coff, argmax)) { ys_set_error("sppf pools: unsupported view"); return YS_ERR_UNSUPPORTED; }
  SppfArgs a = sppf_args(dtype, grad, ldc, coff, H, W, C);
  for (int i = 0; i < 3; i++) { a.amax[i] = argmax[i]; a.acc[i] = accumulate[i]; }
  YsKprofScope prof(st, "sppf_pool3");
  if (dtype == YS_BF16) YS_LAUNCH((sppf_pool3_bwd_kernel<bf16_t>), B * a.nchunk, SPPF_THREADS, st, a);
  else YS_LAUNCH((sppf_pool3_bwd_kernel<float>), B * a.nchunk, SPPF_THREADS, st, a);
  return YS_OK;
}

// ------------------------------------------------------------------ nearest 2x upsample
template <class T>
__global__ void __launch_bounds__(EW_THREADS)
upsample2x_fwd_kernel(const T* __restrict__ x, int x_ldc, int x_coff, int B, int H, int W, int C, T* __restrict__ y,
                      int y_ldc, int y_coff) {
  constexpr int EPL = Elem<T>::EPL;
  const int CG = C / EPL;
  const int OH = 2 * H, OW = 2 * W;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long n = (long)B * OH * OW * CG;
  if (i >= n) return;
  const int c = (int)(i % CG) * EPL;
  const long pix = i / CG;
  const int ow = (int)(pix % OW);
  const int oh = (int)((pix / OW) % OH);
  const long b = pix / ((long)OW * OH);
  const uint4 v = ys_ld16(x + ((b * H + (oh >> 1)) * W + (ow >> 1)) * x_ldc + x_coff + c);
  ys_st16(y + pix * y_ldc + y_coff + c, v);
}
int ys_upsample2x_fwd_launch(hipStream_t st, int dtype, const void* x, int x_ldc, int x_coff, int B, int H, int W, int C,
                             void* y, int y_ldc, int y_coff) {
  const int epl = dtype == YS_BF16 ? 8 : 4;
  const long n = (long)B * 4 * H * W * (C / epl);
  if (dtype == YS_BF16)
    YS_LAUNCH((upsample2x_fwd_kernel<bf16_t>), ys_cdiv(n, EW_THREADS), EW_THREADS, st, (const bf16_t*)x, x_ldc, x_coff, B, H, W, C, (bf16_t*)y, y_ldc, y_coff);
  else
    YS_LAUNCH((upsample2x_fwd_kernel<float>), ys_cdiv(n, EW_THREADS), EW_THREADS, st, (const float*)x, x_ldc, x_coff, B, H, W, C, (float*)y, y_ldc, y_coff);
  return YS_OK;
}

template <class T>
__global__ void __launch_bounds__(EW_THREADS)
upsample2x_bwd_kernel(const T* __restrict__ dy, int dy_ldc, int dy_coff, int B, int H, int W, int C, T* __restrict__ dx,
                      int dx_ldc, int dx_coff, int accumulate) {
  constexpr int EPL = Elem<T>::EPL;
  const int CG = C / EPL;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long n = (long)B * H * W * CG;
  if (i >= n) return;
  const int c = (int)(i % CG) * EPL;
  const long pix = i / CG;
  const int w = (int)(pix % W);
  const int h = (int)((pix / W) % H);
  const long b = pix / ((long)W * H);
  float acc[EPL];
#pragma unroll
  for (int e = 0; e < EPL; e++) acc[e] = 0.f;
  for (int dh = 0; dh < 2; dh++)
    for (int dw = 0; dw < 2; dw++) {
      float g[EPL];
      ys_unpack<T>(ys_ld16(dy + ((b * 2 * H + 2 * h + dh) * 2 * W + 2 * w + dw) * dy_ldc + dy_coff + c), g);
#pragma unroll
      for (int e = 0; e < EPL; e++) acc[e] += g[e];
    }
  T* dp = dx + pix * dx_ldc + dx_coff + c;
  if (accumulate) {
    float o[EPL];
    ys_unpack<T>(ys_ld16(dp), o);
#pragma unroll
    for (int e = 0; e < EPL; e++) acc[e] += o[e];
  }
  ys_st16(dp, ys_pack<T>(acc));
}
int ys_upsample2x_bwd_launch(hipStream_t st, int dtype, const void* dy, int dy_ldc, int dy_coff, int B, int H, int W,
                             int C, void* dx, int dx_ldc, int dx_coff, int accumulate) {
  const int epl = dtype == YS_BF16 ? 8 : 4;
  const long n = (long)B * H * W * (C / epl);
  if (dtype == YS_BF16)
    YS_LAUNCH((upsample2x_bwd_kernel<bf16_t>), ys_cdiv(n, EW_THREADS), EW_THREADS, st, (const bf16_t*)dy, dy_ldc, dy_coff, B, H, W, C, (bf16_t*)dx, dx_ldc, dx_coff, accumulate);
  else
    YS_LAUNCH((upsample2x_bwd_kernel<float>), ys_cdiv(n, EW_THREADS), EW_THREADS, st, (const float*)dy, dy_ldc, dy_coff, B, H, W, C, (float*)dx, dx_ldc, dx_coff, accumulate);
  return YS_OK;
}

// ------------------------------------------------------------------ view copy / accumulate
template <class T>
__global__ void __launch_bounds__(EW_THREADS)
copy_view_kernel(const T* __restrict__ src, int s_ldc, int s_coff, long rows, int C, T* __restrict__ dst, int d_ldc,
                 int d_coff, int accumulate) {
  constexpr int EPL = Elem<T>::EPL;
  const int CG = C / EPL;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * CG) return;
  const long row = i / CG;
  const int c = (int)(i - row * CG) * EPL;
  uint4 v = ys_ld16(src + row * s_ldc + s_coff + c);
  T* dp = dst + row * d_ldc + d_coff + c;
  if (accumulate) {
    float a[EPL], o[EPL];
    ys_unpack<T>(v, a);
    ys_unpack<T>(ys_ld16(dp), o);
#pragma unroll
    for (int e = 0; e < EPL; e++) a[e] += o[e];
    v = ys_pack<T>(a);
  }
  ys_st16(dp, v);
}
int ys_copy_view_launch(hipStream_t st, int dtype, const void* src, int s_ldc, int s_coff, long rows, int C, void* dst,
                        int d_ldc, int d_coff, int accumulate) {
  const int epl = dtype == YS_BF16 ? 8 : 4;
  const long n = rows * (C / epl);
  if (dtype == YS_BF16)
    YS_LAUNCH((copy_view_kernel<bf16_t>), ys_cdiv(n, EW_THREADS), EW_THREADS, st, (const bf16_t*)src, s_ldc, s_coff, rows, C, (bf16_t*)dst, d_ldc, d_coff, accumulate);
  else
    YS_LAUNCH((copy_view_kernel<float>), ys_cdiv(n, EW_THREADS), EW_THREADS, st, (const float*)src, s_ldc, s_coff, rows, C, (float*)dst, d_ldc, d_coff, accumulate);
  return YS_OK;
}

// ------------------------------------------------------------------ AdamW (torch.optim.AdamW single-tensor maths)
__global__ void __launch_bounds__(EW_THREADS)
adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, long n,
             float lr, float beta1, float beta2, float eps, float wd, float bc1, float bc2_sqrt) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float gi = g[i];
  float pi = p[i] * (1.0f - lr * wd);           // param.mul_(1 - lr*weight_decay)
  const float mi = m[i] + (gi - m[i]) * (1.0f - beta1);  // exp_avg.lerp_(grad, 1-beta1)
  const float vi = beta2 * v[i] + (1.0f - beta2) * gi * gi;
  const float denom = sqrtf(vi) / bc2_sqrt + eps;
  pi -= (lr / bc1) * (mi / denom);
  p[i] = pi; m[i] = mi; v[i] = vi;
}
int ys_adamw_launch(hipStream_t st, float* p, const float* g, float* m, float* v, long n, float lr, float beta1,
                    float beta2, float eps, float wd, float bc1, float bc2) {
  if (n <= 0) return YS_OK;
  YS_LAUNCH(adamw_kernel, ys_cdiv(n, EW_THREADS), EW_THREADS, st, p, g, m, v, n, lr, beta1, beta2, eps, wd, bc1, sqrtf(bc2));
  return YS_OK;
}

// All parameter groups in one launch: the flat parameter vector is a few contiguous [offset, count) ranges (segment x group,
// plan.hip layout_params), each with its own learning rate.
__global__ void __launch_bounds__(EW_THREADS)
adamw_ranges_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, long n,
                    AdamwRanges rg, float beta1, float beta2, float eps, float wd, float bc1, float bc2_sqrt, AdamwDup dup) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float lr = 0.f; bool hit = false;
#pragma unroll
  for (int k = 0; k < YS_ADAMW_MAX_RANGES; k++)
    if (k < rg.n && i >= rg.off[k] && i < rg.off[k] + rg.count[k]) { lr = rg.lr[k]; hit = true; }
  if (!hit) return;
  const float gi = g[i];
  // "reference" parameter groups (YoloBaseTaskModel.cs:144-151 as written): a BatchNorm parameter sits in two groups that share
  // one optimizer state, so one optimizer.step() applies two consecutive AdamW updates with the same gradient -- the second with
  // the bn group's learning rate -- and its step counter advances by two (bias corrections of steps 2t-1 and 2t)
  const bool twice = dup.mask != nullptr && dup.mask[i] != 0;
  const float b1 = twice ? dup.bc1_first : bc1, b2s = twice ? dup.bc2s_first : bc2_sqrt;
  float pi = p[i] * (1.0f - lr * wd);
  float mi = m[i] + (gi - m[i]) * (1.0f - beta1);
  float vi = beta2 * v[i] + (1.0f - beta2) * gi * gi;
  float denom = sqrtf(vi) / b2s + eps;
  pi -= (lr / b1) * (mi / denom);
  if (twice) {
    pi *= (1.0f - dup.lr_second * wd);
    mi = mi + (gi - mi) * (1.0f - beta1);
    vi = beta2 * vi + (1.0f - beta2) * gi * gi;
    denom = sqrtf(vi) / dup.bc2s_second + eps;
    pi -= (dup.lr_second / dup.bc1_second) * (mi / denom);
  }
  p[i] = pi; m[i] = mi; v[i] = vi;
}
int ys_adamw_ranges_launch(hipStream_t st, float* p, const float* g, float* m, float* v, long n, const AdamwRanges& rg,
                           float beta1, float beta2, float eps, float wd, float bc1, float bc2, const AdamwDup* dup) {
  if (n <= 0 || rg.n <= 0) return YS_OK;
  AdamwDup d{};
  if (dup) d = *dup;
  YS_LAUNCH(adamw_ranges_kernel, ys_cdiv(n, EW_THREADS), EW_THREADS, st, p, g, m, v, n, rg, beta1, beta2, eps, wd, bc1, sqrtf(bc2), d);
  return YS_OK;
}

__global__ void __launch_bounds__(EW_THREADS) fill_kernel(float* p, long n, float v) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}
int ys_fill_launch(hipStream_t st, float* p, long n, float v) {
  if (n <= 0) return YS_OK;
  YS_LAUNCH(fill_kernel, ys_cdiv(n, EW_THREADS), EW_THREADS, st, p, n, v);
  return YS_OK;
}

// ------------------------------------------------------------------ Detect._inference decode
// pred[b, 0:4, a] = dist2bbox(DFL(boxes), anchors, xywh) * stride ; pred[b, 4:4+nc, a] = sigmoid(scores)
// (Head.cs:204-223; DFL = softmax over reg_max bins, expectation with weights 0..reg_max-1, Block.cs:40-45)
#define DEC_ANCH 64     // anchors per workgroup
template <class T>
__global__ void __launch_bounds__(EW_THREADS)
detect_decode_kernel(const T* __restrict__ pd, int ld_pd, const T* __restrict__ ps, int ld_ps, int B, int A, int nc,
                     int reg_max, int nl, int o0, int o1, int o2, int w0, int w1, int w2, int s0, int s1, int s2,
                     float* __restrict__ pred, int pred_C, const T* __restrict__ px, int ld_px, int xkind, int nx, int kdim, int xyxy) {
  // One workgroup decodes DEC_ANCH consecutive rows of the [B*A][ld] head outputs: the rows are staged in LDS with
  // coalesced 16-byte loads, (anchor, side) threads take the DFL expectation, and the class probabilities are written
  // channel-major so that consecutive lanes store consecutive anchors of pred[b][c][:].
  constexpr int EPL = Elem<T>::EPL;
  YS_DYN_LDS(lds);
  const int nb = 4 * reg_max;                       // box logits per anchor
  const int pb = nb + 1, pc = nc | 1;               // odd LDS pitches (floats): conflict-free column reads
  float* sB = (float*)lds;                          // [DEC_ANCH][pb]
  float* sC = sB + DEC_ANCH * pb;                   // [DEC_ANCH][pc]
  float* sD = sC + DEC_ANCH * pc;                   // [DEC_ANCH][4]
  const int px_p = nx | 1;
  float* sX = sD + DEC_ANCH * 4;                    // [DEC_ANCH][px_p]: the Obb angle logit / the Pose keypoint outputs
  const int tid = threadIdx.x;
  const long r0 = (long)blockIdx.x * DEC_ANCH;
  const long rows = (long)B * A;
  const int ub = (nb + EPL - 1) / EPL, uc = (nc + EPL - 1) / EPL;
  for (int idx = tid; idx < DEC_ANCH * ub; idx += EW_THREADS) {
    const int r = idx / ub, u = idx - r * ub;
    if (r0 + r < rows) {
      float f[EPL];
      ys_unpack<T>(ys_ld16(pd + (r0 + r) * ld_pd + u * EPL), f);
#pragma unroll
      for (int e = 0; e < EPL; e++) if (u * EPL + e < nb) sB[r * pb + u * EPL + e] = f[e];
    }
  }
  for (int idx = tid; idx < DEC_ANCH * uc; idx += EW_THREADS) {
    const int r = idx / uc, u = idx - r * uc;
    if (r0 + r < rows) {
      float f[EPL];
      ys_unpack<T>(ys_ld16(ps + (r0 + r) * ld_ps + u * EPL), f);
#pragma unroll
      for (int e = 0; e < EPL; e++) if (u * EPL + e < nc) sC[r * pc + u * EPL + e] = f[e];
    }
  }
  if (xkind) {
    const int ux = (nx + EPL - 1) / EPL;
    for (int idx = tid; idx < DEC_ANCH * ux; idx += EW_THREADS) {
      const int r = idx / ux, u = idx - r * ux;
      if (r0 + r < rows) {
        float f[EPL];
        ys_unpack<T>(ys_ld16(px + (r0 + r) * ld_px + u * EPL), f);
#pragma unroll
        for (int e = 0; e < EPL; e++) if (u * EPL + e < nx) sX[r * px_p + u * EPL + e] = f[e];
      }
    }
  }
  __syncthreads();
  {   // DFL expectation: thread = (anchor, side)
    const int r = tid >> 2, sd = tid & 3;
    if (r < DEC_ANCH && r0 + r < rows) {
      const float* row = sB + r * pb + sd * reg_max;
      float mx = -INFINITY;
      for (int j = 0; j < reg_max; j++) mx = fmaxf(mx, row[j]);
      float se = 0.f, sw = 0.f;
      for (int j = 0; j < reg_max; j++) {
        const float e = __expf(row[j] - mx);
        se += e;
        sw += e * (float)j;
      }
      sD[r * 4 + sd] = sw / se;
    }
  }
  __syncthreads();
  if (tid < DEC_ANCH && r0 + tid < rows) {
    const long i = r0 + tid;
    const int a = (int)(i % A);
    const long b = i / A;
    int lo = o0, lw = w0, ls = s0;
    if (nl > 1 && a >= o1) { lo = o1; lw = w1; ls = s1; }
    if (nl > 2 && a >= o2) { lo = o2; lw = w2; ls = s2; }
    const int cell = a - lo;
    const float ax = (float)(cell % lw) + 0.5f, ay = (float)(cell / lw) + 0.5f;
    const float* d = sD + tid * 4;
    const float x1 = ax - d[0], y1 = ay - d[1], x2 = ax + d[2], y2 = ay + d[3];
    float* o = pred + b * (long)pred_C * A + a;
    const float st = (float)ls;
    if (xkind == 2) {
      // Obb (Head.cs:429,435-438): angle = (sigmoid(raw) - 0.25) * pi; boxes = dist2rbox (Tal.cs:389-408) * stride;
      // the angle is appended after the class probabilities (Head.cs:411-418)
      const float ang = (ys_sigmoid(sX[tid * px_p]) - 0.25f) * 3.14159265358979323846f;
      const float cs = cosf(ang), sn = sinf(ang);
      const float xf = (d[2] - d[0]) / 2.0f, yf = (d[3] - d[1]) / 2.0f;
      o[0] = (xf * cs - yf * sn + ax) * st;
      o[(long)A] = (xf * sn + yf * cs + ay) * st;
      o[2 * (long)A] = (d[0] + d[2]) * st;
      o[3 * (long)A] = (d[1] + d[3]) * st;
      o[(long)(4 + nc) * A] = ang;
    } else if (xyxy) {   // End2End: dist2bbox(xywh = false) * stride (Head.cs:199-202, Tal.cs:345-346)
      o[0] = x1 * st;
      o[(long)A] = y1 * st;
      o[2 * (long)A] = x2 * st;
      o[3 * (long)A] = y2 * st;
    } else {
      o[0] = (x1 + x2) / 2.0f * st;
      o[(long)A] = (y1 + y2) / 2.0f * st;
      o[2 * (long)A] = (x2 - x1) * st;
      o[3 * (long)A] = (y2 - y1) * st;
    }
  }
  if (xkind == 3) {   // Pose.kpts_decode (Head.cs:590-605): lane = anchor, the 4 waves stride over the keypoint channels
    const int r = tid & (DEC_ANCH - 1);
    if (r0 + r < rows) {
      const long i = r0 + r;
      const int a = (int)(i % A);
      const long b = i / A;
      int lo = o0, lw = w0, ls = s0;
      if (nl > 1 && a >= o1) { lo = o1; lw = w1; ls = s1; }
      if (nl > 2 && a >= o2) { lo = o2; lw = w2; ls = s2; }
      const int cell = a - lo;
      const float gx = (float)(cell % lw), gy = (float)(cell / lw), st = (float)ls;   // anchors - 0.5
      float* o = pred + b * (long)pred_C * A + (long)(4 + nc) * A + a;
      for (int c = tid / DEC_ANCH; c < nx; c += EW_THREADS / DEC_ANCH) {
        const float v = sX[r * px_p + c];
        const int k = c % kdim;
        o[(long)c * A] = k == 0 ? (v * 2.0f + gx) * st : k == 1 ? (v * 2.0f + gy) * st : k == 2 && kdim == 3 ? ys_sigmoid(v) : v;
      }
    }
  }
  {   // class probabilities: lane = anchor, the 4 waves stride over the classes
    const int r = tid & (DEC_ANCH - 1);
    if (r0 + r < rows) {
      const long i = r0 + r;
      const int a = (int)(i % A);
      const long b = i / A;
      float* o = pred + b * (long)pred_C * A + a;
      for (int c = tid / DEC_ANCH; c < nc; c += EW_THREADS / DEC_ANCH) o[(long)(4 + c) * A] = ys_sigmoid(sC[r * pc + c]);
    }
  }
}
__global__ void __launch_bounds__(EW_THREADS) obb_angle_kernel(float* __restrict__ p, long n) {
  const long i = (long)blockIdx.x * EW_THREADS + threadIdx.x;
  if (i < n) p[i] = (ys_sigmoid(p[i]) - 0.25f) * 3.14159265358979323846f;
}
int ys_obb_angle_launch(hipStream_t st, float* p, long n) {
  if (n > 0) YS_LAUNCH(obb_angle_kernel, ys_cdiv(n, EW_THREADS), EW_THREADS, st, p, n);
  return YS_OK;
}
int ys_detect_decode_launch(hipStream_t st, int dtype, const void* pd, int ld_pd, const void* ps, int ld_ps, int B, int A,
                            int nc, int reg_max, int nl, const int* lo, const int* lw, const int* ls, float* pred, int pred_C,
                            const void* px, int ld_px, int xkind, int nx, int kdim, int xyxy) {
  const long n = (long)B * A;
  const int o1 = nl > 1 ? lo[1] : 0, o2 = nl > 2 ? lo[2] : 0, w1 = nl > 1 ? lw[1] : 1, w2 = nl > 2 ? lw[2] : 1;
  const int s1 = nl > 1 ? ls[1] : 1, s2 = nl > 2 ? ls[2] : 1;
  if (!px) xkind = 0;
  if (!xkind) nx = 0;
  const size_t lds_bytes = (size_t)DEC_ANCH * ((4 * reg_max + 1) + (nc | 1) + 4 + (nx | 1)) * 4;
  if (lds_bytes > 60 * 1024 || DEC_ANCH * 4 > EW_THREADS) { ys_set_error("detect decode: nc=%d reg_max=%d too large", nc, reg_max); return YS_ERR_UNSUPPORTED; }
  if (dtype == YS_BF16)
    YS_LAUNCH_LDS((detect_decode_kernel<bf16_t>), ys_cdiv(n, DEC_ANCH), EW_THREADS, lds_bytes, st, (const bf16_t*)pd, ld_pd, (const bf16_t*)ps, ld_ps, B, A, nc, reg_max, nl, lo[0], o1, o2, lw[0], w1, w2, ls[0], s1, s2, pred, pred_C, (const bf16_t*)px, ld_px, xkind, nx, kdim, xyxy);
  else
    YS_LAUNCH_LDS((detect_decode_kernel<float>), ys_cdiv(n, DEC_ANCH), EW_THREADS, lds_bytes, st, (const float*)pd, ld_pd, (const float*)ps, ld_ps, B, A, nc, reg_max, nl, lo[0], o1, o2, lw[0], w1, w2, ls[0], s1, s2, pred, pred_C, (const float*)px, ld_px, xkind, nx, kdim, xyxy);
  return YS_OK;
}
