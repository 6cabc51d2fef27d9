// ops_stage.h -- host-side staging of the entry points that take host arrays: the scoped device buffer, the copies, and the sentinel-padded view the
// per-kernel test entries (ops_conv / ops_bn / ops_attn_dw.hip) place their operands in.  Host code only; no kernel lives here.
#pragma once
#include "ys_internal.h"
#include "ys_kernels.h"
#include "sentinel_check.h"
#include <cstring>
#include <vector>

// device scratch of the host-pointer paths: freed on every exit path (an early return on a later allocation or copy used to leak the earlier ones)
struct DevBuf {
  void* p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
  hipError_t alloc_hip(size_t n) { return hipMalloc(&p, n ? n : 16); }       // for the callers that report YS_ERR_HIP (core.hip)
  int alloc(size_t n) { return alloc_hip(n) == hipSuccess ? YS_OK : YS_ERR_OOM; }
  template <class U> U* as() const { return (U*)p; }
};

inline int h2d(hipStream_t st, void* d, const void* h, size_t bytes) { YS_CHECK_HIP(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, st)); return YS_OK; }
inline int d2h(hipStream_t st, void* h, const void* d, size_t bytes) { YS_CHECK_HIP(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, st)); return YS_OK; }

constexpr int kSentinelByte = 0x4E;          // bf16 0x4E4E = fp32 0x4E4E4E4E = 8.65e8: finite, and ruinous when a kernel reads it as data
constexpr size_t kGuardFloats = 64;          // sentinel floats behind a workspace matrix or an output array
inline int ys_epl(int dtype) { return dtype == YS_BF16 ? 8 : 4; }          // elements of a 16-byte vector
inline size_t ys_es(int dtype) { return dtype == YS_BF16 ? 2 : 4; }
inline int ys_round_up(int n, int m) { return (n + m - 1) / m * m; }

inline int alloc_filled(DevBuf& b, size_t bytes, hipStream_t st) {
  YS_TRY(b.alloc(bytes));
  YS_CHECK_HIP(hipMemsetAsync(b.p, kSentinelByte, bytes ? bytes : 16, st));
  return YS_OK;
}

// fp32 NCHW host tensor [B][C][rpb] -> channels [coff, coff + C) of the pre-filled [B*rpb][ld] device buffer `wide`
inline int stage_view(hipStream_t st, int dtype, const float* host, int B, int C, long rpb, void* wide, int ld, int coff) {
  const int epl = ys_epl(dtype);
  const size_t es = ys_es(dtype);
  const long rows = (long)B * rpb;
  DevBuf d32, compact;
  YS_TRY(d32.alloc((size_t)rows * C * 4));
  YS_TRY(compact.alloc((size_t)rows * C * es));
  YS_TRY(h2d(st, d32.p, host, (size_t)rows * C * 4));
  YS_TRY(ys_pack_input_launch(st, dtype, (const float*)d32.p, B, C, 1, (int)rpb, C, compact.p));
  if (ld % epl == 0 && coff % epl == 0) {
    YS_TRY(ys_copy_view_launch(st, dtype, compact.p, C, 0, rows, C, wide, ld, coff, 0));
  } else {
    // a pitch off the 16-byte grid (the scalar attention kernels accept it; ys_copy_view_launch moves 16-byte vectors): rows placed by the host
    std::vector<char> hc((size_t)rows * C * es), hw((size_t)rows * ld * es);
    YS_TRY(d2h(st, hc.data(), compact.p, hc.size()));
    YS_TRY(d2h(st, hw.data(), wide, hw.size()));
    YS_CHECK_HIP(hipStreamSynchronize(st));
    for (long r = 0; r < rows; r++) memcpy(hw.data() + ((size_t)r * ld + coff) * es, hc.data() + (size_t)r * C * es, (size_t)C * es);
    YS_TRY(h2d(st, wide, hw.data(), hw.size()));
  }
  YS_CHECK_HIP(hipStreamSynchronize(st));      // d32 / compact are temporaries of this scope
  return YS_OK;
}

// channels [coff, coff + C) of a [B*rpb][ld] device buffer -> fp32 NCHW host tensor
inline int fetch_view(hipStream_t st, int dtype, const void* wide, int ld, int coff, int B, int C, long rpb, float* host) {
  DevBuf d32;
  const size_t n = (size_t)B * C * rpb;
  YS_TRY(d32.alloc(n * 4));
  YS_TRY(ys_unpack_nchw_launch(st, dtype, wide, ld, coff, B, C, rpb, (float*)d32.p));
  YS_TRY(d2h(st, host, d32.p, n * 4));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  return YS_OK;
}

// *ok &= every byte of the [rows][ld] buffer of es-byte elements outside the nv channel ranges v[k] = {coff, C} is still the sentinel.  Synchronizes.
inline int check_sentinel(hipStream_t st, const void* wide, long rows, int ld, size_t es, const int (*v)[2], int nv, int* ok) {
  std::vector<unsigned char> h((size_t)rows * ld * es);
  std::vector<YsByteRange> skip;
  for (int k = 0; k < nv; k++) skip.push_back(YsByteRange{(size_t)v[k][0] * es, (size_t)(v[k][0] + v[k][1]) * es});
  YS_TRY(d2h(st, h.data(), wide, h.size()));
  YS_CHECK_HIP(hipStreamSynchronize(st));
  if (!ys_sentinel_intact(h.data(), (size_t)rows, (size_t)ld * es, skip.data(), nv, kSentinelByte)) *ok = 0;
  return YS_OK;
}
// ... and the kGuardFloats * 4 bytes behind the `bytes` bytes of an array
inline int check_guard(hipStream_t st, const void* base, size_t bytes, int* ok) {
  return check_sentinel(st, (const char*)base + bytes, 1, (int)kGuardFloats * 4, 1, nullptr, 0, ok);
}

// ---- what the fp8 entries share: the YS_AMAX_WAYS slots of one tensor, zeroed, with a sentinel guard behind them
inline int alloc_slots(DevBuf& b, hipStream_t st) {
  YS_TRY(alloc_filled(b, (YS_AMAX_WAYS + kGuardFloats) * 4, st));
  YS_CHECK_HIP(hipMemsetAsync(b.p, 0, YS_AMAX_WAYS * 4, st));
  return YS_OK;
}
// slots -> host (optional), *amax = their maximum, guard checked
inline int fetch_slots(hipStream_t st, const DevBuf& b, float* slots, float* amax, int* ok) {
  float h[YS_AMAX_WAYS];
  YS_TRY(d2h(st, h, b.p, sizeof h));
  YS_TRY(check_guard(st, b.p, sizeof h, ok));      // synchronizes
  float m = 0.f;
  for (int i = 0; i < YS_AMAX_WAYS; i++) { if (slots) slots[i] = h[i]; m = h[i] > m ? h[i] : m; }
  *amax = m;
  return YS_OK;
}
inline int scalar_to_device(hipStream_t st, DevBuf& b, float v) {
  YS_TRY(b.alloc(16));
  YS_TRY(h2d(st, b.p, &v, 4));
  YS_CHECK_HIP(hipStreamSynchronize(st));     // v is the caller's local
  return YS_OK;
}

// THE vector-grid condition of a padded view: C channels from channel coff of rows of ld elements, pitch and offset whole 16-byte vectors.
// A caller that takes (pad, coff) passes ld = coff + C + pad.
inline int view_on_grid(const char* who, int dtype, int C, int ld, int coff) {
  const int epl = ys_epl(dtype);
  YS_REQUIRE(coff >= 0 && ld >= coff + C && ld % epl == 0 && coff % epl == 0, "%s: view (ldc %d, coff %d) must hold C=%d channels on the %d-element vector grid",
             who, ld, coff, C, epl);
  return YS_OK;
}

// Channels [coff, coff + C) of a [rows][ld] device buffer, as an operand sits in one of the model's shared activation buffers; everything outside the view
// is a sentinel that must survive the call.  The view owns its buffer, or borrows another view's (`res` in other channels of `z`'s buffer).
struct PadView {
  DevBuf own;
  void* p = nullptr;
  long rows = 0;
  int dtype = YS_F32, ld = 0, coff = 0, C = 0;

  int alloc(hipStream_t st, int dtype_, long rows_, int C_, int ld_, int coff_) {
    dtype = dtype_; rows = rows_; C = C_; ld = ld_; coff = coff_;
    YS_TRY(alloc_filled(own, (size_t)rows * ld * ys_es(dtype), st));
    p = own.p;
    return YS_OK;
  }
  void borrow(const PadView& o, int coff_) { p = o.p; dtype = o.dtype; rows = o.rows; C = o.C; ld = o.ld; coff = coff_; }
  // from / to an fp32 channel-major host tensor [B][C][rows / B]
  int stage(hipStream_t st, const float* host, int B = 1) const { return stage_view(st, dtype, host, B, C, rows / B, p, ld, coff); }
  int fetch(hipStream_t st, float* host, int B = 1) const { return fetch_view(st, dtype, p, ld, coff, B, C, rows / B, host); }
  // *ok &= everything outside my channels -- and those of `sharing`, a view that borrows my buffer -- is still the sentinel
  int check(hipStream_t st, int* ok, const PadView* sharing = nullptr) const {
    if (ld == C) return YS_OK;
    const int v[2][2] = {{coff, C}, {sharing ? sharing->coff : 0, sharing ? sharing->C : 0}};
    return check_sentinel(st, p, rows, ld, ys_es(dtype), v, sharing ? 2 : 1, ok);
  }
};
