// conv_tl.h -- host side of the timeline stamps of the convolution kernels (triage builds only: -DYS_P2_TIMELINE, `build.py timeline`).  With
// $YS_P2_TL set a launch gets a cleared stamp buffer in ConvArgs::tl (64 slots for each of up to 64 recorded workgroups, every 37th of the grid);
// afterwards the launcher waits for the kernel and appends its own header line and one "wg<i>:" line of cycle offsets per recorded workgroup to
// that file.  The product build sees nothing of this.
#pragma once
#ifdef YS_P2_TIMELINE
#include "ys_kernels.h"
#include <cstdio>
#include <cstdlib>

// before the launch: the path to dump to (null = off) with a.tl pointing at the cleared buffer
inline const char* ys_tl_begin(hipStream_t st, ConvArgs& a) {
  static unsigned long long* tl_buf = nullptr;
  const char* tl_path = getenv("YS_P2_TL");
  if (tl_path) {
    if (!tl_buf) hipMalloc(&tl_buf, 64 * 64 * 8);
    hipMemsetAsync(tl_buf, 0, 64 * 64 * 8, st);
    a.tl = tl_buf;
  }
  return tl_path;
}

// after the launch of gx workgroup columns: the header line (printf style, without the newline) and the stamps
template <class... Args>
inline void ys_tl_dump(hipStream_t st, const char* tl_path, const ConvArgs& a, int gx, const char* header, Args... args) {
  if (!tl_path) return;
  static unsigned long long h[64 * 64];
  hipStreamSynchronize(st);
  hipMemcpy(h, a.tl, sizeof(h), hipMemcpyDeviceToHost);
  FILE* f = fopen(tl_path, "a");
  if (!f) return;
  fprintf(f, header, args...);
  fprintf(f, "\n");
  for (int w = 0; w < 64 && w * 37 < gx; w++) {
    const int n = (int)h[w * 64];
    if (n <= 0) continue;
    fprintf(f, "wg%d:", w * 37);
    for (int i = 1; i < n; i++) fprintf(f, " %llu", h[w * 64 + 1 + i] - h[w * 64 + 1]);
    fprintf(f, "\n");
  }
  fclose(f);
}
#endif
