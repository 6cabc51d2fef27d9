// sentinel_check.h -- the predicate every `view_intact` of the per-operator entry points rests on (ops_stage.h calls it for padded views and for guards).
// No HIP include: tests/c/sentinel_check.cpp builds it with plain g++ and shows that it can answer "no".
#pragma once
#include <cstddef>

struct YsByteRange { size_t lo, hi; };       // bytes [lo, hi) of every row

// h: host copy of a [rows][pitch] byte buffer.  True when every byte outside the n_skip ranges of its row is still `sentinel`.
inline bool ys_sentinel_intact(const unsigned char* h, size_t rows, size_t pitch, const YsByteRange* skip, int n_skip, unsigned char sentinel) {
  for (size_t r = 0; r < rows; r++)
    for (size_t i = 0; i < pitch; i++) {
      bool skipped = false;
      for (int k = 0; k < n_skip; k++) skipped |= i >= skip[k].lo && i < skip[k].hi;
      if (!skipped && h[r * pitch + i] != sentinel) return false;
    }
  return true;
}
