// sentinel_check.cpp -- the predicate every `view_intact` of the per-operator entry points rests on (csrc/sentinel_check.h), on hand-made buffers.
// Every test that reads view_intact asserts 1; this program shows that the checker can answer 0: one byte off before the view, behind it, between two views
// of a shared buffer, in the last row -- for element sizes 1, 2 and 4 -- and that a view as wide as its buffer leaves nothing to check.
#include "sentinel_check.h"
#include <cstdio>
#include <vector>

static const unsigned char S = 0x4E;
static int failures = 0;

static void expect(bool got, bool want, const char* what, size_t es) {
  if (got == want) return;
  std::printf("FAIL: %s (element size %zu): the checker says %d, expected %d\n", what, es, (int)got, (int)want);
  failures++;
}

// a [rows][ld] buffer of es-byte elements: the sentinel everywhere, data (never the sentinel byte) in the channel ranges v[k] = {coff, C}
static std::vector<unsigned char> make(size_t rows, size_t ld, size_t es, const size_t (*v)[2], int nv) {
  std::vector<unsigned char> h(rows * ld * es, S);
  for (size_t r = 0; r < rows; r++)
    for (int k = 0; k < nv; k++)
      for (size_t i = v[k][0] * es; i < (v[k][0] + v[k][1]) * es; i++) h[r * ld * es + i] = (unsigned char)(i * 7 + r) == S ? 0 : (unsigned char)(i * 7 + r);
  return h;
}

int main() {
  const size_t sizes[3] = {1, 2, 4};
  for (size_t es : sizes) {
    const size_t rows = 5, ld = 24, pitch = ld * es;
    const size_t one[1][2] = {{8, 8}}, two[2][2] = {{4, 4}, {16, 4}};           // one view in the middle; two views of a shared buffer with a gap between them
    const YsByteRange r1[1] = {{8 * es, 16 * es}}, r2[2] = {{4 * es, 8 * es}, {16 * es, 20 * es}};
    std::vector<unsigned char> h = make(rows, ld, es, one, 1);
    expect(ys_sentinel_intact(h.data(), rows, pitch, r1, 1, S), true, "intact", es);
    expect(ys_sentinel_intact(h.data(), rows, pitch, nullptr, 0, S), false, "the view's own data counts when no range is skipped", es);

    h = make(rows, ld, es, one, 1);
    h[2 * pitch + 8 * es - 1] ^= 1;                     // the last byte before the view, row 2
    expect(ys_sentinel_intact(h.data(), rows, pitch, r1, 1, S), false, "one byte off before the view", es);

    h = make(rows, ld, es, one, 1);
    h[2 * pitch + 16 * es] ^= 1;                        // the first byte behind it
    expect(ys_sentinel_intact(h.data(), rows, pitch, r1, 1, S), false, "one byte off after the view", es);

    h = make(rows, ld, es, one, 1);
    h[rows * pitch - 1] ^= 0x80;                        // the very last byte of the buffer
    expect(ys_sentinel_intact(h.data(), rows, pitch, r1, 1, S), false, "one byte off in the last row", es);
    h = make(rows, ld, es, one, 1);
    h[(rows - 1) * pitch] = 0;                          // the first byte of the last row
    expect(ys_sentinel_intact(h.data(), rows, pitch, r1, 1, S), false, "one byte off at the start of the last row", es);

    h = make(rows, ld, es, two, 2);
    expect(ys_sentinel_intact(h.data(), rows, pitch, r2, 2, S), true, "two views of a shared buffer, intact", es);
    expect(ys_sentinel_intact(h.data(), rows, pitch, r2, 1, S), false, "the second view's data counts when only the first is skipped", es);
    h[3 * pitch + 12 * es] ^= 1;                        // between the two views
    expect(ys_sentinel_intact(h.data(), rows, pitch, r2, 2, S), false, "one byte off between two views of a shared buffer", es);

    const size_t full[1][2] = {{0, ld}};                // ld == C: nothing outside the view
    const YsByteRange rf[1] = {{0, pitch}};
    h = make(rows, ld, es, full, 1);
    expect(ys_sentinel_intact(h.data(), rows, pitch, rf, 1, S), true, "ld == C: nothing to check", es);

    std::vector<unsigned char> g(256, S);               // a guard: one row, no range
    expect(ys_sentinel_intact(g.data(), 1, g.size(), nullptr, 0, S), true, "guard intact", es);
    g[255] = 0;
    expect(ys_sentinel_intact(g.data(), 1, g.size(), nullptr, 0, S), false, "guard: last byte off", es);
  }
  expect(ys_sentinel_intact(nullptr, 0, 16, nullptr, 0, S), true, "no rows", 1);
  if (failures) return 1;
  std::printf("sentinel_check OK\n");
  return 0;
}
