// mxfp6_selftest: the MXFP6 host codec (core/mxfp6.h) under Address and
// UndefinedBehavior sanitizer (make sanitize-mxfp6). Every buffer is a heap
// allocation of exactly the size the format defines, so a 6-bit extraction
// that reads past a block, a chunk's q region or the layer is reported:
//   * pack / unpack of one chunk of 1, 3, 7 and 64 blocks;
//   * a layer of 64 * 1031 B in 4096-B chunks (16 full chunks and a tail of 7
//     blocks, an odd count): pack_layer, unpack_layer, and unpack_range at
//     offsets and lengths that start and end inside a block, inside a code that
//     straddles two bytes, across a chunk edge and in the tail chunk, each
//     compared with the slice of the whole layer;
//   * all 65536 bf16 patterns: unpack(pack(x)) is a fixed point of pack.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "core/mxfp6.h"

using namespace dissem;

static int failures = 0;
#define EXPECT(c)                                                    \
  do {                                                               \
    if (!(c)) {                                                      \
      ++failures;                                                    \
      fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);   \
    }                                                                \
  } while (0)

// exact-size heap arrays (a std::vector may round its capacity up)
template <class T>
static std::unique_ptr<T[]> exact(size_t n) {
  return std::unique_ptr<T[]>(new T[n ? n : 1]);
}

static uint64_t splitmix(uint64_t& s) {
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static void fill(uint16_t* x, int64_t n, uint64_t seed, bool nans) {
  for (int64_t i = 0; i < n; ++i) {
    uint16_t v = uint16_t(splitmix(seed));
    if (!nans && (v & 0x7FFF) > 0x7F80) v &= 0xBFFF;
    x[i] = v;
  }
}

static void one_chunk(int64_t blocks) {
  const int64_t n = blocks * 32;
  auto x = exact<uint16_t>(size_t(n)), y = exact<uint16_t>(size_t(n));
  auto q = exact<uint8_t>(size_t(blocks * 24)), s = exact<uint8_t>(size_t(blocks));
  fill(x.get(), n, uint64_t(blocks), false);
  mxfp6::pack_host(x.get(), n, q.get(), s.get());
  mxfp6::unpack_host(q.get(), s.get(), n, y.get());
  for (int64_t b = 0; b < blocks; ++b) {
    EXPECT(s[b] >= 1 && s[b] <= 252);
    for (int i = 0; i < 32; ++i) {
      const uint8_t code = mxfp6::get_code(q.get() + 24 * b, i);
      EXPECT((code >> 5) == (x[32 * b + i] >> 15));               // the sign is kept
      EXPECT((y[32 * b + i] & 0x7FFF) < 0x7F80);                  // finite
    }
  }
}

static void layer_and_ranges() {
  const int64_t src = 64 * 1031, chunk = 4096, total = src / 2;
  const int64_t psize = mxfp6::packed_size(src, chunk);
  EXPECT(psize == 16 * 1600 + 7 * 25);
  EXPECT(mxfp6::source_size(psize, chunk) == src);
  auto x = exact<uint16_t>(size_t(total)), whole = exact<uint16_t>(size_t(total));
  auto packed = exact<uint8_t>(size_t(psize));
  fill(x.get(), total, 11, false);
  x[40] = 0x7FC0;          // a NaN block in chunk 0
  x[total - 3] = 0xFFC1;   // and the last block of the odd tail
  mxfp6::pack_layer_host(reinterpret_cast<const uint8_t*>(x.get()), src, chunk, packed.get());
  mxfp6::unpack_layer_host(packed.get(), src, chunk, reinterpret_cast<uint8_t*>(whole.get()));
  for (int i = 32; i < 64; ++i) EXPECT(whole[i] == 0x7FC0);
  for (int64_t i = total - 32; i < total; ++i) EXPECT(whole[i] == 0x7FC0);
  const int64_t ranges[][2] = {{7, 1}, {1, 1}, {33, 2}, {2, 4}, {5, 30}, {32, 32}, {2040, 20}, {2047, 2},
                               {2048 * 3 - 1, 2048 + 2}, {32768 + 5, 200}, {32768 + 192 + 1, 31}, {32768 + 223, 1},
                               {0, total}, {total, 0}, {500, 100}, {total - 1, 1}};
  for (auto& r : ranges) {
    auto got = exact<uint16_t>(size_t(r[1]));
    mxfp6::unpack_range_host(packed.get(), src, chunk, r[0], r[1], got.get());
    EXPECT(memcmp(got.get(), whole.get() + r[0], size_t(r[1]) * 2) == 0);
  }
  // every single element of the tail chunk and of the chunk edge before it
  for (int64_t e = 32768 - 40; e < total; ++e) {
    uint16_t one;
    mxfp6::unpack_range_host(packed.get(), src, chunk, e, 1, &one);
    EXPECT(one == whole[e]);
  }
  const int64_t bad[][2] = {{total - 31, 32}, {-1, 1}, {0, total + 1}, {total + 1, 0}};
  for (auto& r : bad) {
    bool threw = false;
    try {
      uint16_t sink[32];
      mxfp6::unpack_range_host(packed.get(), src, chunk, r[0], r[1], sink);
    } catch (const std::runtime_error&) {
      threw = true;
    }
    EXPECT(threw);
  }
  bool threw = false;
  try {
    mxfp6::check(96, 4096);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  EXPECT(threw);
}

static void fixed_point() {
  const int64_t n = 65536, src = 2 * n, chunk = src;
  auto x = exact<uint16_t>(size_t(n)), y = exact<uint16_t>(size_t(n)), z = exact<uint16_t>(size_t(n));
  const int64_t psize = mxfp6::packed_size(src, chunk);
  auto p = exact<uint8_t>(size_t(psize)), again = exact<uint8_t>(size_t(psize));
  for (int64_t i = 0; i < n; ++i) x[i] = uint16_t(i);
  mxfp6::pack_layer_host(reinterpret_cast<const uint8_t*>(x.get()), src, chunk, p.get());
  mxfp6::unpack_layer_host(p.get(), src, chunk, reinterpret_cast<uint8_t*>(y.get()));
  mxfp6::pack_layer_host(reinterpret_cast<const uint8_t*>(y.get()), src, chunk, again.get());
  mxfp6::unpack_layer_host(again.get(), src, chunk, reinterpret_cast<uint8_t*>(z.get()));
  EXPECT(memcmp(y.get(), z.get(), size_t(src)) == 0);
  for (int64_t i = 0; i < n; ++i) EXPECT((y[i] & 0x7FFF) != 0x7F80);  // nothing packed unpacks to inf
}

int main() {
  for (int64_t b : {1, 3, 7, 64}) one_chunk(b);
  layer_and_ranges();
  fixed_point();
  if (failures) {
    fprintf(stderr, "mxfp6_selftest: %d failure(s)\n", failures);
    return 1;
  }
  printf("mxfp6_selftest ok\n");
  return 0;
}
