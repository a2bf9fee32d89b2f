// layout_check.cc — sdvl_layout.h on its own, built with the host compiler under AddressSanitizer and UBSan (test_layout_cpu.py).
// For lists of parts: every offset is the running sum of the sizes rounded up to 256, every part starts 256-aligned, bytes() is that
// sum; then a block of bytes() is allocated, every part is filled with a pattern of its own and all are read back — parts that
// overlapped would disturb each other's pattern, a part outside the block is what the sanitizer reports.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "sdvl_layout.h"

#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);          \
      exit(1);                                                            \
    }                                                                     \
  } while (0)

template <int N>
struct Rec {
  uint8_t b[N];
};

static size_t round256(size_t v) { return (v + 255) & ~static_cast<size_t>(255); }

struct Taken {
  size_t off, bytes;
};

// takes `count` elements of T, checks the part against the running sum, records it
template <typename T>
static void take(sdvl_layout &L, size_t count, size_t &sum, std::vector<Taken> &parts) {
  const sdvl_part<T> p = L.take<T>(count);
  CHECK(p.off == sum);
  CHECK(p.off % 256 == 0);
  CHECK(p.count == count);
  CHECK(p.bytes() == sizeof(T) * count);
  uint8_t probe[1];
  CHECK(reinterpret_cast<uint8_t *>(p.in(probe)) == probe + p.off);
  CHECK(reinterpret_cast<const uint8_t *>(p.cin(probe)) == probe + p.off);
  sum += round256(sizeof(T) * count);
  CHECK(L.bytes() == sum);
  parts.push_back(Taken{p.off, p.bytes()});
}

static void fill_and_read_back(const sdvl_layout &L, const std::vector<Taken> &parts) {
  uint8_t *block = static_cast<uint8_t *>(malloc(L.bytes() ? L.bytes() : 1));
  CHECK(block != nullptr);
  for (size_t i = 0; i < parts.size(); i++) memset(block + parts[i].off, static_cast<int>(0x11 * (i + 1)), parts[i].bytes);
  for (size_t i = 0; i < parts.size(); i++)
    for (size_t k = 0; k < parts[i].bytes; k++) CHECK(block[parts[i].off + k] == static_cast<uint8_t>(0x11 * (i + 1)));
  free(block);
}

int main() {
  CHECK(sdvl_align256(0) == 0 && sdvl_align256(1) == 256 && sdvl_align256(255) == 256 && sdvl_align256(256) == 256 && sdvl_align256(257) == 512);
  {  // nothing taken
    sdvl_layout L;
    CHECK(L.bytes() == 0);
  }
  {  // counts 0 and 1, byte sizes 255, 256 and 257, in one list: an empty part shares its offset with the next one
    sdvl_layout L;
    size_t sum = 0;
    std::vector<Taken> parts;
    take<double>(L, 0, sum, parts);
    take<double>(L, 1, sum, parts);
    take<Rec<255>>(L, 1, sum, parts);
    take<Rec<256>>(L, 1, sum, parts);
    take<Rec<257>>(L, 1, sum, parts);
    take<uint8_t>(L, 255, sum, parts);
    take<uint8_t>(L, 256, sum, parts);
    take<uint8_t>(L, 257, sum, parts);
    take<Rec<255>>(L, 0, sum, parts);
    take<int32_t>(L, 64, sum, parts);  // exactly 256
    take<int32_t>(L, 65, sum, parts);  // one element more
    take<uint16_t>(L, 1, sum, parts);
    CHECK(sum == 0 + 256 + 256 + 256 + 512 + 256 + 256 + 512 + 0 + 256 + 512 + 256);
    fill_and_read_back(L, parts);
  }
  for (size_t size : {255, 256, 257}) {  // each size alone and last: bytes() pads the last part like the others
    sdvl_layout L;
    size_t sum = 0;
    std::vector<Taken> parts;
    take<uint8_t>(L, size, sum, parts);
    CHECK(L.bytes() == round256(size));
    fill_and_read_back(L, parts);
  }
  {  // 2^31 eight-byte elements: 16 GiB, past every 32-bit count and byte offset; arithmetic only (nothing that size is allocated)
    sdvl_layout L;
    size_t sum = 0;
    std::vector<Taken> parts;
    const size_t big = static_cast<size_t>(1) << 31;
    take<uint8_t>(L, 1, sum, parts);
    take<double>(L, big, sum, parts);
    take<double>(L, big + 1, sum, parts);
    take<int32_t>(L, 1, sum, parts);
    CHECK(parts[2].off == 256 + 8 * big);
    CHECK(parts[3].off == 256 + 8 * big + 8 * big + 256);
    CHECK(L.bytes() == 256 + 16 * big + 256 + 256);
    CHECK(L.bytes() > (static_cast<size_t>(1) << 34));
  }
  printf("layout ok\n");
  return 0;
}
