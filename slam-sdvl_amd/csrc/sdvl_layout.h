// sdvl_layout.h — how the launch code cuts one buffer into typed parts (host only; no allocation, size_t throughout).  A layout is
// stated once, before any base pointer exists; the allocation, the host fill, the kernel arguments and the copy back all take their
// pointers and sizes from the same parts.  Every part starts on a 256-byte boundary.
#ifndef SDVL_LAYOUT_H_
#define SDVL_LAYOUT_H_

#include <stddef.h>
#include <stdint.h>

inline size_t sdvl_align256(size_t v) { return (v + 255) / 256 * 256; }

template <typename T>
struct sdvl_part {
  size_t off = 0, count = 0;  // byte offset inside the buffer, elements
  size_t bytes() const { return sizeof(T) * count; }  // what the elements take, without the padding behind them
  T *in(void *base) const { return reinterpret_cast<T *>(static_cast<uint8_t *>(base) + off); }
  const T *cin(const void *base) const { return reinterpret_cast<const T *>(static_cast<const uint8_t *>(base) + off); }
};

struct sdvl_layout {
  size_t size = 0;
  template <typename T>
  sdvl_part<T> take(size_t count) {
    const sdvl_part<T> p{size, count};
    size = sdvl_align256(size + p.bytes());
    return p;
  }
  size_t bytes() const { return size; }  // all parts, the last one padded like the others
};

#endif  // SDVL_LAYOUT_H_
