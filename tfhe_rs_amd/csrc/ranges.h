// ranges.h — what the library derived from a range of device memory and must forget when that range is freed or written
#pragma once
#include <cstddef>
#include <mutex>
#include <vector>

namespace tfhe_hip {

// [base, base + bytes) of device `dev` meets [p, p + n) of `device` (n = 0: the one byte at p)
inline bool range_overlaps(int dev, const void *base, size_t bytes, int device, const void *p, size_t n) {
  const char *lo = (const char *)p, *hi = lo + (n ? n : 1), *klo = (const char *)base;
  return dev == device && klo < hi && lo < klo + bytes;
}

template <class Payload>
class RangeRegistry {
 public:
  void add(int device, const void *base, size_t bytes, const Payload &payload) {
    std::lock_guard<std::mutex> lock(mu_);
    entries_.push_back(Entry{device, base, bytes, payload});
  }
  bool find(int device, const void *base, Payload *out) {
    std::lock_guard<std::mutex> lock(mu_);
    for (const Entry &e : entries_)
      if (e.device == device && e.base == base) {
        *out = e.payload;
        return true;
      }
    return false;
  }
  // unlinks what overlaps [p, p + bytes) under the lock; the caller releases the payloads outside it
  std::vector<Payload> take_overlapping(int device, const void *p, size_t bytes) {
    std::vector<Payload> taken;
    if (p == nullptr) return taken;
    std::lock_guard<std::mutex> lock(mu_);
    for (size_t i = 0; i < entries_.size();) {
      if (range_overlaps(entries_[i].device, entries_[i].base, entries_[i].bytes, device, p, bytes)) {
        taken.push_back(entries_[i].payload);
        entries_.erase(entries_.begin() + i);
      } else {
        ++i;
      }
    }
    return taken;
  }
  bool empty() {
    std::lock_guard<std::mutex> lock(mu_);
    return entries_.empty();
  }

 private:
  struct Entry {
    int device;
    const void *base;  // [base, base + bytes)
    size_t bytes;
    Payload payload;
  };
  std::mutex mu_;
  std::vector<Entry> entries_;
};

}  // namespace tfhe_hip
