// What every host-side check of a call's device buffers shares: the byte span of a buffer, the extent of a pitched plane and the overlap sweep.  Plain C++ — the
// multi-geometry request (geoms_request.hpp), the NV12 output records (vcam_nv12_plan.hpp) and the n-picture image batches (picture_batch_plan.hpp) include it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace bsx {
// the bytes from a plane's first to one past its last byte: `rows` rows of `w` bytes, `pitch` apart
inline size_t vcam_nv12_extent(int pitch, int rows, int w) { return (size_t)pitch * (size_t)(rows - 1) + (size_t)w; }

struct Span { uintptr_t begin, end; int item; bool dst; };
// Does a destination among the spans overlap a source or another destination?  Sorted by address, one sweep; *d = the destination (named first: it is the one the
// caller placed wrongly), *o = what it overlaps.
inline bool spans_overlap(std::vector<Span>& sp, const Span** d, const Span** o) {
  std::sort(sp.begin(), sp.end(), [](const Span& a, const Span& b) { return a.begin < b.begin; });
  const Span* far_any = nullptr;   // of the spans that begin at or below the current one: the one that ends last, and the destination that ends last
  const Span* far_dst = nullptr;
  for (const Span& v : sp) {
    const Span* hit = v.dst ? far_any : far_dst;
    if (hit && hit->end > v.begin) { *d = v.dst ? &v : hit; *o = v.dst ? hit : &v; return true; }
    if (!far_any || v.end > far_any->end) far_any = &v;
    if (v.dst && (!far_dst || v.end > far_dst->end)) far_dst = &v;
  }
  return false;
}
}  // namespace bsx
