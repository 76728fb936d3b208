// Stand-alone check of overlapnet_amd/csrc/ovn_scratch.h (tests/test_scratch_carver.py builds it with AddressSanitizer and UBSan and
// runs it): a sample layout with optional and zero-count regions, measured and then placed in a heap block of exactly bytes() bytes.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "ovn_scratch.h"

struct Region {
  char* p;
  size_t bytes;
};

struct Sample {   // what a consumer's layout looks like: typed pointers, the regions listed once, in the constructor
  float* a;
  double* b;
  char* none;       // zero-count region
  int32_t* opt;     // optional region: NULL when the call does not need it
  uint16_t* tail;
  std::vector<Region> regions;   // (the check's own record of what was taken)
  template <class T>
  T* rec(OvnCarver& c, size_t n) {
    T* p = c.take<T>(n);
    regions.push_back({reinterpret_cast<char*>(p), n * sizeof(T)});
    return p;
  }
  Sample(OvnCarver& c, size_t n, bool with_opt) {
    a = rec<float>(c, n);              // n = 3: 12 bytes -> one 256-byte slot
    b = rec<double>(c, 32 * n + 1);    // 776 bytes -> rounded up
    none = rec<char>(c, 0);
    opt = with_opt ? rec<int32_t>(c, 64 * n) : nullptr;   // 768 bytes: an exact multiple stays as it is
    tail = rec<uint16_t>(c, 1);
  }
};

#define CHECK(cond)                                             \
  do {                                                          \
    if (!(cond)) {                                              \
      fprintf(stderr, "line %d: %s\n", __LINE__, #cond);        \
      return 1;                                                 \
    }                                                           \
  } while (0)

static int check(size_t n, bool with_opt, size_t want_bytes) {
  OvnCarver m(nullptr);
  const Sample meas(m, n, with_opt);
  CHECK(m.bytes() == want_bytes);
  CHECK((ovn_scratch_bytes<Sample>(n, with_opt)) == want_bytes);
  for (const Region& r : meas.regions) CHECK(r.p == nullptr);           // a measuring pass hands out no pointer
  char* block = static_cast<char*>(aligned_alloc(OvnCarver::ALIGN, want_bytes));   // exactly bytes(): one byte past it is ASan's
  CHECK(block != nullptr);
  OvnCarver c(block);
  const Sample s(c, n, with_opt);
  CHECK(c.bytes() == m.bytes());                                        // same total ...
  CHECK(s.regions.size() == meas.regions.size());
  // ... and the offsets of the placing pass are the running totals of the measuring pass
  OvnCarver again(nullptr);
  size_t expect = 0;
  for (size_t i = 0; i < s.regions.size(); ++i) {
    const Region& r = s.regions[i];
    CHECK((size_t)(r.p - block) == expect);
    CHECK((reinterpret_cast<uintptr_t>(r.p) & (OvnCarver::ALIGN - 1)) == 0);
    (void)again.take<char>(r.bytes);
    expect = again.bytes();
    CHECK(expect % OvnCarver::ALIGN == 0);
    if (r.bytes) {                                                      // first and last byte of every region
      r.p[0] = (char)(i + 1);
      r.p[r.bytes - 1] = (char)(i + 101);
    } else if (i + 1 < s.regions.size()) {
      CHECK(s.regions[i + 1].p == r.p);                                 // take(0) takes nothing
    }
  }
  CHECK(expect == want_bytes);
  for (size_t i = 0; i < s.regions.size(); ++i) {                       // no region's write landed in another
    const Region& r = s.regions[i];
    if (!r.bytes) continue;
    CHECK(r.p[r.bytes - 1] == (char)(i + 101));
    if (r.bytes > 1) CHECK(r.p[0] == (char)(i + 1));
  }
  CHECK((with_opt ? s.opt != nullptr : s.opt == nullptr));
  free(block);
  return 0;
}

int main() {
  if (check(3, true, 256 + 1024 + 0 + 768 + 256)) return 1;
  if (check(3, false, 256 + 1024 + 0 + 256)) return 1;
  if (check(0, true, 0 + 256 + 0 + 0 + 256)) return 1;    // every count that can be zero is
  puts("ovn_scratch ok");
  return 0;
}
