// Stand-alone check of DescKind::Stats in ops/hip/desc_check.h, built with
// host sanitizers and run directly (tests/test_desc_check_stats.py). No HIP:
// tensor_stats' rules are applied on the host. Exit status 0 = all passed.

#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "desc_check.h"

using namespace tsamd;

namespace {

int g_failures = 0;

using Row = std::vector<unsigned long long>;

// 64 rows of 128 B at a 256 B pitch, vec 16
Row good_row() {
  Row r(kRowInts, 0);
  r[0] = 0x7f0000001000ull;
  r[2] = 64 * 128;
  r[3] = 128;
  r[4] = 16;
  r[5] = 1;
  for (int k = 0; k < kMaxDims; ++k) r[6 + k] = 1;
  r[6] = 64;
  r[12] = 256;
  return r;
}

// "" when accepted, else the refusal's message
std::string verdict(const Row& row, uint32_t cls, size_t n_classes = 1) {
  try {
    const std::vector<uint32_t> classes(n_classes, cls);
    check_descs(parse_descs(row, 1), DescKind::Stats, nullptr, &classes);
  } catch (const std::runtime_error& e) {
    return e.what();
  }
  return "";
}

void expect(const Row& row, uint32_t cls, size_t n_classes, const char* needle,
            int line) {
  const std::string got = verdict(row, cls, n_classes);
  const bool ok = needle[0] ? got.find(needle) != std::string::npos : got.empty();
  if (!ok) {
    std::fprintf(stderr, "FAIL line %d: got \"%s\", wanted \"%s\"\n", line,
                 got.c_str(), needle);
    ++g_failures;
  }
}
#define EXPECT(row, cls, n, needle) expect(row, cls, n, needle, __LINE__)

}  // namespace

int main() {
  for (uint32_t cls = 0; cls < kStatsClasses; ++cls) {
    EXPECT(good_row(), cls, 1, "");
  }
  // the classes that do not widen to f64 exactly, and anything past them
  EXPECT(good_row(), kScanE5M2, 1, "tensor_stats: unknown element class");
  EXPECT(good_row(), 0xFFFFFFFFu, 1, "unknown element class");
  EXPECT(good_row(), kScanF32, 0, "one class code per descriptor");
  for (unsigned long long code = kCastBF16; code <= kCastF16toF32; ++code) {
    Row r = good_row();
    r[18] = code;
    EXPECT(r, kScanF32, 1, "cast descriptors not allowed");
  }
  Row r = good_row();
  r[4] = 4;  // vec below an f64 element, at an f32 one
  EXPECT(r, kScanF64, 1, "vec below the element size");
  EXPECT(r, kScanF32, 1, "");
  r = good_row();
  r[0] += 8;  // base not aligned for vec 16
  EXPECT(r, kScanBF16, 1, "tensor not aligned for its vec");
  r = good_row();
  r[6] = 63;
  EXPECT(r, kScanF32, 1, "sizes do not cover nbytes");
  r = good_row();
  r[2] = (1ull << 32) - 128;  // past the size cap
  r[6] = (uint32_t)(r[2] / 128);
  EXPECT(r, kScanF32, 1, "tensor too large");
  if (g_failures == 0) std::printf("desc_check stats selftest OK\n");
  return g_failures == 0 ? 0 : 1;
}
