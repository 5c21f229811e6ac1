// DescKind::Compare of ops/hip/desc_check.h, stand-alone and without HIP:
// built with host sanitizers and run by tests/test_compare_cpu.py. Exit 0 = ok.

#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "desc_check.h"

using namespace tsamd;
using Row = std::vector<unsigned long long>;

static int g_failures = 0;
static const FlatSide kFlat{0, 0x7e0000000000ull, 256 + 64 * 128, 0};

// 64 rows of 128 stored bytes at a 512 B pitch, vec 16, 256 B into a payload
static Row good_row(uint32_t cls) {
  Row r(kRowInts, 0);
  r[0] = 0x7f0000001000ull;
  r[1] = 256, r[2] = 64 * 128, r[3] = 128, r[4] = 16, r[5] = 1;
  for (int k = 0; k < kMaxDims; ++k) r[6 + k] = 1;
  r[6] = 64;
  r[12] = 512;
  r[18] = cls < kCmpClasses ? cmp_cast_code(cls) : 0;
  return r;
}

// the refusal's message must hold `needle`; "" = accepted
static void expect(const Row& row, uint32_t cls, const FlatSide* flat,
                   const char* needle, int line) {
  std::string got;
  try {
    const std::vector<uint32_t> classes(1, cls);
    check_descs(parse_descs(row, 1), DescKind::Compare, flat, &classes);
  } catch (const std::runtime_error& e) {
    got = e.what();
  }
  if (needle[0] ? got.find(needle) == std::string::npos : !got.empty()) {
    std::fprintf(stderr, "FAIL line %d: got \"%s\", wanted \"%s\"\n", line,
                 got.c_str(), needle);
    ++g_failures;
  }
}
#define EXPECT(row, cls, flat, needle) expect(row, cls, flat, needle, __LINE__)

int main() {
  for (uint32_t cls = 0; cls < kCmpClasses; ++cls) {
    EXPECT(good_row(cls), cls, &kFlat, "");
  }
  EXPECT(good_row(kCmpClasses), kCmpClasses, &kFlat,
         "compare_tensors: unknown element class");
  EXPECT(good_row(kScanF32), kScanF32, nullptr, "no flat side given");
  const char* mismatch = "cast code does not go with the element class";
  EXPECT(good_row(kCmpBF16toF32), kScanF32, &kFlat, mismatch);
  EXPECT(good_row(kScanF32), kCmpBF16toF32, &kFlat, mismatch);
  Row r = good_row(kCmpRaw1);
  r[1] = 257;
  EXPECT(r, kCmpRaw1, &kFlat, "descriptor outside the payload");
  r = good_row(kScanF32);
  r[1] = 8, r[2] = 128, r[6] = 1;
  EXPECT(r, kScanF32, &kFlat, "flat address not aligned for its vec");
  r[4] = 8;
  EXPECT(r, kScanF32, &kFlat, "");
  EXPECT(r, kCmpRaw16, &kFlat, "vec below the element size");
  r = good_row(kScanBF16);
  r[0] += 8;
  EXPECT(r, kScanBF16, &kFlat, "tensor not aligned for its vec");
  r = good_row(kScanF32);
  r[6] = 63;  // loads only inside the rows named
  EXPECT(r, kScanF32, &kFlat, "sizes do not cover nbytes");
  r = good_row(kCmpBF16toF32);
  r[12] = 0;  // an expanded dim overlaps itself: fine, nothing is written
  EXPECT(r, kCmpBF16toF32, &kFlat, "");
  if (g_failures == 0) std::printf("desc_check compare selftest OK\n");
  return g_failures == 0 ? 0 : 1;
}
