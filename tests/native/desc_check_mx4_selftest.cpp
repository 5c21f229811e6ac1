// Stand-alone check of the block-scaled fp4 (mx4) rules of check_descs in
// ops/hip/desc_check.h, built with host sanitizers and run directly
// (tests/test_desc_check_mx4.py). No HIP. Exit status 0 = all passed.

#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "desc_check.h"

using namespace tsamd;

namespace {

int g_failures = 0;

using Row = std::vector<unsigned long long>;

// 40 rows of 64 elements at a 512 B pitch, aligned class, slab offset 256:
// 80 blocks, 16 code bytes each
Row good_row(unsigned long long code) {
  Row r(kRowInts, 0);
  r[0] = 0x7f0000001000ull;
  r[1] = 256;
  r[2] = 80 * 16;
  r[3] = 64;
  r[4] = 8;
  r[5] = 1;
  for (int k = 0; k < kMaxDims; ++k) r[6 + k] = 1;
  r[6] = 40;
  r[12] = 512;
  r[18] = code;
  return r;
}

const FlatSide kFlat{0, 0x7e0000000000ull, 256 + 17 * 80, 0};

// r with r[field] = value: refused with `needle`, accepted when it is empty
void expect(Row r, int field, unsigned long long value, DescKind kind,
            const FlatSide* flat, const char* needle, int line) {
  std::string got;
  if (field >= 0) r[field] = value;
  try {
    check_descs(parse_descs(r, 1), kind, flat);
  } catch (const std::runtime_error& e) {
    got = e.what();
  }
  if (needle[0] ? got.find(needle) != std::string::npos : got.empty()) return;
  std::fprintf(stderr, "FAIL line %d: got \"%s\", wanted \"%s\"\n", line,
               got.c_str(), needle);
  ++g_failures;
}
#define EXPECT(r, field, value, kind, flat, needle) \
  expect(r, field, value, kind, flat, needle, __LINE__)

}  // namespace

int main() {
  EXPECT(good_row(kCastMX4toBF16 + 1), -1, 0, DescKind::Gather, &kFlat,
         "unknown cast code");
  for (unsigned long long code = kCastF32toMX4; code <= kCastMX4toBF16; ++code) {
    const bool narrowing = code <= kCastBF16toMX4;
    const DescKind mine = narrowing ? DescKind::Gather : DescKind::Unpack;
    const DescKind other = narrowing ? DescKind::Unpack : DescKind::Gather;
    const Row good = good_row(code);
    EXPECT(good, -1, 0, mine, &kFlat, "");
    EXPECT(good, -1, 0, other, &kFlat, narrowing ? "narrowing cast" : "scatter-only");
    EXPECT(good, -1, 0, DescKind::Fingerprint, &kFlat, "scatter-only");
    EXPECT(good, -1, 0, DescKind::Scatter, &kFlat, "cast");
    EXPECT(good, 2, 80 * 16 + 8, mine, &kFlat, "mx4: nbytes must be whole blocks");
    EXPECT(good, 2, 80 * 16 + 16, mine, &kFlat, "mx4: nbytes is not the block-padded");
    EXPECT(good, 4, 16, mine, &kFlat, "mx4: vec must be 8 (aligned) or 1 (general)");
    EXPECT(good, 1, 264, mine, &kFlat, "mx4: flat offset must be 16-aligned");
    FlatSide flat = kFlat;
    flat.total_bytes = 256 + 33 * 80;
    // fp8's count for the same elements is not fp4's
    EXPECT(good, 2, 80 * 32, mine, &flat, "mx4: nbytes is not the block-padded");
    flat = kFlat;
    flat.pinned_ptr += 8;
    EXPECT(good, -1, 0, mine, &flat, "mx4: flat side must be 16-aligned");
    flat = kFlat;
    flat.total_bytes -= 1;  // the last scale byte falls outside
    EXPECT(good, -1, 0, mine, &flat, "mx4: scales region outside the slab");

    // aligned: 16 B aligned tensor side, rows of 32k; general: any layout
    EXPECT(good, 0, good[0] + 8, mine, &kFlat, "mx4: tensor side not aligned");
    Row r = good;
    r[3] = 80;
    r[6] = 32;
    EXPECT(r, -1, 0, mine, &kFlat, "mx4: aligned class needs rows of 32k");
    r[4] = 1;
    EXPECT(r, 0, r[0] + 8, mine, &kFlat, "");
    EXPECT(r, 0, r[0] + 1, mine, &kFlat, "mx4: tensor side not aligned");

    // contiguous, 37 elements: the second block is short
    r = good;
    r[5] = 0;
    r[6] = 1;
    r[3] = 37;
    EXPECT(r, 2, 32, mine, &kFlat, "");

    // the size cap is on elements: 2^32 - 64 Ki of them pass, one block
    // more does not (fp8 takes that many code bytes)
    flat = kFlat;
    flat.total_bytes = 1ull << 32;
    r[3] = kMaxDescBytes;
    EXPECT(r, 2, kMaxDescBytes / 2, mine, &flat, "");
    r[3] = kMaxDescBytes + 32;
    EXPECT(r, 2, kMaxDescBytes / 2 + 16, mine, &flat, "mx4: too many elements");
  }
  if (g_failures == 0) std::printf("desc_check mx4 selftest OK\n");
  return g_failures == 0 ? 0 : 1;
}
