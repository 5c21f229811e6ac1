// Stand-alone check of ops/hip/desc_check.h, meant to be compiled with
// -fsanitize=address,undefined and run directly (see
// tests/test_desc_check.py). No HIP: this is the proof that every
// descriptor rule is applied on the host, before any GPU call.
// Exit status 0 = every case passed.

#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "desc_check.h"

using namespace tsamd;

namespace {

int g_failures = 0;

#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failures;                                                      \
    }                                                                    \
  } while (0)

using Row = std::vector<unsigned long long>;

constexpr unsigned long long kBase = 0x7f0000001000ull;  // 4 KiB aligned
constexpr unsigned long long kCap = (1ull << 32) - (1ull << 16);

// 64 rows of 128 B at a 256 B pitch, vec 16: valid for every kind
Row good_row() {
  Row r(kRowInts, 0);
  r[0] = kBase;
  r[1] = 256;       // flat_off
  r[2] = 64 * 128;  // nbytes
  r[3] = 128;       // row_bytes
  r[4] = 16;        // vec
  r[5] = 1;         // ndim
  for (int k = 0; k < kMaxDims; ++k) r[6 + k] = 1;
  r[6] = 64;
  r[12] = 256;
  return r;
}

const FlatSide kFlat{/*slab_ptr=*/0, /*pinned_ptr=*/0x7e0000000000ull,
                     /*total_bytes=*/1 << 20, /*hash_byte0=*/0};

// "" when accepted, else the refusal's message
std::string verdict(const Row& row, DescKind kind,
                    const FlatSide* flat = &kFlat, uint32_t cls = kScanF32,
                    size_t n_classes = 1) {
  try {
    const std::vector<Desc> descs = parse_descs(row, 1);
    const std::vector<uint32_t> classes(n_classes, cls);
    check_descs(descs, kind, flat, &classes);
  } catch (const std::runtime_error& e) {
    return e.what()[0] ? e.what() : "(empty message)";
  }
  return "";
}

bool refused(const std::string& got, const char* needle) {
  if (got.find(needle) == std::string::npos) {
    std::fprintf(stderr, "  got \"%s\", wanted \"%s\"\n", got.c_str(), needle);
    return false;
  }
  return true;
}

const DescKind kAllKinds[] = {DescKind::Gather, DescKind::Scatter,
                              DescKind::Unpack, DescKind::Scan};

void shared_rules() {
  for (DescKind kind : kAllKinds) {
    CHECK(verdict(good_row(), kind) == "");
    Row r = good_row();
    r[2] = 0;  // an empty descriptor is skipped whatever else it says
    r[4] = 3;
    CHECK(verdict(r, kind) == "");

    // the size cap: exactly 2^32 - 64 KiB passes, 16 B more does not
    r = good_row();
    r[5] = 0;
    r[2] = r[3] = kCap;
    FlatSide big = kFlat;
    big.total_bytes = 1ull << 33;
    CHECK(verdict(r, kind, &big) == "");
    r[2] = r[3] = kCap + 16;
    CHECK(refused(verdict(r, kind, &big), "too large"));
    r[2] = r[3] = 1ull << 32;  // does not fit the struct at all
    CHECK(refused(verdict(r, kind, &big), ">=4GB"));

    for (unsigned long long vec : {0ull, 3ull, 32ull}) {
      r = good_row();
      r[4] = vec;
      CHECK(refused(verdict(r, kind), "vec must be 16/8/4/2/1"));
    }
    r = good_row();
    r[3] = 120;  // vec 16 does not divide the row
    r[2] = 64 * 120;
    CHECK(refused(verdict(r, kind), "row_bytes/vec mismatch"));
    r = good_row();
    r[2] += 16;  // rows do not divide nbytes
    CHECK(refused(verdict(r, kind), "row_bytes/vec mismatch"));
    r = good_row();
    r[3] = 0;
    CHECK(refused(verdict(r, kind), "row_bytes/vec mismatch"));
    r = good_row();
    r[0] += 8;  // base misaligned for vec 16
    CHECK(refused(verdict(r, kind), "not aligned for its vec"));
    r[4] = 8;  // ... and fine for vec 8
    CHECK(verdict(r, kind) == "");
    r = good_row();
    r[12] = 264;  // stride misaligned for vec 16
    CHECK(refused(verdict(r, kind), "not aligned for its vec"));

    r = good_row();
    r[5] = 7;
    CHECK(refused(verdict(r, kind), "too many outer dims"));
    r = good_row();
    r[18] = 5;
    CHECK(refused(verdict(r, kind), "unknown cast code"));
  }
  Row two = good_row();
  two.push_back(0);
  CHECK(refused(verdict(two, DescKind::Gather), "descriptor array length"));
}

void cast_codes() {
  for (unsigned long long code = 1; code <= 4; ++code) {
    Row r = good_row();
    r[18] = code;
    const bool narrowing = code <= 2;
    if (narrowing) {
      CHECK(verdict(r, DescKind::Gather) == "");
      CHECK(refused(verdict(r, DescKind::Unpack), "narrowing"));
    } else {
      CHECK(refused(verdict(r, DescKind::Gather), "scatter-only"));
      CHECK(verdict(r, DescKind::Unpack) == "");
    }
    CHECK(refused(verdict(r, DescKind::Scatter), "cast"));
    CHECK(refused(verdict(r, DescKind::Scan), "cast"));
    // refused even on an empty descriptor
    r[2] = 0;
    CHECK(refused(verdict(r, DescKind::Scatter), "cast"));

    // the tensor side moves 2*vec bytes per lane
    const DescKind kind = narrowing ? DescKind::Gather : DescKind::Unpack;
    r = good_row();
    r[18] = code;
    r[4] = 1;
    CHECK(refused(verdict(r, kind), "vec must be 16/8/4/2"));
    r[4] = 4;
    r[0] = kBase + 4;  // 4-aligned: enough for a copy at vec 4, not a cast
    CHECK(refused(verdict(r, kind), "not aligned for its vec"));
    r[0] = kBase + 8;
    CHECK(verdict(r, kind) == "");
    r[4] = 8;
    CHECK(refused(verdict(r, kind), "not aligned for its vec"));
    r[4] = 16;  // two 16 B accesses: 16-alignment is what it takes
    r[0] = kBase + 16;
    CHECK(verdict(r, kind) == "");
    r[12] = 264;
    CHECK(refused(verdict(r, kind), "not aligned for its vec"));
  }
}

void unpack_extras() {
  const DescKind kind = DescKind::Unpack;
  FlatSide f = kFlat;
  f.hash_byte0 = 4;
  CHECK(refused(verdict(good_row(), kind, &f), "hash_byte0"));
  f = kFlat;
  f.slab_ptr = 0x7d0000000008ull;
  CHECK(refused(verdict(good_row(), kind, &f), "slab must be 16-aligned"));
  f = kFlat;
  f.total_bytes = 256 + 64 * 128 - 1;
  CHECK(refused(verdict(good_row(), kind, &f), "outside the payload"));
  f.total_bytes += 1;
  CHECK(verdict(good_row(), kind, &f) == "");
  f.total_bytes = 100;  // flat_off itself past the end
  CHECK(refused(verdict(good_row(), kind, &f), "outside the payload"));
  f = kFlat;
  f.pinned_ptr += 8;
  CHECK(refused(verdict(good_row(), kind, &f), "flat address"));
  Row r = good_row();
  r[1] = 264;
  CHECK(refused(verdict(r, kind), "flat address"));
  CHECK(refused(verdict(good_row(), kind, nullptr), "flat side"));
  // none of these is a gather rule
  f = kFlat;
  f.hash_byte0 = 4;
  f.total_bytes = 0;
  CHECK(verdict(good_row(), DescKind::Gather, &f) == "");
}

void scan_extras() {
  const DescKind kind = DescKind::Scan;
  CHECK(refused(verdict(good_row(), kind, nullptr, kScanClasses),
                "unknown element class"));
  CHECK(refused(verdict(good_row(), kind, nullptr, kScanF32, 0),
                "one class code per descriptor"));
  CHECK(refused(verdict(good_row(), kind, nullptr, kScanF32, 2),
                "one class code per descriptor"));
  Row r = good_row();
  r[4] = 4;
  CHECK(verdict(r, kind, nullptr, kScanF32) == "");
  CHECK(refused(verdict(r, kind, nullptr, kScanF64),
                "below the element size"));
  r[4] = 1;
  CHECK(verdict(r, kind, nullptr, kScanE5M2) == "");
  CHECK(refused(verdict(r, kind, nullptr, kScanBF16),
                "below the element size"));
  r = good_row();
  r[12] = (unsigned long long)-256ll;  // negative stride
  CHECK(refused(verdict(r, kind), "not aligned for its vec"));
  CHECK(verdict(r, DescKind::Gather) == "");  // the copies allow it
  r = good_row();
  r[6] = 63;
  CHECK(refused(verdict(r, kind), "sizes do not cover nbytes"));
  r = good_row();
  r[5] = 2;
  r[7] = 0;  // a zero size
  CHECK(refused(verdict(r, kind), "not aligned for its vec"));
  r = good_row();
  r[12] = 0;  // an expanded dim is fine
  CHECK(verdict(r, kind) == "");
}

void launch_prologue() {
  Row rows;
  for (unsigned long long nbytes : {0ull, 1ull, 65536ull, 65537ull, kCap}) {
    Row r = good_row();
    r[5] = 0;
    r[2] = r[3] = nbytes;
    r[4] = 1;
    rows.insert(rows.end(), r.begin(), r.end());
  }
  const std::vector<Desc> descs = parse_descs(rows, 5);
  const std::vector<unsigned long long> prefix = wu_prefix_of(descs);
  const std::vector<unsigned long long> want = {0, 0, 1, 2, 4, 4 + 65535};
  CHECK(prefix == want);

  CHECK(grid_for(0, 256, nullptr) == 1);
  CHECK(grid_for(100, 256, nullptr) == 100);
  CHECK(grid_for(1000, 256, nullptr) == 256);
  CHECK(grid_for(1000, 256, "64") == 64);
  CHECK(grid_for(1000, 256, "4096") == 1000);
  CHECK(grid_for(1000, 256, "0") == 256);
  CHECK(grid_for(1000, 256, "-3") == 256);
  CHECK(grid_for(1000, 256, "junk") == 256);

  const std::vector<uint32_t> classes = {1, 2, 3, 4, 5};
  const LaunchTables t(descs, prefix, classes.data(), 5 * sizeof(uint32_t));
  CHECK(t.prefix_off == 5 * sizeof(Desc));
  CHECK(t.extra_off == t.prefix_off + 6 * 8);
  CHECK(t.host.size() == (t.extra_off + 20 + 7) / 8 * 8);
  CHECK(t.host.size() % 8 == 0);
  const char* dev = t.host.data();  // the image, read where it was built
  CHECK(std::memcmp(t.descs(dev), descs.data(), t.prefix_off) == 0);
  CHECK(std::memcmp(t.prefix(dev), prefix.data(), 6 * 8) == 0);
  CHECK(std::memcmp(t.extra(dev), classes.data(), 20) == 0);
  const LaunchTables none({}, {0});
  CHECK(none.host.size() == 8 && none.prefix_off == 0);
}

}  // namespace

int main() {
  shared_rules();
  cast_codes();
  unpack_extras();
  scan_extras();
  launch_prologue();
  if (g_failures) {
    std::fprintf(stderr, "%d check(s) failed\n", g_failures);
    return 1;
  }
  std::printf("desc_check selftest OK\n");
  return 0;
}
