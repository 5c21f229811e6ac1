// Stand-alone check of the block-scaled codec in ops/hip/mx_codec.h against
// a reference written here in double with frexp / ldexp / nearbyint, after
// docs/format.md; built with host sanitizers and run directly
// (tests/test_mx_codec.py). No HIP. Exit status 0 = all passed.

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "mx_codec.h"

using namespace tsamd;

namespace {

int g_failures = 0;

void fail(const char* what, const char* fmt, uint32_t a, int b, uint32_t got,
          uint32_t want) {
  if (++g_failures <= 20) {
    std::fprintf(stderr, "FAIL %s %s: (0x%08x, %d) gave 0x%08x, wanted 0x%08x\n",
                 fmt, what, a, b, got, want);
  }
}

float as_float(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

uint32_t as_bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

// A format as docs/format.md gives it, in words of its own: the widths, the
// largest value, and whether the all-ones magnitude is NaN
struct RefFormat {
  const char* name;
  int bits, mant, bias;
  double max_value;
  bool has_nan;
};
const RefFormat kRefFp8{"mxfp8_e4m3", 8, 3, 7, 448.0, true};
const RefFormat kRefFp4{"mxfp4_e2m1", 4, 1, 1, 6.0, false};

int floor_log2(double y) {  // y > 0
  int e;
  std::frexp(y, &e);
  return e - 1;
}

// E of a block whose largest finite magnitude is amax
int ref_block_exp(const RefFormat& f, double amax) {
  if (amax == 0.0) return -127;
  int E = floor_log2(amax) - floor_log2(f.max_value);
  if (std::ldexp(amax, -E) > f.max_value) ++E;
  return E < -127 ? -127 : E;
}

// the code of the magnitude q, a value of the format's grid
uint32_t ref_code_of(const RefFormat& f, double q) {
  if (q == 0.0) return 0;
  const int e = floor_log2(q);
  if (e < 1 - f.bias) {  // subnormal: a multiple of 2^(1 - bias - mant)
    return (uint32_t)std::ldexp(q, f.bias - 1 + f.mant);
  }
  const double frac = std::ldexp(q, -e) - 1.0;  // [0, 1)
  return ((uint32_t)(e + f.bias) << f.mant) | (uint32_t)std::ldexp(frac, f.mant);
}

uint32_t ref_encode(const RefFormat& f, uint32_t u, int E) {
  const uint32_t sign = (u >> 31) << (f.bits - 1);
  const uint32_t all_ones = (1u << (f.bits - 1)) - 1u;
  const double x = std::fabs((double)as_float(u));
  if (!std::isfinite(x)) return sign | all_ones;
  double y = std::ldexp(x, -E);
  if (y > f.max_value) y = f.max_value;
  if (y == 0.0) return sign;
  // the grid's step at y: 2^(floor(log2 y) - mant), and the smallest normal's
  // below it; nearbyint rounds ties to even
  int e = floor_log2(y);
  if (e < 1 - f.bias) e = 1 - f.bias;
  const double q = std::ldexp(std::nearbyint(std::ldexp(y, f.mant - e)), e - f.mant);
  return sign | ref_code_of(f, q);
}

uint32_t ref_decode(const RefFormat& f, uint32_t c, uint32_t X) {
  const uint32_t sign = ((c >> (f.bits - 1)) & 1u) << 31;
  const uint32_t a = c & ((1u << (f.bits - 1)) - 1u);
  if (X == 0xFFu || (f.has_nan && a == (1u << (f.bits - 1)) - 1u)) {
    return sign | 0x7FC00000u;
  }
  const uint32_t ef = a >> f.mant, m = a & ((1u << f.mant) - 1u);
  const double frac = std::ldexp((double)m, -f.mant);
  const double v = ef != 0 ? std::ldexp(1.0 + frac, (int)ef - f.bias)
                           : std::ldexp(frac, 1 - f.bias);
  const double r = std::ldexp(v, (int)X - 127);
  if (r >= std::ldexp(1.0, 128)) return sign | 0x7F800000u;
  const float out = (float)r;  // at most four significant bits: exact
  if ((double)out != r) return 0xDEADBEEFu;
  return sign | as_bits(out);
}

template <typename FMT>
void check(const RefFormat& f) {
  static const uint32_t kLow[] = {0u, 1u, 0x7FFFu, 0x8000u, 0x8001u, 0xFFFFu};
  for (uint32_t hi = 0; hi < 0x10000u; ++hi) {
    for (uint32_t lo : kLow) {
      const uint32_t u = (hi << 16) | lo;
      const uint32_t a = u & 0x7FFFFFFFu;
      int natural = 0;
      if (a < 0x7F800000u) {
        natural = ref_block_exp(f, (double)as_float(a));
        const int got = mx_block_exp<FMT>(a);
        if (got != natural) {
          fail("block_exp", f.name, a, 0, (uint32_t)got, (uint32_t)natural);
        }
      }
      for (int d = -2; d <= 40; ++d) {
        int E = natural + d;
        E = E < -127 ? -127 : E > 127 ? 127 : E;
        const uint32_t got = mx_encode<FMT>(u, E), want = ref_encode(f, u, E);
        if (got != want) fail("encode", f.name, u, E, got, want);
      }
    }
  }
  const uint32_t all_ones = (1u << (FMT::kBits - 1)) - 1u;
  for (uint32_t c = 0; c < (1u << FMT::kBits); ++c) {
    for (uint32_t X = 0; X < 256; ++X) {
      const uint32_t got = mx_decode<FMT>(c, X), want = ref_decode(f, c, X);
      if (got != want) fail("decode", f.name, c, (int)X, got, want);
      // round trip, where the decoded value is a finite normal f32
      const uint32_t ex = (got >> 23) & 0xFFu;
      if ((FMT::kHasNan && (c & all_ones) == all_ones) || ex == 0 || ex == 255) {
        continue;
      }
      const uint32_t back = mx_encode<FMT>(got, (int)X - 127);
      if (back != c) fail("round trip", f.name, got, (int)X - 127, back, c);
    }
  }
}

}  // namespace

int main() {
  // the structs say what docs/format.md says
  static_assert(MxFp8E4M3::kBlockBytes == 32 && MxFp4E2M1::kBlockBytes == 16 &&
                    kMxBlock == 32,
                "33 and 17 bytes per 32 elements");
  check<MxFp8E4M3>(kRefFp8);
  check<MxFp4E2M1>(kRefFp4);
  if (g_failures == 0) std::printf("mx_codec selftest OK\n");
  return g_failures == 0 ? 0 : 1;
}
