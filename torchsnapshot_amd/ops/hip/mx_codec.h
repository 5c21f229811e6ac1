// The block-scaled codec (docs/format.md): one description per stored format
// and the three pieces of bit arithmetic every format shares - a block's
// scale exponent, an element's code, a code's value.
//
// Plain C++17: no HIP, no pybind, so tests/native/mx_codec_selftest.cpp holds
// it to a floating-point reference on the host, under sanitizers. staging.hip
// compiles the same functions for the device; desc_check.h takes the block
// sizes from here.
//
// Everything is integer arithmetic on f32 bit patterns: f32 subnormals, code
// subnormals and ties come out the same on the host and in every wave mode.

#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define TSAMD_MX_FN __host__ __device__ inline
#else
#define TSAMD_MX_FN inline
#endif

namespace tsamd {

constexpr uint32_t kMxBlock = 32;  // elements per scale byte, every format

// A code is sign | exponent field | mantissa field, kBits wide, with value
// 2^(ef - kBias) * (1 + m / 2^kMantBits), or 2^(1 - kBias) * m / 2^kMantBits
// where ef == 0. The largest finite magnitude kMaxCode has the value
// (1 + kMaxMant / 2^23) * 2^kMaxExp.

// mxfp8_e4m3: e4m3fn codes, one per byte; 448 = 1.75 * 2^8; magnitude 0x7F
// is NaN, and there is no Inf
struct MxFp8E4M3 {
  static constexpr uint32_t kBits = 8;
  static constexpr uint32_t kMantBits = 3;
  static constexpr int kBias = 7;
  static constexpr uint32_t kMaxCode = 0x7E;
  static constexpr int kMaxExp = 8;
  static constexpr uint32_t kMaxMant = 0x00600000u;
  static constexpr bool kHasNan = true;
  static constexpr uint32_t kBlockBytes = kMxBlock * kBits / 8;
};

// mxfp4_e2m1: the grid 0, 0.5, 1, 1.5, 2, 3, 4, 6, two codes per byte with
// the even element in the low nibble; 6 = 1.5 * 2^2; neither NaN nor Inf, so
// magnitude 7 is 6 and a block with a non-finite element says so in its scale
// byte (X = 0xFF)
struct MxFp4E2M1 {
  static constexpr uint32_t kBits = 4;
  static constexpr uint32_t kMantBits = 1;
  static constexpr int kBias = 1;
  static constexpr uint32_t kMaxCode = 0x7;
  static constexpr int kMaxExp = 2;
  static constexpr uint32_t kMaxMant = 0x00400000u;
  static constexpr bool kHasNan = false;
  static constexpr uint32_t kBlockBytes = kMxBlock * kBits / 8;
};

// E of a block from the pattern of its amax (finite, sign cleared):
// floor(log2 amax) - kMaxExp, one more when amax * 2^-E would exceed the
// largest code's value, at least -127. Zero and f32 subnormals end at -127.
template <typename FMT>
TSAMD_MX_FN int mx_block_exp(uint32_t amax) {
  if (amax < 0x00800000u) return -127;
  const int e = (int)(amax >> 23) - (127 + FMT::kMaxExp) +
                ((amax & 0x007FFFFFu) > FMT::kMaxMant);
  return e < -127 ? -127 : e;
}

// Code of the f32 pattern u scaled by 2^-E, round to nearest even, clamped to
// +-kMaxCode's value; NaN and +-Inf become the all-ones magnitude with the
// sign kept (fp8's NaN code; in fp4 the block's scale byte carries the NaN).
template <typename FMT>
TSAMD_MX_FN uint32_t mx_encode(uint32_t u, int E) {
  constexpr uint32_t kMag = (1u << (FMT::kBits - 1)) - 1u;
  constexpr int kTMin = 1 - FMT::kBias;  // exponent of the smallest normal
  const uint32_t sign = (u >> (32 - FMT::kBits)) & (kMag + 1u);
  const uint32_t a = u & 0x7FFFFFFFu;
  if (a >= 0x7F800000u) return sign | kMag;
  if (a == 0u) return sign;
  // |x| = M * 2^(ex - 23) with M in [2^23, 2^24)
  uint32_t M = a & 0x007FFFFFu;
  int ex = (int)(a >> 23) - 127;
  if (a < 0x00800000u) {
    const int lz = __builtin_clz(M) - 8;  // 1..23
    M <<= lz;
    ex = -126 - lz;
  } else {
    M |= 0x00800000u;
  }
  // y = |x| * 2^-E has exponent t. From kTMin up it is a normal with step
  // 2^(t - kMantBits): q = RNE(M / 2^(23 - kMantBits)) in [2^kMantBits,
  // 2^(kMantBits + 1)], and a carry to the top runs into the exponent field.
  // Below, the step stays 2^(kTMin - kMantBits) (the code's subnormals).
  const int t = ex - E;
  const int shift = 23 - (int)FMT::kMantBits + (t < kTMin ? kTMin - t : 0);
  const uint32_t sh = shift > 26 ? 26u : (uint32_t)shift;  // >= 25 gives 0
  const uint32_t q = (M + ((1u << (sh - 1)) - 1u) + ((M >> sh) & 1u)) >> sh;
  const uint32_t code =
      t >= kTMin ? ((uint32_t)(t - kTMin) << FMT::kMantBits) + q : q;
  return sign | (code > FMT::kMaxCode ? FMT::kMaxCode : code);
}

// f32 pattern of value(code) * 2^(X - 127): exact, f32 subnormals included.
// X = 0xFF decodes to NaN, and so does a format's own NaN code.
template <typename FMT>
TSAMD_MX_FN uint32_t mx_decode(uint32_t c, uint32_t X) {
  constexpr uint32_t kMag = (1u << (FMT::kBits - 1)) - 1u;
  const uint32_t sign = (c & (kMag + 1u)) << (32 - FMT::kBits);
  const uint32_t a = c & kMag;
  if ((FMT::kHasNan && a == kMag) || X == 0xFFu) return sign | 0x7FC00000u;
  if (a == 0u) return sign;
  const uint32_t ef = a >> FMT::kMantBits, m = a & ((1u << FMT::kMantBits) - 1u);
  int ex;
  uint32_t frac;
  if (ef != 0u) {
    ex = (int)ef - FMT::kBias;
    frac = m << (23 - FMT::kMantBits);
  } else {
    const int p = 31 - __builtin_clz(m);  // the leading one of a subnormal
    ex = p + 1 - FMT::kBias - (int)FMT::kMantBits;
    frac = (m << (23 - p)) & 0x007FFFFFu;
  }
  const int biased = ex + (int)X;  // ex + (X - 127) + 127
  if (biased >= 255) return sign | 0x7F800000u;
  if (biased > 0) return sign | ((uint32_t)biased << 23) | frac;
  // only the top kMantBits + 1 bits of the significand are set and the shift
  // is at most kBias + kMantBits: nothing is lost
  return sign | ((0x00800000u | frac) >> (1 - biased));
}

}  // namespace tsamd
