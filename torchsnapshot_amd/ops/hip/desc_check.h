// Descriptor ABI of the staging kernels, its one host-side validator, and
// the host half of the launch prologue.
//
// Plain C++17: no HIP, no pybind, so it builds stand-alone (the host
// sanitizer test compiles tests/native/desc_check_selftest.cpp with an
// ordinary C++ compiler) and staging.hip includes it for both the kernels
// (Desc, the codes) and the entry points (parse_descs, check_descs,
// wu_prefix_of, grid_for, LaunchTables).
//
// Every entry point of the extension that takes descriptor rows -
// pack_d2h, scatter_h2d, unpack_h2d, scan_nonfinite - runs check_descs
// before it touches the GPU: a row that would make a kernel issue a
// misaligned vector access, index past its rows, or wrap a u32 index is a
// std::runtime_error here, not a device fault there.

#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace tsamd {

constexpr int kMaxDims = 6;
constexpr uint32_t kWorkUnitBytes = 64 * 1024;

// Largest flat-side size of one descriptor. The kernels index within a
// tensor in u32 and step up to 4 KiB (256 lanes x 16 B) past the end of a
// work unit before the loop test fails, so the last work unit must end at
// least that far below 2^32; one whole work unit of headroom keeps the
// rule simple. ops/staging.py's _KERNEL_MAX_BYTES is this value.
constexpr uint32_t kMaxDescBytes = 0xFFFFFFFFu - kWorkUnitBytes + 1u;

struct Desc {
  const char* tensor_base;
  unsigned long long flat_off;   // byte offset of this tensor in the slab
  uint32_t nbytes;               // payload bytes (<= kMaxDescBytes)
  uint32_t row_bytes;            // innermost contiguous run
  uint32_t vec;                  // safe vector width (16/8/4/2/1)
  uint32_t ndim;                 // number of outer (strided) dims
  uint32_t sizes[kMaxDims];
  long long strides[kMaxDims];   // byte strides of outer dims
  // narrowing cast fused into the gather: 0 none, 1 f32->bf16, 2 f32->f16.
  // With a cast, every flat-side quantity above (nbytes, row_bytes,
  // flat_off, vec) is in DESTINATION bytes; tensor_base and strides stay
  // in source bytes. A lane writes `vec` bytes and reads 2*vec.
  // Scatter only: 3 bf16->f32, 4 f16->f32 widening, same convention (flat
  // side in stored 2-byte units, tensor side in f32 bytes): a lane reads
  // `vec` stored bytes and writes 2*vec.
  uint32_t cast;
};

constexpr uint32_t kCastNone = 0;
constexpr uint32_t kCastBF16 = 1;
constexpr uint32_t kCastF16 = 2;
constexpr uint32_t kCastBF16toF32 = 3;
constexpr uint32_t kCastF16toF32 = 4;

// element classes of the non-finite scan (SCAN_* in ops/staging.py)
constexpr uint32_t kScanF64 = 0;
constexpr uint32_t kScanF32 = 1;
constexpr uint32_t kScanF16 = 2;
constexpr uint32_t kScanBF16 = 3;
constexpr uint32_t kScanE5M2 = 4;
constexpr uint32_t kScanE4M3FN = 5;
constexpr uint32_t kScanFNUZ = 6;  // e4m3fnuz and e5m2fnuz: NaN is 0x80
constexpr uint32_t kScanF32asF16 = 7;
constexpr uint32_t kScanF32asBF16 = 8;
constexpr uint32_t kScanClasses = 9;

constexpr uint32_t scan_elem_size(uint32_t cls) {
  return cls == kScanF64 ? 8u
         : (cls == kScanF32 || cls >= kScanF32asF16) ? 4u
         : (cls == kScanF16 || cls == kScanBF16) ? 2u
                                                 : 1u;
}

// flat desc rows from python: 19 u64 each (see ops/staging.py)
constexpr int kRowInts = 19;

// Decode the rows. Only what the struct itself cannot hold is refused
// here; every rule about what the kernels may be asked to do is
// check_descs' below.
inline std::vector<Desc> parse_descs(
    const std::vector<unsigned long long>& flat, int n) {
  if (n < 0 || flat.size() != (size_t)n * kRowInts) {
    throw std::runtime_error("bad descriptor array length");
  }
  std::vector<Desc> descs(n);
  for (int i = 0; i < n; ++i) {
    const unsigned long long* r = flat.data() + (size_t)i * kRowInts;
    Desc& d = descs[i];
    d.tensor_base = reinterpret_cast<const char*>(r[0]);
    d.flat_off = r[1];
    if (r[2] >= (1ull << 32)) {
      throw std::runtime_error(
          "tensor too large for pack kernel (>=4GB); chunk it upstream");
    }
    d.nbytes = (uint32_t)r[2];
    d.row_bytes = (uint32_t)r[3];
    d.vec = (uint32_t)r[4];
    if (r[5] > (unsigned long long)kMaxDims) {
      throw std::runtime_error("too many outer dims");
    }
    d.ndim = (uint32_t)r[5];
    for (int k = 0; k < kMaxDims; ++k) {
      d.sizes[k] = (uint32_t)r[6 + k];
      d.strides[k] = (long long)r[12 + k];
    }
    if (r[18] > kCastF16toF32) {
      throw std::runtime_error("unknown cast code in descriptor");
    }
    d.cast = (uint32_t)r[18];
  }
  return descs;
}

// Which entry point the descriptors are for.
enum class DescKind {
  Gather,   // pack_d2h: cast codes 0..2
  Scatter,  // scatter_h2d: plain byte scatter, no cast code
  Unpack,   // unpack_h2d: cast codes 0, 3, 4; needs a FlatSide
  Scan,     // scan_nonfinite: no cast code; needs one class per descriptor
};

// unpack_h2d's flat side: where the payload sits and how long it is
struct FlatSide {
  uintptr_t slab_ptr = 0;
  uintptr_t pinned_ptr = 0;
  unsigned long long total_bytes = 0;
  unsigned long long hash_byte0 = 0;
};

// The one validator. Shared rules, for every kind and every non-empty
// descriptor: nbytes <= kMaxDescBytes; vec in {16,8,4,2,1} ({16,8,4,2}
// under a cast); vec divides row_bytes and row_bytes divides nbytes; the
// tensor base and every outer stride are naturally aligned for the access
// the kernel makes on the tensor side (vec bytes; under a cast 2*vec, as
// two 16 B accesses at vec 16). Per-kind extras are marked below.
//
// The plain gather is held to the size cap like the rest, although
// nbytes in (2^32 - 64 KiB, 2^32) fits the descriptor: build_pack_items
// never produces it. Chunks are at most 512 MB, and StagingEngine.stage
// materialises non-contiguous tensors of 2 GiB and more before they are
// described.
inline void check_descs(const std::vector<Desc>& descs, DescKind kind,
                        const FlatSide* flat = nullptr,
                        const std::vector<uint32_t>* classes = nullptr) {
  const std::string who = kind == DescKind::Gather    ? "pack_d2h: "
                          : kind == DescKind::Scatter ? "scatter_h2d: "
                          : kind == DescKind::Unpack  ? "unpack_h2d: "
                                                      : "scan_nonfinite: ";
  auto refuse = [&who](const char* what) {
    throw std::runtime_error(who + what);
  };
  if (kind == DescKind::Unpack) {
    if (flat == nullptr) refuse("no flat side given");
    if (flat->hash_byte0 % 8 != 0) refuse("hash_byte0 must be 8-aligned");
    if (flat->slab_ptr % 16 != 0) refuse("slab must be 16-aligned");
  }
  if (kind == DescKind::Scan &&
      (classes == nullptr || classes->size() != descs.size())) {
    refuse("one class code per descriptor");
  }
  for (size_t i = 0; i < descs.size(); ++i) {
    const Desc& d = descs[i];
    const bool cast = d.cast != kCastNone;
    switch (kind) {
      case DescKind::Gather:
        if (d.cast > kCastF16) {
          refuse("widening cast descriptors are scatter-only (unpack_h2d)");
        }
        break;
      case DescKind::Scatter:
        // stays a plain byte scatter
        if (cast) refuse("does not support cast descriptors");
        break;
      case DescKind::Unpack:
        if (cast && d.cast <= kCastF16) {
          refuse("does not support narrowing cast descriptors");
        }
        break;
      case DescKind::Scan:
        if ((*classes)[i] >= kScanClasses) refuse("unknown element class");
        if (cast) refuse("cast descriptors not allowed");
        break;
    }
    if (d.nbytes == 0) continue;
    if (d.nbytes > kMaxDescBytes) {
      refuse("tensor too large (> 4 GiB - 64 KiB)");
    }
    if (kind == DescKind::Unpack &&
        (d.flat_off > flat->total_bytes ||
         d.nbytes > flat->total_bytes - d.flat_off)) {
      refuse("descriptor outside the payload");
    }
    const uint32_t v = d.vec;
    if (v != 16 && v != 8 && v != 4 && v != 2 && (v != 1 || cast)) {
      refuse(cast ? "cast descriptor: vec must be 16/8/4/2"
                  : "vec must be 16/8/4/2/1");
    }
    if (kind == DescKind::Scan && v < scan_elem_size((*classes)[i])) {
      refuse("vec below the element size");
    }
    if (d.row_bytes == 0 || d.row_bytes % v != 0 ||
        d.nbytes % d.row_bytes != 0) {
      refuse("row_bytes/vec mismatch");
    }
    if (kind == DescKind::Unpack && (flat->pinned_ptr + d.flat_off) % v != 0) {
      refuse("flat address not aligned for its vec");
    }
    // the widest single access on the tensor side
    const unsigned long long align = !cast ? v : v == 16 ? 16 : 2ull * v;
    bool ok = reinterpret_cast<uintptr_t>(d.tensor_base) % align == 0;
    unsigned long long rows = 1;
    for (uint32_t k = 0; k < d.ndim; ++k) {
      ok = ok && (unsigned long long)d.strides[k] % align == 0;
      if (kind == DescKind::Scan) {
        // loads only ever land inside the rows the descriptor names
        ok = ok && d.strides[k] >= 0 && d.sizes[k] != 0;
      }
      rows *= d.sizes[k];
    }
    if (!ok) {
      refuse(cast ? "cast descriptor: tensor side not aligned for its vec"
                  : "tensor not aligned for its vec");
    }
    if (kind == DescKind::Scan && d.ndim != 0 &&
        rows * d.row_bytes != d.nbytes) {
      refuse("sizes do not cover nbytes");
    }
  }
}

// ---------------------------------------------------------------------------
// launch prologue, host half: work-unit prefix sums, the grid cap, and the
// one host image (descriptors | prefix sums | extra array) that a launch
// uploads with a single copy into a single device allocation.
// ---------------------------------------------------------------------------

inline std::vector<unsigned long long> wu_prefix_of(
    const std::vector<Desc>& descs) {
  std::vector<unsigned long long> prefix(descs.size() + 1, 0);
  for (size_t i = 0; i < descs.size(); ++i) {
    // 64-bit: nbytes + 64 KiB does not fit a u32 at the size cap
    const unsigned long long nbytes = descs[i].nbytes;
    prefix[i + 1] = prefix[i] + (nbytes + kWorkUnitBytes - 1) / kWorkUnitBytes;
  }
  return prefix;
}

// min(total_wus, cap), at least 1; TSAMD_PACK_GRID, when a positive
// number, replaces the caller's cap
inline unsigned int grid_for(unsigned long long total_wus,
                             unsigned long long cap, const char* env) {
  if (env != nullptr) {
    const long v = std::strtol(env, nullptr, 10);
    if (v > 0) cap = (unsigned long long)v;
  }
  const unsigned long long g = total_wus < cap ? total_wus : cap;
  return (unsigned int)(g == 0 ? 1 : g);
}

struct LaunchTables {
  std::vector<char> host;  // descriptors | prefix sums | extra, 8-padded
  size_t prefix_off = 0;
  size_t extra_off = 0;

  LaunchTables(const std::vector<Desc>& descs,
               const std::vector<unsigned long long>& prefix,
               const void* extra = nullptr, size_t extra_bytes = 0) {
    static_assert(sizeof(Desc) % 8 == 0, "prefix sums must stay 8-aligned");
    prefix_off = sizeof(Desc) * descs.size();
    extra_off = prefix_off + sizeof(unsigned long long) * prefix.size();
    host.resize((extra_off + extra_bytes + 7) / 8 * 8);
    if (!descs.empty()) std::memcpy(host.data(), descs.data(), prefix_off);
    std::memcpy(host.data() + prefix_off, prefix.data(),
                extra_off - prefix_off);
    if (extra_bytes) std::memcpy(host.data() + extra_off, extra, extra_bytes);
  }
  // the three arrays inside the device copy at `dev`
  const Desc* descs(const void* dev) const {
    return static_cast<const Desc*>(dev);
  }
  const unsigned long long* prefix(const void* dev) const {
    return reinterpret_cast<const unsigned long long*>(
        static_cast<const char*>(dev) + prefix_off);
  }
  const void* extra(const void* dev) const {
    return static_cast<const char*>(dev) + extra_off;
  }
};

}  // namespace tsamd
