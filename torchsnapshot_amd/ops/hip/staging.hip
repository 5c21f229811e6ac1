// MI355X (gfx950) staging data plane for torchsnapshot_amd.
//
// What lives here:
//   - per-device side HIP streams: checkpoint D2H traffic runs beside the
//     training step's streams, so staging overlaps compute
//   - gather-pack kernel: N strided device tensors -> one contiguous slab,
//     in a single launch (replaces the reference's per-tensor
//     UntypedStorage copies + ByteTensor slab, torchsnapshot/batcher.py
//     :104-162, and its tensor.cpu() staging, io_preparers/tensor.py:353)
//   - gather-and-cast: per-descriptor f32 -> bf16/f16 narrowing fused into
//     the same launch (save_dtype), so only stored-size bytes leave the GPU
//   - scatter kernel for restore (and for scatter_h2d), with bf16/f16 ->
//     f32 widening and the psum64 check fused into the launch
//   - block-scaled saves (mxfp8_e4m3, mxfp4_e2m1): one set of gather and
//     scatter routes over the format structs and bit arithmetic of
//     mx_codec.h, in a gather and a scatter kernel of their own
//   - scan kernel: NaN / Inf counts per tensor over the same descriptors,
//     read-only, one launch for the whole state (the nonfinite= policy)
//   - fingerprint kernel: the psum64 of each tensor's stored bytes, read in
//     place over the same descriptors (the replicated_check= policy)
//   - stats kernel: count, zeros, min, max, sum and sum of squares of each
//     tensor's finite elements in f64, read in place over the same
//     descriptors, with sums that are bit-identical for any grid (stats=)
//   - histogram kernel: the distribution of floor(log2|x|) of each tensor
//     over the same descriptors, binned in 32 private LDS copies of 280
//     counters per workgroup (histogram=)
//   - compare kernel: a stored payload, read in place from pinned host
//     memory or from HBM, against the live strided tensors element by
//     element; both sides read-only, six words per tensor, the f64 sums
//     through the stats kernel's two-stage reduction (Snapshot.compare)
//   - SDMA copies (hipMemcpyAsync) slab <-> pinned host memory; the slab
//     can also be skipped entirely ("direct" mode): the kernel writes
//     gathered bytes straight into pinned host memory over PCIe
//
// How the kernels are put together. There is one of each of these, and
// every kernel is a composition of them:
//   - for_each_work_unit: grid-stride loop over 64 KiB work units, the
//     owner search over the prefix sums, the unit's byte range [s, e)
//   - for_each_vec<VEC, TS>: the three-way traversal of that range
//     (contiguous / wide rows / narrow rows), calling a lane operation
//     with (flat index, tensor address). TS = tensor bytes per flat byte:
//     1 for copy, scatter and scan, 2 for cast and widen
//   - lane operations: copy_vec (+ psum_contrib), cast_vec, scatter_vec,
//     widen_vec, scan_vec; the fingerprint's is psum_contrib alone, or
//     cast_regs + psum_regs, the register half of cast_vec. Each kernel
//     family differs only in this
//   - add_per_wave: wave64 reduction and one atomic per wave, for the u64
//     hashes and the u32 counters alike
//   - on the host (desc_check.h): parse_descs + check_descs validate every
//     descriptor before the GPU is touched; wu_prefix_of, grid_for and
//     LaunchTables are the launch prologue of both launchers: launch_pack
//     for the copies, read_launch for the blocking read-only scan,
//     fingerprint, statistics and histogram
//   - on the host (table_ring.h): the launch tables reach the device
//     through a ring of pinned slots, so a launch never waits for the
//     stream it enqueues on, and the launch entry points hold no GIL
//
// Design notes (CDNA4):
//   - wave64; block = 256 threads; work units of 64 KiB of slab bytes,
//     grid-strided with >> 256 workgroups so all 8 XCDs fill
//   - wide rows (>= 2 KiB contiguous) copy lane-across-columns with the
//     widest vector the layout allows (16 B/lane -> 1 KiB per wave per
//     instruction); narrow rows copy lane-per-row so writes to the slab
//     stay coalesced across lanes even when reads are scattered
//   - all within-tensor indices fit u32 (check_descs caps a descriptor at
//     4 GiB - 64 KiB; tensors are chunked to <= 512 MB upstream);
//     row->coordinate decomposition uses u32 div/mod. Tensor-side offsets
//     are 64-bit: under a cast they are twice the flat index
//
// Deliberately torch-free: tensors enter as raw pointers; stream ordering
// against the producer is a caller-provided stream handle we event-chain.
// This keeps the extension ABI-independent of the torch build.

#include <hip/hip_runtime.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "desc_check.h"
#include "file_sink.h"
#include "table_ring.h"

namespace py = pybind11;

#define HIP_CHECK(expr)                                                     \
  do {                                                                      \
    hipError_t _e = (expr);                                                 \
    if (_e != hipSuccess) {                                                 \
      throw std::runtime_error(std::string("HIP error at " #expr ": ") +    \
                               hipGetErrorString(_e));                      \
    }                                                                       \
  } while (0)

namespace {

// Desc, the cast and scan codes, kWorkUnitBytes and the host-side checks
using namespace tsamd;

constexpr int kBlockThreads = 256;
constexpr uint32_t kWideRowBytes = 2048;

// ---------------------------------------------------------------------------
// psum64 checksum: an order-independent weighted word sum over the flat
// payload. contribution(byte b, value v) treats the payload as little-endian
// u64 words at FILE offsets: word w = flat_offset+b >> 3, lane = b & 7, and
// adds (v << 8*lane) * M(w) where M(w) = splitmix64(w) | 1. Linear in the
// value bytes, so any write width (16/8/4/2/1) contributes independently —
// the CPU verifier just does sum(words * M(index)) over the whole file
// (padding bytes are zeroed, contributing nothing).
// ---------------------------------------------------------------------------

__device__ __host__ inline unsigned long long psum_mult(unsigned long long w) {
  // splitmix64 finalizer
  unsigned long long z = w + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  return z | 1ull;  // odd multiplier
}

template <int VEC>
__device__ inline unsigned long long psum_contrib(
    const char* bytes, unsigned long long file_off) {
  unsigned long long acc = 0;
  if (VEC == 16) {
    const unsigned long long* p = reinterpret_cast<const unsigned long long*>(bytes);
    unsigned long long w = file_off >> 3;
    acc += p[0] * psum_mult(w);
    acc += p[1] * psum_mult(w + 1);
  } else if (VEC == 8) {
    acc += *reinterpret_cast<const unsigned long long*>(bytes) *
           psum_mult(file_off >> 3);
  } else {
    // narrow writes: shift the piece into its word lane
    unsigned long long v = 0;
    if (VEC == 4) v = *reinterpret_cast<const uint32_t*>(bytes);
    else if (VEC == 2) v = *reinterpret_cast<const uint16_t*>(bytes);
    else v = *reinterpret_cast<const unsigned char*>(bytes);
    acc += (v << (8 * (file_off & 7))) * psum_mult(file_off >> 3);
  }
  return acc;
}

// byte offset of row `row` within the strided tensor (excluding columns)
__device__ inline unsigned long long row_offset(const Desc& d, uint32_t row) {
  unsigned long long off = 0;
  uint32_t rem = row;
#pragma unroll
  for (int k = kMaxDims - 1; k >= 0; --k) {
    if (k >= (int)d.ndim) continue;
    uint32_t sz = d.sizes[k];
    uint32_t idx = rem % sz;
    rem /= sz;
    off += (unsigned long long)idx * (unsigned long long)d.strides[k];
  }
  return off;
}

// ---------------------------------------------------------------------------
// The traversal: visit [s, e) of one descriptor's flat byte range, VEC
// flat bytes per call, as op(flat_index, tensor_address). TS is the number
// of tensor bytes per flat byte (2 under a cast: the tensor side is f32,
// the flat side 16-bit), applied in 64 bits: a contiguous tensor just
// under 4 GiB stored has just under 8 GiB of f32. The flat index is handed
// over widened to 64 bits as row start + lane offset, so that `flat + index`
// in a lane operation splits into a per-row base and a small offset; as a
// u32 sum it cost the cast and widen kernels 6-8 VGPRs and one wave of
// occupancy (profiles/traversal_refactor_measurements.md). UNROLL > 1 asks
// for that unroll of the contiguous loop (the scan's loads are independent
// and its body is small; the copies are left to the compiler).
// ---------------------------------------------------------------------------

template <int VEC, int TS, int UNROLL = 1, typename Op>
__device__ __forceinline__ void for_each_vec(const Desc& d, uint32_t s,
                                             uint32_t e, Op op) {
  const uint32_t tid = threadIdx.x;
  const uint32_t rb = d.row_bytes;
  const char* base = d.tensor_base;
  if (d.ndim == 0 || rb == d.nbytes) {
    // fully contiguous: lanes across [s, e)
    if constexpr (UNROLL > 1) {
#pragma unroll UNROLL
      for (uint32_t i = s + tid * VEC; i < e; i += kBlockThreads * VEC) {
        op(i, base + (unsigned long long)TS * i);
      }
    } else {
      for (uint32_t i = s + tid * VEC; i < e; i += kBlockThreads * VEC) {
        op(i, base + (unsigned long long)TS * i);
      }
    }
    return;
  }
  if (rb >= kWideRowBytes) {
    // wide rows: rows sequential, lanes across columns
    uint32_t row = s / rb;
    uint32_t col = s - row * rb;
    uint32_t off = s;
    while (off < e) {
      const char* p = base + row_offset(d, row) + (unsigned long long)TS * col;
      uint32_t n = min(rb - col, e - off);
      for (uint32_t i = tid * VEC; i < n; i += kBlockThreads * VEC) {
        op((unsigned long long)off + i, p + (unsigned long long)TS * i);
      }
      off += n;
      ++row;
      col = 0;
    }
  } else {
    // narrow rows: one lane per row; flat-side access stays coalesced
    uint32_t first_row = s / rb;
    uint32_t last_row = (e - 1) / rb;
    for (uint32_t r = first_row + tid; r <= last_row; r += kBlockThreads) {
      const char* p = base + row_offset(d, r);
      uint32_t flat_pos = r * rb;
      uint32_t lo = flat_pos < s ? (s - flat_pos) : 0;
      uint32_t hi = (flat_pos + rb > e) ? (e - flat_pos) : rb;
      for (uint32_t i = lo; i < hi; i += VEC) {
        op((unsigned long long)flat_pos + i, p + (unsigned long long)TS * i);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// The work-unit driver: grid-stride over all work units of the batch,
// find the descriptor that owns each, and hand body(owner, desc, s, e)
// the unit's flat byte range. check_descs caps nbytes at 2^32 - 64 KiB,
// and `e` is formed without adding to `s` first, so nothing here or in
// the traversal wraps a u32.
// ---------------------------------------------------------------------------

template <typename Body>
__device__ __forceinline__ void for_each_work_unit(
    const Desc* __restrict__ descs, int n,
    const unsigned long long* __restrict__ wu_prefix,
    unsigned long long total_wus, Body body) {
  for (unsigned long long wu = blockIdx.x; wu < total_wus; wu += gridDim.x) {
    // binary search: which tensor owns this work unit
    int lo = 0, hi = n - 1;
    while (lo < hi) {
      int mid = (lo + hi + 1) >> 1;
      if (wu_prefix[mid] <= wu) lo = mid;
      else hi = mid - 1;
    }
    const Desc d = descs[lo];
    unsigned long long local_wu = wu - wu_prefix[lo];
    uint32_t s = (uint32_t)(local_wu * kWorkUnitBytes);
    uint32_t e = d.nbytes - s > kWorkUnitBytes ? s + kWorkUnitBytes : d.nbytes;
    body(lo, d, s, e);
  }
}

// wave64 reduction, then one atomic per wave per work unit (none for zero)
template <typename T>
__device__ __forceinline__ void add_per_wave(unsigned long long* dst, T v) {
  for (int delta = 32; delta > 0; delta >>= 1) {
    v += __shfl_down(v, delta, 64);
  }
  if ((threadIdx.x & 63) == 0 && v != 0) {
    atomicAdd(dst, (unsigned long long)v);
  }
}

template <int VEC>
__device__ inline void copy_vec(char* flat, const char* strided) {
  if (VEC == 16)
    *reinterpret_cast<uint4*>(flat) = *reinterpret_cast<const uint4*>(strided);
  else if (VEC == 8)
    *reinterpret_cast<uint64_t*>(flat) = *reinterpret_cast<const uint64_t*>(strided);
  else if (VEC == 4)
    *reinterpret_cast<uint32_t*>(flat) = *reinterpret_cast<const uint32_t*>(strided);
  else if (VEC == 2)
    *reinterpret_cast<uint16_t*>(flat) = *reinterpret_cast<const uint16_t*>(strided);
  else
    *flat = *strided;
}

// Scatter VEC flat bytes into the strided tensor. When HASH, returns the
// psum64 contribution of those bytes, computed from the registers just
// loaded: the flat side may be uncached host memory across PCIe and is
// read exactly once.
template <int VEC, bool HASH>
__device__ inline unsigned long long scatter_vec(
    char* strided, const char* flat, unsigned long long file_off) {
  unsigned long long h = 0;
  if (VEC == 16) {
    const uint4 a = *reinterpret_cast<const uint4*>(flat);
    *reinterpret_cast<uint4*>(strided) = a;
    if (HASH) {
      unsigned long long w = file_off >> 3;
      h += (((unsigned long long)a.y << 32) | a.x) * psum_mult(w);
      h += (((unsigned long long)a.w << 32) | a.z) * psum_mult(w + 1);
    }
  } else if (VEC == 8) {
    const unsigned long long a =
        *reinterpret_cast<const unsigned long long*>(flat);
    *reinterpret_cast<unsigned long long*>(strided) = a;
    if (HASH) h += a * psum_mult(file_off >> 3);
  } else {
    unsigned long long v;
    if (VEC == 4) {
      const uint32_t a = *reinterpret_cast<const uint32_t*>(flat);
      *reinterpret_cast<uint32_t*>(strided) = a;
      v = a;
    } else if (VEC == 2) {
      const uint16_t a = *reinterpret_cast<const uint16_t*>(flat);
      *reinterpret_cast<uint16_t*>(strided) = a;
      v = a;
    } else {
      const unsigned char a = *reinterpret_cast<const unsigned char*>(flat);
      *reinterpret_cast<unsigned char*>(strided) = a;
      v = a;
    }
    if (HASH) h += (v << (8 * (file_off & 7))) * psum_mult(file_off >> 3);
  }
  return h;
}

// Gather [s, e) of the tensor's flat byte range for one work unit. When
// HASH, returns this thread's psum64 contribution at slab offsets.
template <int VEC, bool HASH>
__device__ unsigned long long gather_range(const Desc& d, char* flat_base,
                                           uint32_t s, uint32_t e) {
  char* flat = flat_base + d.flat_off;
  unsigned long long h = 0;
  for_each_vec<VEC, 1>(d, s, e, [&](unsigned long long i, const char* src) {
    copy_vec<VEC>(flat + i, src);
    if (HASH) h += psum_contrib<VEC>(src, d.flat_off + i);
  });
  return h;
}

// Scatter counterpart: hashes at `hash_off`, the file offset of the
// descriptor's first flat byte.
template <int VEC, bool HASH>
__device__ unsigned long long scatter_range(const Desc& d,
                                            const char* flat_base, uint32_t s,
                                            uint32_t e,
                                            unsigned long long hash_off) {
  const char* flat = flat_base + d.flat_off;
  unsigned long long h = 0;
  for_each_vec<VEC, 1>(d, s, e, [&](unsigned long long i, const char* dst) {
    h += scatter_vec<VEC, HASH>(const_cast<char*>(dst), flat + i,
                                hash_off + i);
  });
  return h;
}

// ---------------------------------------------------------------------------
// gather-and-cast (f32 -> bf16 / f16). Integer round-to-nearest-even on
// the bit patterns: no dependence on the wave's denormal mode, so f32
// subnormal inputs and f16 subnormal results are exact. The kernel is
// PCIe- or HBM-bound; the handful of integer ops per element is free.
// ---------------------------------------------------------------------------

__device__ __host__ inline uint32_t f32_to_bf16_bits(uint32_t u) {
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) {
    return (u >> 16) | 0x0040u;  // NaN stays NaN (quiet bit set)
  }
  // RNE; the carry runs into the exponent, so overflow lands on +-inf
  return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

__device__ __host__ inline uint32_t f32_to_f16_bits(uint32_t u) {
  const uint32_t sign = (u >> 16) & 0x8000u;
  const uint32_t a = u & 0x7FFFFFFFu;
  if (a > 0x7F800000u) return sign | 0x7E00u;   // NaN
  if (a >= 0x47800000u) return sign | 0x7C00u;  // >= 65536 (and inf)
  if (a >= 0x38800000u) {
    // f16-normal range: rebias the exponent (127 -> 15), RNE off 13 bits;
    // 65520 <= |x| < 65536 carries to 0x7C00 = inf
    uint32_t r = a - 0x38000000u;
    r += 0x0FFFu + ((r >> 13) & 1u);
    return sign | (r >> 13);
  }
  if (a < 0x33000000u) return sign;  // < 2^-25 (incl. f32 subnormals): +-0
  // f16-subnormal range: result = RNE(|x| / 2^-24); shift is 14..24
  const uint32_t mant = (a & 0x007FFFFFu) | 0x00800000u;
  const uint32_t shift = 126u - (a >> 23);
  uint32_t h = mant >> shift;
  const uint32_t rem = mant & ((1u << shift) - 1u);
  const uint32_t half = 1u << (shift - 1u);
  if (rem > half || (rem == half && (h & 1u))) ++h;  // may carry to 0x0400
  return sign | h;
}

__device__ inline uint32_t cast_pair(uint32_t lo, uint32_t hi, uint32_t code) {
  // two f32 bit patterns -> two 16-bit results packed little-endian
  if (code == kCastBF16) {
    return (f32_to_bf16_bits(lo) & 0xFFFFu) | (f32_to_bf16_bits(hi) << 16);
  }
  return f32_to_f16_bits(lo) | (f32_to_f16_bits(hi) << 16);
}

// The register part of the narrowing, shared by the gather and the
// fingerprint: read 2*VEC source bytes at `src` and return the VEC stored
// bytes packed little-endian in the low words of a uint4 (x | y | z | w;
// at VEC 2 the low half of x). Every load is naturally aligned to its own
// width (the host picks vec so).
template <int VEC>
__device__ inline uint4 cast_regs(const char* src, uint32_t code) {
  uint4 o = make_uint4(0u, 0u, 0u, 0u);
  if (VEC == 16) {
    const uint4 a = *reinterpret_cast<const uint4*>(src);
    const uint4 b = *reinterpret_cast<const uint4*>(src + 16);
    o.x = cast_pair(a.x, a.y, code);
    o.y = cast_pair(a.z, a.w, code);
    o.z = cast_pair(b.x, b.y, code);
    o.w = cast_pair(b.z, b.w, code);
  } else if (VEC == 8) {
    const uint4 a = *reinterpret_cast<const uint4*>(src);
    o.x = cast_pair(a.x, a.y, code);
    o.y = cast_pair(a.z, a.w, code);
  } else if (VEC == 4) {
    const uint2 a = *reinterpret_cast<const uint2*>(src);
    o.x = cast_pair(a.x, a.y, code);
  } else {
    const uint32_t a = *reinterpret_cast<const uint32_t*>(src);
    o.x = (code == kCastBF16 ? f32_to_bf16_bits(a) : f32_to_f16_bits(a)) &
          0xFFFFu;
  }
  return o;
}

// psum64 contribution of the VEC stored bytes cast_regs returned
template <int VEC>
__device__ inline unsigned long long psum_regs(const uint4& o,
                                               unsigned long long file_off) {
  if (VEC == 16) {
    const unsigned long long w = file_off >> 3;
    return (((unsigned long long)o.y << 32) | o.x) * psum_mult(w) +
           (((unsigned long long)o.w << 32) | o.z) * psum_mult(w + 1);
  }
  if (VEC == 8) {
    return (((unsigned long long)o.y << 32) | o.x) * psum_mult(file_off >> 3);
  }
  return ((unsigned long long)o.x << (8 * (file_off & 7))) *
         psum_mult(file_off >> 3);
}

// Convert 2*VEC source bytes at `src` into VEC bytes at `flat`; the store
// is naturally aligned to its own width. When HASH, returns the psum64
// contribution of the STORED bytes.
template <int VEC, bool HASH>
__device__ inline unsigned long long cast_vec(char* flat, const char* src,
                                              uint32_t code,
                                              unsigned long long file_off) {
  const uint4 o = cast_regs<VEC>(src, code);
  if (VEC == 16)
    *reinterpret_cast<uint4*>(flat) = o;
  else if (VEC == 8)
    *reinterpret_cast<uint2*>(flat) = make_uint2(o.x, o.y);
  else if (VEC == 4)
    *reinterpret_cast<uint32_t*>(flat) = o.x;
  else
    *reinterpret_cast<uint16_t*>(flat) = (uint16_t)o.x;
  return HASH ? psum_regs<VEC>(o, file_off) : 0ull;
}

// Cast counterpart of gather_range: [s, e) is in destination (flat-side)
// bytes, the f32 source sits at twice the offset.
template <int VEC, bool HASH>
__device__ unsigned long long cast_range(const Desc& d, char* flat_base,
                                         uint32_t s, uint32_t e) {
  char* flat = flat_base + d.flat_off;
  const uint32_t code = d.cast;
  unsigned long long h = 0;
  for_each_vec<VEC, 2>(d, s, e, [&](unsigned long long i, const char* src) {
    h += cast_vec<VEC, HASH>(flat + i, src, code, d.flat_off + i);
  });
  return h;
}

// One plain or cast descriptor's work unit of the gather, by its vec. Only
// CAST instantiations hold the cast route.
template <bool HASH, bool CAST>
__device__ __forceinline__ unsigned long long pack_unit(const Desc& d,
                                                        char* flat_base,
                                                        uint32_t s,
                                                        uint32_t e) {
  if (CAST && d.cast != kCastNone) {
    switch (d.vec) {
      case 16: return cast_range<16, HASH>(d, flat_base, s, e);
      case 8: return cast_range<8, HASH>(d, flat_base, s, e);
      case 4: return cast_range<4, HASH>(d, flat_base, s, e);
      default: return cast_range<2, HASH>(d, flat_base, s, e);
    }
  }
  switch (d.vec) {
    case 16: return gather_range<16, HASH>(d, flat_base, s, e);
    case 8: return gather_range<8, HASH>(d, flat_base, s, e);
    case 4: return gather_range<4, HASH>(d, flat_base, s, e);
    case 2: return gather_range<2, HASH>(d, flat_base, s, e);
    default: return gather_range<1, HASH>(d, flat_base, s, e);
  }
}

// Gather kernel; when HASH, hash_out[i] accumulates the psum64 of
// descriptor i's bytes at slab offsets. CAST instantiations additionally
// route descriptors with a cast code to cast_range; they are launched only
// for batches that contain one.
template <bool HASH, bool CAST>
__global__ __launch_bounds__(kBlockThreads) void pack_kernel(
    const Desc* __restrict__ descs, int n,
    const unsigned long long* __restrict__ wu_prefix,
    unsigned long long total_wus, char* __restrict__ flat_base,
    unsigned long long* __restrict__ hash_out) {
  for_each_work_unit(
      descs, n, wu_prefix, total_wus,
      [&](int owner, const Desc& d, uint32_t s, uint32_t e) {
        const unsigned long long h = pack_unit<HASH, CAST>(d, flat_base, s, e);
        if (HASH) add_per_wave(&hash_out[owner], h);
      });
}

// ---------------------------------------------------------------------------
// scatter-and-widen (bf16 / f16 -> f32), the restore half of save_dtype.
// Exact integer bit arithmetic like the narrowing above: no dependence on
// the wave's denormal mode, f16 subnormals renormalise exactly.
// ---------------------------------------------------------------------------

__device__ __host__ inline uint32_t bf16_to_f32_bits(uint32_t b) {
  return b << 16;  // every pattern, NaN payloads included
}

__device__ __host__ inline uint32_t f16_to_f32_bits(uint32_t h) {
  const uint32_t sign = (h & 0x8000u) << 16;
  const uint32_t exp = (h >> 10) & 0x1Fu;
  const uint32_t mant = h & 0x03FFu;
  if (exp == 0x1Fu) {
    // inf keeps a zero mantissa; NaN turns quiet, payload kept
    return sign | 0x7F800000u | (mant << 13) | (mant ? 0x00400000u : 0u);
  }
  if (exp != 0u) return sign | ((exp + 112u) << 23) | (mant << 13);
  if (mant == 0u) return sign;  // +-0
  // subnormal: mant * 2^-24. Shift the leading one up to bit 10 (the
  // implicit bit); each position shifted lowers the exponent from 2^-14
  const uint32_t shift = (uint32_t)__builtin_clz(mant) - 21u;  // 1..10
  return sign | ((113u - shift) << 23) | (((mant << shift) & 0x03FFu) << 13);
}

__device__ inline uint2 widen_pair(uint32_t packed, uint32_t code) {
  // two 16-bit patterns packed little-endian -> two f32 bit patterns
  uint2 o;
  if (code == kCastBF16toF32) {
    o.x = bf16_to_f32_bits(packed & 0xFFFFu);
    o.y = packed & 0xFFFF0000u;
  } else {
    o.x = f16_to_f32_bits(packed & 0xFFFFu);
    o.y = f16_to_f32_bits(packed >> 16);
  }
  return o;
}

// Convert VEC stored bytes at `flat` into 2*VEC bytes at `dst`. Every load
// and store is naturally aligned to its own width (the host picks vec so).
// When HASH, returns the psum64 contribution of the STORED bytes, taken
// from the registers the conversion reads.
template <int VEC, bool HASH>
__device__ inline unsigned long long widen_vec(char* dst, const char* flat,
                                               uint32_t code,
                                               unsigned long long file_off) {
  unsigned long long h = 0;
  if (VEC == 16) {
    const uint4 a = *reinterpret_cast<const uint4*>(flat);
    const uint2 p0 = widen_pair(a.x, code), p1 = widen_pair(a.y, code);
    const uint2 p2 = widen_pair(a.z, code), p3 = widen_pair(a.w, code);
    *reinterpret_cast<uint4*>(dst) = make_uint4(p0.x, p0.y, p1.x, p1.y);
    *reinterpret_cast<uint4*>(dst + 16) = make_uint4(p2.x, p2.y, p3.x, p3.y);
    if (HASH) {
      unsigned long long w = file_off >> 3;
      h += (((unsigned long long)a.y << 32) | a.x) * psum_mult(w);
      h += (((unsigned long long)a.w << 32) | a.z) * psum_mult(w + 1);
    }
  } else if (VEC == 8) {
    const uint2 a = *reinterpret_cast<const uint2*>(flat);
    const uint2 p0 = widen_pair(a.x, code), p1 = widen_pair(a.y, code);
    *reinterpret_cast<uint4*>(dst) = make_uint4(p0.x, p0.y, p1.x, p1.y);
    if (HASH) {
      h += (((unsigned long long)a.y << 32) | a.x) * psum_mult(file_off >> 3);
    }
  } else if (VEC == 4) {
    const uint32_t a = *reinterpret_cast<const uint32_t*>(flat);
    *reinterpret_cast<uint2*>(dst) = widen_pair(a, code);
    if (HASH) {
      h += ((unsigned long long)a << (8 * (file_off & 7))) *
           psum_mult(file_off >> 3);
    }
  } else {
    const uint32_t a = *reinterpret_cast<const uint16_t*>(flat);
    *reinterpret_cast<uint32_t*>(dst) =
        code == kCastBF16toF32 ? bf16_to_f32_bits(a) : f16_to_f32_bits(a);
    if (HASH) {
      h += ((unsigned long long)a << (8 * (file_off & 7))) *
           psum_mult(file_off >> 3);
    }
  }
  return h;
}

// Widen counterpart of scatter_range: [s, e) is in stored (flat-side)
// bytes, the f32 target sits at twice the offset.
template <int VEC, bool HASH>
__device__ unsigned long long widen_range(const Desc& d,
                                          const char* flat_base, uint32_t s,
                                          uint32_t e,
                                          unsigned long long hash_off) {
  const char* flat = flat_base + d.flat_off;
  const uint32_t code = d.cast;
  unsigned long long h = 0;
  for_each_vec<VEC, 2>(d, s, e, [&](unsigned long long i, const char* dst) {
    h += widen_vec<VEC, HASH>(const_cast<char*>(dst), flat + i, code,
                              hash_off + i);
  });
  return h;
}

// One plain or cast descriptor's work unit of the scatter, by its vec. Only
// WIDEN instantiations hold the widening route.
template <bool HASH, bool WIDEN>
__device__ __forceinline__ unsigned long long unpack_unit(
    const Desc& d, const char* fb, uint32_t s, uint32_t e,
    unsigned long long ho) {
  if (WIDEN && d.cast != kCastNone) {
    switch (d.vec) {
      case 16: return widen_range<16, HASH>(d, fb, s, e, ho);
      case 8: return widen_range<8, HASH>(d, fb, s, e, ho);
      case 4: return widen_range<4, HASH>(d, fb, s, e, ho);
      default: return widen_range<2, HASH>(d, fb, s, e, ho);
    }
  }
  switch (d.vec) {
    case 16: return scatter_range<16, HASH>(d, fb, s, e, ho);
    case 8: return scatter_range<8, HASH>(d, fb, s, e, ho);
    case 4: return scatter_range<4, HASH>(d, fb, s, e, ho);
    case 2: return scatter_range<2, HASH>(d, fb, s, e, ho);
    default: return scatter_range<1, HASH>(d, fb, s, e, ho);
  }
}

// Scatter kernel (restore, and scatter_h2d): flat bytes into strided
// device tensors, widening when WIDEN; when HASH, hash_out[i] accumulates
// the psum64 of descriptor i's flat bytes at file offset hash_byte0 +
// flat_off. It is the gather with the lane operation reversed: same
// driver, same traversal. It stays a kernel of its own because its flat
// side is read-only and its hash offsets are file offsets, which takes
// one more argument than the gather has.
template <bool HASH, bool WIDEN>
__global__ __launch_bounds__(kBlockThreads) void unpack_kernel(
    const Desc* __restrict__ descs, int n,
    const unsigned long long* __restrict__ wu_prefix,
    unsigned long long total_wus, const char* __restrict__ flat_base,
    unsigned long long* __restrict__ hash_out,
    unsigned long long hash_byte0) {
  for_each_work_unit(
      descs, n, wu_prefix, total_wus,
      [&](int owner, const Desc& d, uint32_t s, uint32_t e) {
        const unsigned long long h = unpack_unit<HASH, WIDEN>(
            d, flat_base, s, e, hash_byte0 + d.flat_off);
        if (HASH) add_per_wave(&hash_out[owner], h);
      });
}

// ---------------------------------------------------------------------------
// block-scaled saves (mxfp8_e4m3 and mxfp4_e2m1; docs/format.md): 32
// elements share one power-of-two scale byte X = E + 127 (E8M0), each
// element is one code of x * 2^-E. A payload is [codes: B*nb bytes][scales:
// nb bytes], B = FMT::kBlockBytes code bytes per block. The descriptor's flat
// range is the codes region, so a 64 KiB work unit is 65536 / B blocks and
// owns that many scale bytes at flat_off + nbytes + s / B. The formats are
// the structs of mx_codec.h, which also holds the bit arithmetic; every
// route below is one template over them.
//
//   - aligned class (vec 8: contiguous tensors, and rows of 32k elements
//     with a 16 B aligned tensor side): lanes run across the unit, 8
//     elements each: one 16 B load of bf16 or two of f32. The four lanes of
//     a block reduce amax on the bit patterns (the order of non-negative
//     floats is the order of their patterns) with two xor shuffles; a block
//     never crosses a wave. Each lane converts its 8 elements and stores
//     their code bytes in one piece
//   - general class (vec 1: every other layout): one lane per block, two
//     passes over its elements, taking row_offset again at each row
//     boundary: the first takes amax, the second reads them again (from
//     cache) and encodes them dword by dword. The loops over a block's
//     pieces, dwords and codes have constant trip counts and nothing is
//     indexed at run time, so the block never sits in private memory; the
//     codes leave as 16 B stores. (fp8 alone walks once and keeps the block
//     in registers, see mx_gather_general.) The scatter loads a block's
//     codes as 16 B pieces and walks the rows once
//   - scales never leave as single bytes (in direct mode the flat side is
//     pinned host memory across PCIe): the unit's scale bytes are collected
//     in LDS and, after a workgroup barrier, written as 16 B pieces; only
//     the payload's last, short piece goes narrower. The scatter mirrors
//     this: it first loads the unit's scales into LDS with 16 B loads (the
//     flat side is read exactly once), then decodes
//   - psum64: codes are hashed from the registers stored (or loaded), scales
//     where they leave (enter) LDS, at their own payload offsets
//   - the kernels below also run plain and cast descriptors, so a slab may
//     mix all of them; they are launched only for batches that hold an mx
//     descriptor, and pack_kernel / unpack_kernel stay as they were
//
// What a format changes, and nothing else:
//   - mxfp8_e4m3: B = 32, a unit is 2048 blocks. A lane of the aligned class
//     stores 8 code bytes, a wave 512 contiguous bytes; a block of the
//     general class is two 16 B pieces. The codes carry NaN themselves
//   - mxfp4_e2m1: B = 16, two codes per byte, element 2j of a block in the
//     low nibble of its byte j; a unit is 4096 blocks (131072 elements),
//     which sizes the LDS buffer at 4 KiB. A lane of the aligned class packs
//     its eight nibbles into one dword, a wave stores 256 contiguous bytes;
//     a block of the general class is one 16 B piece. e2m1 has no NaN and
//     no Inf: a block with a non-finite element stores X = 0xFF (the whole
//     block decodes to NaN), its non-finite elements magnitude 7. Whether a
//     block has one is a ballot over its four lanes
// ---------------------------------------------------------------------------

// the most blocks a work unit holds in any format: the LDS scale buffer
constexpr uint32_t kMxUnitBlocks = kWorkUnitBytes / MxFp4E2M1::kBlockBytes;
static_assert(MxFp8E4M3::kBlockBytes >= MxFp4E2M1::kBlockBytes);

__device__ __forceinline__ unsigned long long psum_piece(
    unsigned long long v, unsigned long long file_off) {
  // a naturally aligned piece of at most 8 bytes, shifted into its word lane
  return (v << (8 * (file_off & 7))) * psum_mult(file_off >> 3);
}

// 8 consecutive source elements as f32 patterns; the ones from `valid` on do
// not exist and read as +0. A bf16 source is its f32 pattern (<< 16)
template <bool BF16>
__device__ __forceinline__ void mx_load8(const char* src, uint32_t valid,
                                         uint32_t (&v)[8]) {
  if (valid >= 8) {
    const uint4 a = *reinterpret_cast<const uint4*>(src);
    if (BF16) {
      v[0] = a.x << 16; v[1] = a.x & 0xFFFF0000u;
      v[2] = a.y << 16; v[3] = a.y & 0xFFFF0000u;
      v[4] = a.z << 16; v[5] = a.z & 0xFFFF0000u;
      v[6] = a.w << 16; v[7] = a.w & 0xFFFF0000u;
    } else {
      const uint4 b = *reinterpret_cast<const uint4*>(src + 16);
      v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
      v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    }
  } else {
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) {
      v[k] = 0u;
      if (k < valid) {
        v[k] = BF16 ? (uint32_t)reinterpret_cast<const uint16_t*>(src)[k] << 16
                    : reinterpret_cast<const uint32_t*>(src)[k];
      }
    }
  }
}

__device__ __forceinline__ bool mx_nonfinite(uint32_t u) {
  return (u & 0x7FFFFFFFu) >= 0x7F800000u;
}

// amax pattern of one element: non-finite elements do not exist for it
__device__ __forceinline__ uint32_t mx_amax_of(uint32_t u) {
  return mx_nonfinite(u) ? 0u : u & 0x7FFFFFFFu;
}

// where element i of an aligned-class tensor sits, and how many of the 8
// elements from it on exist
template <int TS>
__device__ __forceinline__ const char* mx_aligned_addr(const Desc& d,
                                                       uint32_t i,
                                                       uint32_t& valid) {
  if (d.ndim == 0) {
    const uint32_t n = d.row_bytes;
    valid = i < n ? n - i : 0u;
    return d.tensor_base + (unsigned long long)TS * i;
  }
  // rows of 32k elements tile the codes region: every element exists
  const uint32_t row = i / d.row_bytes;
  const uint32_t col = i - row * d.row_bytes;
  valid = 8u;
  return d.tensor_base + row_offset(d, row) + (unsigned long long)TS * col;
}

// The aligned class's lane piece: the codes of a lane's 8 elements are
// FMT::kBits bytes, stored (and loaded) as one naturally aligned piece, a
// uint2 or a dword. When HASH, `h` takes its psum64 contribution.
template <typename FMT, bool HASH>
__device__ __forceinline__ void mx_store_lane(char* flat,
                                              const uint32_t (&c)[2],
                                              unsigned long long file_off,
                                              unsigned long long& h) {
  if constexpr (FMT::kBits == 8) {
    *reinterpret_cast<uint2*>(flat) = make_uint2(c[0], c[1]);
    if (HASH) {
      h += (((unsigned long long)c[1] << 32) | c[0]) * psum_mult(file_off >> 3);
    }
  } else {
    static_assert(FMT::kBits == 4, "a lane's codes are a uint2 or a dword");
    *reinterpret_cast<uint32_t*>(flat) = c[0];
    if (HASH) h += psum_piece(c[0], file_off);
  }
}

template <typename FMT, bool HASH>
__device__ __forceinline__ void mx_load_lane(const char* flat, uint32_t (&c)[2],
                                             unsigned long long file_off,
                                             unsigned long long& h) {
  if constexpr (FMT::kBits == 8) {
    const uint2 a = *reinterpret_cast<const uint2*>(flat);
    c[0] = a.x;
    c[1] = a.y;
    if (HASH) {
      h += (((unsigned long long)c[1] << 32) | c[0]) * psum_mult(file_off >> 3);
    }
  } else {
    static_assert(FMT::kBits == 4, "a lane's codes are a uint2 or a dword");
    c[0] = *reinterpret_cast<const uint32_t*>(flat);
    c[1] = 0u;
    if (HASH) h += psum_piece(c[0], file_off);
  }
}

// Aligned gather of [s, e) of the codes region of one work unit; the unit's
// scale bytes go to `lds`.
template <typename FMT, bool BF16, bool HASH>
__device__ unsigned long long mx_gather_aligned(const Desc& d, char* flat_base,
                                                uint32_t s, uint32_t e,
                                                unsigned char* lds) {
  constexpr uint32_t LB = FMT::kBits;        // code bytes of 8 elements
  constexpr uint32_t CPW = 32 / FMT::kBits;  // codes per dword
  char* flat = flat_base + d.flat_off;
  unsigned long long h = 0;
  for (uint32_t i = s + threadIdx.x * LB; i < e; i += kBlockThreads * LB) {
    uint32_t valid;
    const char* src = mx_aligned_addr<BF16 ? 2 : 4>(d, i * (8 / LB), valid);
    uint32_t v[8];
    mx_load8<BF16>(src, valid, v);
    uint32_t amax = 0;
    bool nonfinite = false;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      amax = max(amax, mx_amax_of(v[k]));
      nonfinite = nonfinite || mx_nonfinite(v[k]);
    }
    // e and the unit are whole blocks: the four lanes of a block are all
    // here or all gone
    amax = max(amax, (uint32_t)__shfl_xor((int)amax, 1, 64));
    amax = max(amax, (uint32_t)__shfl_xor((int)amax, 2, 64));
    const int E = mx_block_exp<FMT>(amax);
    uint32_t X = (uint32_t)(E + 127);
    if constexpr (!FMT::kHasNan) {
      // the codes cannot say NaN, the block's scale byte does
      if (((__ballot(nonfinite) >> (threadIdx.x & 60u)) & 0xFull) != 0) X = 0xFFu;
    }
    uint32_t c[2] = {0u, 0u};
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) {
      c[k / CPW] |= mx_encode<FMT>(v[k], E) << (FMT::kBits * (k % CPW));
    }
    mx_store_lane<FMT, HASH>(flat + i, c, d.flat_off + i, h);
    if ((threadIdx.x & 3u) == 0u) {
      lds[(i - s) / FMT::kBlockBytes] = (unsigned char)X;
    }
  }
  return h;
}

// number of elements of a general-class tensor
__device__ __forceinline__ uint32_t mx_numel(const Desc& d) {
  uint32_t n = d.row_bytes;
  for (uint32_t k = 0; k < d.ndim; ++k) n *= d.sizes[k];
  return n;
}

// The general class's walk: the f32 pattern of the element at (p, col), then
// one step on in row-major order; `more` is false at the tensor's last element
template <bool BF16>
__device__ __forceinline__ uint32_t mx_walk_load(const Desc& d, const char*& p,
                                                 uint32_t& row, uint32_t& col,
                                                 bool more) {
  const char* q = p + (unsigned long long)(BF16 ? 2 : 4) * col;
  const uint32_t u = BF16 ? (uint32_t)*reinterpret_cast<const uint16_t*>(q) << 16
                          : *reinterpret_cast<const uint32_t*>(q);
  if (++col == d.row_bytes && more) {
    col = 0;
    p = d.tensor_base + row_offset(d, ++row);
  }
  return u;
}

// General gather: one lane per block, walking rows twice. The one place where
// the formats choose differently, by measurement
// (profiles/mx_codec_refactor_measurements.md): fp8 walks once and keeps the
// block's elements in registers between the amax and the encoding, which is
// 4 % faster for it on strided reads and sets the register count of both mx
// kernels; fp4 reads its elements twice.
template <typename FMT, bool BF16, bool HASH>
__device__ unsigned long long mx_gather_general(const Desc& d, char* flat_base,
                                                uint32_t s, uint32_t e,
                                                unsigned char* lds) {
  constexpr uint32_t BB = FMT::kBlockBytes;
  constexpr uint32_t CPW = 32 / FMT::kBits;  // codes per dword
  constexpr bool KEEP = FMT::kBits == 8;
  char* flat = flat_base + d.flat_off;
  const uint32_t n = mx_numel(d);
  unsigned long long h = 0;
  for (uint32_t i0 = s + threadIdx.x * BB; i0 < e; i0 += kBlockThreads * BB) {
    // the block's first element exists: nbytes is ceil(n / 32) blocks
    const uint32_t el0 = i0 * (8 / FMT::kBits);
    const uint32_t count = min(n - el0, kMxBlock);
    const uint32_t row0 = el0 / d.row_bytes;
    const uint32_t col0 = el0 - row0 * d.row_bytes;
    const char* const p0 = d.tensor_base + row_offset(d, row0);

    uint32_t row = row0, col = col0;
    const char* p = p0;
    uint32_t amax = 0;
    bool nonfinite = false;
    uint32_t v[KEEP ? kMxBlock : 1];
    if constexpr (KEEP) {
#pragma unroll
      for (uint32_t j = 0; j < kMxBlock; ++j) {
        v[j] = 0u;
        if (j < count) v[j] = mx_walk_load<BF16>(d, p, row, col, j + 1 < count);
        amax = max(amax, mx_amax_of(v[j]));
        nonfinite = nonfinite || mx_nonfinite(v[j]);
      }
    } else {
      for (uint32_t j = 0; j < count; ++j) {
        const uint32_t u = mx_walk_load<BF16>(d, p, row, col, j + 1 < count);
        amax = max(amax, mx_amax_of(u));
        nonfinite = nonfinite || mx_nonfinite(u);
      }
      row = row0, col = col0, p = p0;
    }
    const int E = mx_block_exp<FMT>(amax);

    // constant trip counts, so that `o` stays in registers
    uint4 o[BB / 16];
#pragma unroll
    for (uint32_t piece = 0; piece < BB / 16; ++piece) {
      uint32_t w[4];
#pragma unroll
      for (uint32_t q = 0; q < 4; ++q) {
        w[q] = 0;
#pragma unroll
        for (uint32_t k = 0; k < CPW; ++k) {
          const uint32_t j = (4 * piece + q) * CPW + k;
          if constexpr (KEEP) {
            w[q] |= mx_encode<FMT>(v[j], E) << (FMT::kBits * k);
          } else if (j < count) {
            const uint32_t u = mx_walk_load<BF16>(d, p, row, col, j + 1 < count);
            w[q] |= mx_encode<FMT>(u, E) << (FMT::kBits * k);
          }
        }
      }
      o[piece] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    // a block's pieces leave together: across PCIe two halves of a 32 B run
    // stored far apart in time are two partial writes
#pragma unroll
    for (uint32_t piece = 0; piece < BB / 16; ++piece) {
      *reinterpret_cast<uint4*>(flat + i0 + 16 * piece) = o[piece];
      if (HASH) h += psum_regs<16>(o[piece], d.flat_off + i0 + 16 * piece);
    }
    lds[(i0 - s) / BB] = !FMT::kHasNan && nonfinite ? 0xFFu
                                                    : (unsigned char)(E + 127);
  }
  return h;
}

// Move one unit's `count` scale bytes between LDS and the payload (TO_FLAT:
// out of LDS after the gather filled it; else into LDS before the scatter
// reads it), as 16 B pieces; only a payload's last piece is cut into
// naturally aligned 8 / 4 / 2 / 1 B ones. `payload` is 16 B aligned
// (check_descs). When HASH, returns the psum64 contribution of the bytes
// moved. Both barriers are reached by the whole workgroup: the owner, the
// cast code and the unit are uniform across it.
template <bool TO_FLAT, bool HASH>
__device__ unsigned long long mx_move_scales(char* payload, unsigned char* lds,
                                             uint32_t count,
                                             unsigned long long file_off) {
  unsigned long long h = 0;
  __syncthreads();
  const uint32_t wide = count >> 4;
  if (threadIdx.x < wide) {
    uint4* src = reinterpret_cast<uint4*>(TO_FLAT ? (char*)lds : payload);
    uint4* dst = reinterpret_cast<uint4*>(TO_FLAT ? payload : (char*)lds);
    const uint4 a = src[threadIdx.x];
    dst[threadIdx.x] = a;
    if (HASH) h += psum_regs<16>(a, file_off + 16ull * threadIdx.x);
  }
  if (threadIdx.x == 0) {
    uint32_t p = wide << 4;
#pragma unroll
    for (uint32_t w = 8; w >= 1; w >>= 1) {
      if (count - p < w) continue;
      char* src = (TO_FLAT ? (char*)lds : payload) + p;
      char* dst = (TO_FLAT ? payload : (char*)lds) + p;
      unsigned long long a;
      if (w == 8) {
        a = *reinterpret_cast<unsigned long long*>(src);
        *reinterpret_cast<unsigned long long*>(dst) = a;
      } else if (w == 4) {
        a = *reinterpret_cast<uint32_t*>(src);
        *reinterpret_cast<uint32_t*>(dst) = (uint32_t)a;
      } else if (w == 2) {
        a = *reinterpret_cast<uint16_t*>(src);
        *reinterpret_cast<uint16_t*>(dst) = (uint16_t)a;
      } else {
        a = *reinterpret_cast<unsigned char*>(src);
        *reinterpret_cast<unsigned char*>(dst) = (unsigned char)a;
      }
      if (HASH) h += psum_piece(a, file_off + p);
      p += w;
    }
  }
  __syncthreads();
  return h;
}

// One mx descriptor's work unit of the gather: codes, then the scales.
template <typename FMT, bool BF16, bool HASH>
__device__ unsigned long long mx_gather_unit(const Desc& d, char* flat_base,
                                             uint32_t s, uint32_t e,
                                             unsigned char* lds) {
  const unsigned long long h =
      d.vec == 8 ? mx_gather_aligned<FMT, BF16, HASH>(d, flat_base, s, e, lds)
                 : mx_gather_general<FMT, BF16, HASH>(d, flat_base, s, e, lds);
  const unsigned long long scales_off =
      d.flat_off + d.nbytes + s / FMT::kBlockBytes;
  return h + mx_move_scales<true, HASH>(flat_base + scales_off, lds,
                                        (e - s) / FMT::kBlockBytes, scales_off);
}

// The one place where an mx cast code becomes compile-time tags: calls
// f(format, bf16) with a format struct of mx_codec.h and whether the tensor
// side is bf16 (else f32).
template <typename F>
__device__ __forceinline__ void mx_dispatch(uint32_t cast, F&& f) {
  const bool fp4 = cast >= kCastF32toMX4;
  if (mx_elem_size(cast) == 2) {
    if (fp4) f(MxFp4E2M1{}, std::true_type{});
    else f(MxFp8E4M3{}, std::true_type{});
  } else {
    if (fp4) f(MxFp4E2M1{}, std::false_type{});
    else f(MxFp8E4M3{}, std::false_type{});
  }
}

// pack_kernel for batches that hold an mx descriptor; plain and cast
// descriptors of the same slab take pack_kernel's own routes.
template <bool HASH>
__global__ __launch_bounds__(kBlockThreads) void pack_mx_kernel(
    const Desc* __restrict__ descs, int n,
    const unsigned long long* __restrict__ wu_prefix,
    unsigned long long total_wus, char* __restrict__ flat_base,
    unsigned long long* __restrict__ hash_out) {
  __shared__ uint4 lds_scales[kMxUnitBlocks / 16];
  unsigned char* lds = reinterpret_cast<unsigned char*>(lds_scales);
  for_each_work_unit(
      descs, n, wu_prefix, total_wus,
      [&](int owner, const Desc& d, uint32_t s, uint32_t e) {
        unsigned long long h = 0;
        if (is_mx_cast(d.cast)) {
          mx_dispatch(d.cast, [&](auto fmt, auto bf16) {
            h = mx_gather_unit<decltype(fmt), decltype(bf16)::value, HASH>(
                d, flat_base, s, e, lds);
          });
        } else {
          h = pack_unit<HASH, true>(d, flat_base, s, e);
        }
        if (HASH) add_per_wave(&hash_out[owner], h);
      });
}

// the decoded element as the target stores it: an f32 pattern, or its bf16
// rounding (to nearest even) in the low half
template <typename FMT, bool BF16>
__device__ __forceinline__ uint32_t mx_out(uint32_t code, uint32_t X) {
  const uint32_t f = mx_decode<FMT>(code, X);
  return BF16 ? (f32_to_bf16_bits(f) & 0xFFFFu) : f;
}

// 8 consecutive decoded elements, as mx_out gives them, to an aligned-class
// target: 16 B stores; the ones from `valid` on do not exist
template <bool BF16>
__device__ __forceinline__ void mx_store8(char* dst, uint32_t valid,
                                          const uint32_t (&o)[8]) {
  if (valid >= 8) {
    if (BF16) {
      *reinterpret_cast<uint4*>(dst) =
          make_uint4(o[0] | (o[1] << 16), o[2] | (o[3] << 16),
                     o[4] | (o[5] << 16), o[6] | (o[7] << 16));
    } else {
      *reinterpret_cast<uint4*>(dst) = make_uint4(o[0], o[1], o[2], o[3]);
      *reinterpret_cast<uint4*>(dst + 16) = make_uint4(o[4], o[5], o[6], o[7]);
    }
  } else {
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) {
      if (k < valid) {
        if (BF16) reinterpret_cast<uint16_t*>(dst)[k] = (uint16_t)o[k];
        else reinterpret_cast<uint32_t*>(dst)[k] = o[k];
      }
    }
  }
}

// code j of the dwords c[], element 0 lowest
template <typename FMT>
__device__ __forceinline__ uint32_t mx_code_at(const uint32_t* c, uint32_t j) {
  constexpr uint32_t CPW = 32 / FMT::kBits;
  return (c[j / CPW] >> (FMT::kBits * (j % CPW))) & ((1u << FMT::kBits) - 1u);
}

// Aligned scatter of [s, e) of the codes region; the unit's scales are in
// `lds` already.
template <typename FMT, bool BF16, bool HASH>
__device__ unsigned long long mx_scatter_aligned(const Desc& d,
                                                 const char* flat_base,
                                                 uint32_t s, uint32_t e,
                                                 unsigned long long hash_off,
                                                 const unsigned char* lds) {
  constexpr uint32_t LB = FMT::kBits;  // code bytes of 8 elements
  const char* flat = flat_base + d.flat_off;
  unsigned long long h = 0;
  for (uint32_t i = s + threadIdx.x * LB; i < e; i += kBlockThreads * LB) {
    uint32_t c[2];
    mx_load_lane<FMT, HASH>(flat + i, c, hash_off + i, h);
    const uint32_t X = lds[(i - s) / FMT::kBlockBytes];
    uint32_t valid;
    char* dst = const_cast<char*>(
        mx_aligned_addr<BF16 ? 2 : 4>(d, i * (8 / LB), valid));
    uint32_t o[8];
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) {
      o[k] = mx_out<FMT, BF16>(mx_code_at<FMT>(c, k), X);
    }
    mx_store8<BF16>(dst, valid, o);
  }
  return h;
}

// General scatter: one lane per block, walking rows once.
template <typename FMT, bool BF16, bool HASH>
__device__ unsigned long long mx_scatter_general(const Desc& d,
                                                 const char* flat_base,
                                                 uint32_t s, uint32_t e,
                                                 unsigned long long hash_off,
                                                 const unsigned char* lds) {
  constexpr int TS = BF16 ? 2 : 4;
  constexpr uint32_t BB = FMT::kBlockBytes;
  constexpr uint32_t CPW = 32 / FMT::kBits;  // codes per dword
  const char* flat = flat_base + d.flat_off;
  char* base = const_cast<char*>(d.tensor_base);
  const uint32_t rb = d.row_bytes;
  const uint32_t n = mx_numel(d);
  unsigned long long h = 0;
  for (uint32_t i0 = s + threadIdx.x * BB; i0 < e; i0 += kBlockThreads * BB) {
    uint32_t c[BB / 4];
#pragma unroll
    for (uint32_t piece = 0; piece < BB / 16; ++piece) {
      const uint4 a =
          *reinterpret_cast<const uint4*>(flat + i0 + 16 * piece);
      if (HASH) h += psum_regs<16>(a, hash_off + i0 + 16 * piece);
      c[4 * piece] = a.x;
      c[4 * piece + 1] = a.y;
      c[4 * piece + 2] = a.z;
      c[4 * piece + 3] = a.w;
    }
    const uint32_t X = lds[(i0 - s) / BB];
    const uint32_t el0 = i0 * (8 / FMT::kBits);
    const uint32_t count = min(n - el0, kMxBlock);
    uint32_t row = el0 / rb;
    uint32_t col = el0 - row * rb;
    char* p = base + row_offset(d, row);
    for (uint32_t j = 0; j < count; ++j) {
      // selects, not an index: `c` stays in registers
      uint32_t w = c[0];
#pragma unroll
      for (uint32_t k = 1; k < BB / 4; ++k) {
        if (j >= k * CPW) w = c[k];
      }
      const uint32_t o = mx_out<FMT, BF16>(mx_code_at<FMT>(&w, j % CPW), X);
      char* q = p + (unsigned long long)TS * col;
      if (BF16) *reinterpret_cast<uint16_t*>(q) = (uint16_t)o;
      else *reinterpret_cast<uint32_t*>(q) = o;
      if (++col == rb && j + 1 < count) {
        col = 0;
        p = base + row_offset(d, ++row);
      }
    }
  }
  return h;
}

// One mx descriptor's work unit of the scatter: the scales, then the codes.
template <typename FMT, bool BF16, bool HASH>
__device__ unsigned long long mx_scatter_unit(const Desc& d,
                                              const char* flat_base, uint32_t s,
                                              uint32_t e,
                                              unsigned long long hash_off,
                                              unsigned char* lds) {
  const unsigned long long scales_off =
      (unsigned long long)d.nbytes + s / FMT::kBlockBytes;
  const unsigned long long h = mx_move_scales<false, HASH>(
      const_cast<char*>(flat_base) + d.flat_off + scales_off, lds,
      (e - s) / FMT::kBlockBytes, hash_off + scales_off);
  return h + (d.vec == 8 ? mx_scatter_aligned<FMT, BF16, HASH>(
                               d, flat_base, s, e, hash_off, lds)
                         : mx_scatter_general<FMT, BF16, HASH>(
                               d, flat_base, s, e, hash_off, lds));
}

// unpack_kernel for batches that hold an mx descriptor
template <bool HASH>
__global__ __launch_bounds__(kBlockThreads) void unpack_mx_kernel(
    const Desc* __restrict__ descs, int n,
    const unsigned long long* __restrict__ wu_prefix,
    unsigned long long total_wus, const char* __restrict__ flat_base,
    unsigned long long* __restrict__ hash_out,
    unsigned long long hash_byte0) {
  __shared__ uint4 lds_scales[kMxUnitBlocks / 16];
  unsigned char* lds = reinterpret_cast<unsigned char*>(lds_scales);
  for_each_work_unit(
      descs, n, wu_prefix, total_wus,
      [&](int owner, const Desc& d, uint32_t s, uint32_t e) {
        const unsigned long long ho = hash_byte0 + d.flat_off;
        unsigned long long h = 0;
        if (is_mx_cast(d.cast)) {
          mx_dispatch(d.cast, [&](auto fmt, auto bf16) {
            h = mx_scatter_unit<decltype(fmt), decltype(bf16)::value, HASH>(
                d, flat_base, s, e, ho, lds);
          });
        } else {
          h = unpack_unit<HASH, true>(d, flat_base, s, e, ho);
        }
        if (HASH) add_per_wave(&hash_out[owner], h);
      });
}

// ---------------------------------------------------------------------------
// non-finite scan: count NaN and +-Inf elements per descriptor, read-only.
// Same descriptors, driver and traversal as the gather; there is no flat
// side (flat_off is unused) and nbytes/row_bytes/vec are the tensor's own
// bytes. The element class travels in an array beside the descriptors
// (kScan* in desc_check.h), so Desc::cast stays a gather/scatter matter.
// Classification is integer arithmetic on the loaded words, like the casts:
// no dependence on the wave's float mode. The two "stored" classes count
// what the save_dtype narrowing above will write: a finite f32 at or above
// 65520 (0x477FF000) rounds to f16 inf, one at or above 0x7F7F8000 to bf16
// inf.
// ---------------------------------------------------------------------------

// Classify the elements packed in one 32-bit word. A narrower load arrives
// zero-extended, and an all-zero element is finite in every class, so the
// padding never counts. The 8- and 16-bit classes test all elements of the
// word at once: with the sign bits cleared every element is at most
// 0x7F / 0x7FFF, so adding (limit's complement) carries into the element's
// own top bit exactly when it exceeds the limit, and never into a
// neighbour.
template <uint32_t CLS>
__device__ inline void scan_word(uint32_t w, uint32_t& nan, uint32_t& inf) {
  if (CLS == kScanF32 || CLS == kScanF32asF16 || CLS == kScanF32asBF16) {
    const uint32_t a = w & 0x7FFFFFFFu;
    const uint32_t first_inf = CLS == kScanF32asF16    ? 0x477FF000u
                               : CLS == kScanF32asBF16 ? 0x7F7F8000u
                                                       : 0x7F800000u;
    nan += a > 0x7F800000u;
    inf += (a >= first_inf) & (a <= 0x7F800000u);
  } else if (CLS == kScanF16 || CLS == kScanBF16) {
    const uint32_t a = w & 0x7FFF7FFFu;
    const uint32_t gt = CLS == kScanF16 ? 0x03FF03FFu : 0x007F007Fu;
    const uint32_t ge = CLS == kScanF16 ? 0x04000400u : 0x00800080u;
    const uint32_t n = __popc((a + gt) & 0x80008000u);
    nan += n;
    inf += __popc((a + ge) & 0x80008000u) - n;
  } else if (CLS == kScanE5M2) {
    const uint32_t a = w & 0x7F7F7F7Fu;
    const uint32_t n = __popc((a + 0x03030303u) & 0x80808080u);
    nan += n;
    inf += __popc((a + 0x04040404u) & 0x80808080u) - n;
  } else if (CLS == kScanE4M3FN) {
    const uint32_t a = w & 0x7F7F7F7Fu;
    nan += __popc((a + 0x01010101u) & 0x80808080u);
  } else {  // kScanFNUZ: the whole byte equals 0x80
    const uint32_t x = w ^ 0x80808080u;
    // exact zero-byte test: top bit set where the byte of x is zero
    const uint32_t z =
        ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
    nan += __popc(z);
  }
}

__device__ inline void scan_f64(uint32_t lo, uint32_t hi, uint32_t& nan,
                                uint32_t& inf) {
  const unsigned long long a =
      (((unsigned long long)hi << 32) | lo) & 0x7FFFFFFFFFFFFFFFull;
  nan += a > 0x7FF0000000000000ull;
  inf += a == 0x7FF0000000000000ull;
}

// One naturally aligned VEC-byte load (VEC >= the element size) and the
// classification of every element in it.
template <int VEC, uint32_t CLS>
__device__ inline void scan_vec(const char* p, uint32_t& nan, uint32_t& inf) {
  if (VEC == 16) {
    const uint4 a = *reinterpret_cast<const uint4*>(p);
    if (CLS == kScanF64) {
      scan_f64(a.x, a.y, nan, inf);
      scan_f64(a.z, a.w, nan, inf);
    } else {
      scan_word<CLS>(a.x, nan, inf);
      scan_word<CLS>(a.y, nan, inf);
      scan_word<CLS>(a.z, nan, inf);
      scan_word<CLS>(a.w, nan, inf);
    }
  } else if (VEC == 8) {
    const uint2 a = *reinterpret_cast<const uint2*>(p);
    if (CLS == kScanF64) {
      scan_f64(a.x, a.y, nan, inf);
    } else {
      scan_word<CLS>(a.x, nan, inf);
      scan_word<CLS>(a.y, nan, inf);
    }
  } else if (CLS != kScanF64) {
    uint32_t w;
    if (VEC == 4) w = *reinterpret_cast<const uint32_t*>(p);
    else if (VEC == 2) w = *reinterpret_cast<const uint16_t*>(p);
    else w = *reinterpret_cast<const unsigned char*>(p);
    scan_word<CLS>(w, nan, inf);
  }
}

// Scan counterpart of gather_range: [s, e) of the tensor's own bytes for
// one work unit, loads only.
template <int VEC, uint32_t CLS>
__device__ __forceinline__ void scan_range(const Desc& d, uint32_t s,
                                           uint32_t e, uint32_t& nan,
                                           uint32_t& inf) {
  for_each_vec<VEC, 1, 4>(d, s, e, [&](unsigned long long, const char* p) {
    scan_vec<VEC, CLS>(p, nan, inf);
  });
}

// The class switch sits outside the traversal: the inner loops are
// specialised per (vec, class) and never branch per element. The host
// refuses vec below the element size, so those pairs are not instantiated.
template <uint32_t CLS>
__device__ __forceinline__ void scan_class(const Desc& d, uint32_t s,
                                           uint32_t e, uint32_t& nan,
                                           uint32_t& inf) {
  constexpr uint32_t ESZ = scan_elem_size(CLS);
  switch (d.vec) {
    case 16: scan_range<16, CLS>(d, s, e, nan, inf); break;
    case 8: scan_range<8, CLS>(d, s, e, nan, inf); break;
    case 4:
      if constexpr (ESZ <= 4) scan_range<4, CLS>(d, s, e, nan, inf);
      break;
    case 2:
      if constexpr (ESZ <= 2) scan_range<2, CLS>(d, s, e, nan, inf);
      break;
    default:
      if constexpr (ESZ <= 1) scan_range<1, CLS>(d, s, e, nan, inf);
      break;
  }
}

// counts[2*i] / counts[2*i+1]: NaN / Inf elements of descriptor i. A work
// unit holds at most 64 Ki elements, so the per-lane and per-wave counters
// fit u32; the totals are u64.
__global__ __launch_bounds__(kBlockThreads) void scan_kernel(
    const Desc* __restrict__ descs, const uint32_t* __restrict__ classes,
    int n, const unsigned long long* __restrict__ wu_prefix,
    unsigned long long total_wus, unsigned long long* __restrict__ counts) {
  for_each_work_unit(
      descs, n, wu_prefix, total_wus,
      [&](int owner, const Desc& d, uint32_t s, uint32_t e) {
        uint32_t nan = 0, inf = 0;
        switch (classes[owner]) {
          case kScanF64: scan_class<kScanF64>(d, s, e, nan, inf); break;
          case kScanF32: scan_class<kScanF32>(d, s, e, nan, inf); break;
          case kScanF16: scan_class<kScanF16>(d, s, e, nan, inf); break;
          case kScanBF16: scan_class<kScanBF16>(d, s, e, nan, inf); break;
          case kScanE5M2: scan_class<kScanE5M2>(d, s, e, nan, inf); break;
          case kScanE4M3FN: scan_class<kScanE4M3FN>(d, s, e, nan, inf); break;
          case kScanFNUZ: scan_class<kScanFNUZ>(d, s, e, nan, inf); break;
          case kScanF32asF16:
            scan_class<kScanF32asF16>(d, s, e, nan, inf);
            break;
          default: scan_class<kScanF32asBF16>(d, s, e, nan, inf); break;
        }
        add_per_wave(&counts[2 * owner], nan);
        add_per_wave(&counts[2 * owner + 1], inf);
      });
}

// ---------------------------------------------------------------------------
// fingerprint: the psum64 of each descriptor's STORED bytes in logical
// (row-major) order, as if they began at file offset flat_off, read in
// place from the strided tensor. Nothing is staged and nothing is stored
// but one u64 per descriptor. With flat_off = 0 the value is the host
// psum64 of t.contiguous()'s bytes (of t.to(stored).contiguous()'s under a
// cast code), whatever the tensor's strides: the flat index the traversal
// hands the lane operation is the byte's position in that contiguous image,
// and the contribution rule (psum_mult of the word index, narrow pieces
// shifted into their word lane) is the gather's.
//
//   - driver and traversal: for_each_work_unit and for_each_vec, like every
//     other kernel here; the gather's descriptors describe the tensor, so
//     the work split (64 KiB of stored bytes per workgroup pass, lanes
//     across a contiguous run or a wide row, one lane per narrow row) is
//     the gather's and the scan's. The grid is capped lower than theirs,
//     at 2048 workgroups (see the launcher)
//   - plain descriptors (TS = 1): one naturally aligned VEC-byte load and
//     psum_contrib of the registers it filled
//   - cast descriptors, codes 1 and 2 (TS = 2): the lane reads 2*VEC bytes
//     of f32, narrows them with cast_regs - the conversion the gather
//     stores - and hashes the packed result with psum_regs. Nothing is
//     written, so the value is the hash of what a save_dtype gather would
//     store, NaN quieting and overflow to inf included
//   - load scheduling: the kernel is a pure HBM read; per 64-bit word it
//     pays the two multiplies of splitmix64 and the one by the weight. The
//     multiplier is a function of the flat index alone, never of loaded
//     data, so it sits off the load's dependency chain; the contiguous loop
//     is unrolled by 4 (as scan_range's is), which puts four independent
//     loads in flight per lane while the multipliers of those four words
//     are computed. Each lane keeps one u64 accumulator
//   - reduction: the lane sums are carried from one work unit to the next
//     while the workgroup stays on one descriptor, and add_per_wave issues
//     one atomic per wave each time it moves on. Unlike the scan's
//     counters, which are zero on healthy state and then issue no atomic,
//     every wave here has a sum to add, and all waves of a tensor add to
//     one address: the fewer atomics, the better
//     (profiles/replicated_check_measurements.md)
//   - determinism: every step - the lane sums, the wave reduction, the
//     atomics - is wrapping u64 addition, which is associative and
//     commutative. The result is therefore bit-exact for any grid size,
//     any unroll and any order in which the atomics land. The cross-rank
//     comparison of replicated state rests on this: equal bytes give equal
//     fingerprints on every rank, always
//
// check_descs (DescKind::Fingerprint) keeps every load inside the rows the
// descriptor names and requires flat_off % vec == 0, so that no piece
// straddles a word of the hash (a 16-byte piece covers exactly two).
// ---------------------------------------------------------------------------

// Fingerprint counterpart of gather_range / cast_range: this thread's
// psum64 contribution over [s, e) of the stored bytes of one work unit.
template <int VEC, int TS>
__device__ __forceinline__ unsigned long long fingerprint_range(
    const Desc& d, uint32_t s, uint32_t e) {
  const unsigned long long off0 = d.flat_off;
  const uint32_t code = d.cast;
  unsigned long long h = 0;
  for_each_vec<VEC, TS, 4>(d, s, e, [&](unsigned long long i, const char* src) {
    if constexpr (TS == 2) {
      h += psum_regs<VEC>(cast_regs<VEC>(src, code), off0 + i);
    } else {
      h += psum_contrib<VEC>(src, off0 + i);
    }
  });
  return h;
}

// out[i]: fingerprint of descriptor i (zeroed by the launcher)
__global__ __launch_bounds__(kBlockThreads) void fingerprint_kernel(
    const Desc* __restrict__ descs, int n,
    const unsigned long long* __restrict__ wu_prefix,
    unsigned long long total_wus, unsigned long long* __restrict__ out) {
  // The lane sums are carried from one work unit to the next for as long
  // as the workgroup stays with the same descriptor (the owner is uniform
  // across the workgroup), and reduced when it moves on: a large tensor
  // costs each wave one atomic, not one per work unit.
  unsigned long long acc = 0;
  int cur = -1;
  for_each_work_unit(
      descs, n, wu_prefix, total_wus,
      [&](int owner, const Desc& d, uint32_t s, uint32_t e) {
        if (owner != cur) {
          if (cur >= 0) add_per_wave(&out[cur], acc);
          acc = 0;
          cur = owner;
        }
        unsigned long long h = 0;
        if (d.cast != kCastNone) {
          switch (d.vec) {
            case 16: h = fingerprint_range<16, 2>(d, s, e); break;
            case 8: h = fingerprint_range<8, 2>(d, s, e); break;
            case 4: h = fingerprint_range<4, 2>(d, s, e); break;
            default: h = fingerprint_range<2, 2>(d, s, e); break;
          }
        } else {
          switch (d.vec) {
            case 16: h = fingerprint_range<16, 1>(d, s, e); break;
            case 8: h = fingerprint_range<8, 1>(d, s, e); break;
            case 4: h = fingerprint_range<4, 1>(d, s, e); break;
            case 2: h = fingerprint_range<2, 1>(d, s, e); break;
            default: h = fingerprint_range<1, 1>(d, s, e); break;
          }
        }
        acc += h;
      });
  if (cur >= 0) add_per_wave(&out[cur], acc);
}

// ---------------------------------------------------------------------------
// tensor statistics: six u64 words per descriptor over its FINITE elements
// (NaN and +-Inf are skipped; counting them is the scan's job), read in
// place and read-only like the scan, with the scan's descriptors (no flat
// side, one class per descriptor beside them: f64, f32, f16, bf16):
//
//   0  n_finite                      4  sum, f64 bits
//   1  n_zero (+0 and -0)            5  sum of squares, f64 bits
//   2  minimum, as a key             (key = order-preserving u64 image of
//   3  maximum, as a key              the value widened to f64)
//
//   - widening: every class widens to f64 exactly. It is done on the bit
//     patterns (f16 -> f32 with the restore's f16_to_f32_bits, bf16 by a
//     shift, f32 -> f64 below), so f16, bf16 and f32 subnormals come out
//     exact whatever the wave's f32 denormal mode is. The f64 additions and
//     the multiply are written as __dadd_rn / __dmul_rn: never contracted
//     into an fma, so what a lane computes does not depend on how the
//     compiler schedules an instantiation. Only an f64 tensor can produce an
//     f64 subnormal operand (the square of the smallest f32 subnormal is
//     2^-298), and f64 denormals are kept by the kernel's float mode
//   - key: bits ^ (sign ? ~0 : 1 << 63). Keys compare as unsigned integers
//     the way the values compare as numbers (-0 below +0). No finite value
//     has the key 0 or ~0 (both are NaN patterns), so the launcher's initial
//     words, ~0 for the minimum and 0 for the maximum, mean "no finite
//     element" and never win against a real key
//   - words 0-3: lane registers, carried from one work unit to the next
//     while the workgroup stays on one descriptor, as the fingerprint
//     carries its sum. When it moves on: add_per_wave for the counters, a
//     wave64 shuffle min / max and ONE atomicMin / atomicMax per wave for
//     the keys. Integer min, max and addition are associative and
//     commutative: any grid and any order give the same words
//   - words 4-5 are floating-point sums, and f64 addition is not
//     associative: a float atomic, or carrying, would make the result
//     depend on the grid size and on which workgroup lands first, and ranks
//     compare and merge these values. So they are reduced in two stages of
//     fixed shape. Stage one, per 64 KiB work unit: a lane adds its elements
//     in traversal order (a function of the descriptor, the unit and the
//     lane alone); a fixed wave64 shuffle tree follows; the four wave
//     results go through LDS and thread 0 adds them in wave order and stores
//     the pair at partials[2 * global work-unit number]. Stage two,
//     stats_finish_kernel, one wave per descriptor on the same stream: lane
//     l adds partials l, l + 64, ... of the descriptor's work units in that
//     order, then the same tree. The grid size, the order of workgroups and
//     the descriptor's place in the batch do not enter anywhere
//   - LDS: 64 bytes (4 waves x 2 doubles). It is the first use of LDS among
//     these kernels because it is the first reduction here that has to
//     cross waves in a FIXED order; everything else reduces with atomics,
//     whose order is free because integer addition does not care
//   - loads: the widest the descriptor allows, UNROLL 4 on the contiguous
//     loop like the scan; every element of a loaded word is classified
//     and accumulated without a branch (a non-finite element contributes
//     0.0 to the sums and the neutral key to min and max)
// ---------------------------------------------------------------------------

// finite f32 pattern -> the f64 pattern of the same value
__device__ __host__ inline unsigned long long f32_to_f64_bits(uint32_t u) {
  const unsigned long long sign = (unsigned long long)(u & 0x80000000u) << 32;
  const uint32_t exp = (u >> 23) & 0xFFu;
  const uint32_t mant = u & 0x007FFFFFu;
  if (exp != 0u) {
    // rebias 127 -> 1023; 23 mantissa bits move to the top of 52
    return sign | ((unsigned long long)(exp + 896u) << 52) |
           ((unsigned long long)mant << 29);
  }
  if (mant == 0u) return sign;  // +-0
  // subnormal: mant * 2^-149. Shift the leading one up to bit 23 (the
  // implicit bit); each position shifted lowers the exponent from 2^-126
  const uint32_t shift = (uint32_t)__builtin_clz(mant) - 8u;  // 1..23
  return sign | ((unsigned long long)(897u - shift) << 52) |
         ((unsigned long long)((mant << shift) & 0x007FFFFFu) << 29);
}

// What one lane keeps. The counters, like the scan's, fit u32 within a work
// unit; the kernel adds them into u64 ones it carries.
struct StatsLane {
  uint32_t n_finite = 0, n_zero = 0;
  unsigned long long kmin = ~0ull, kmax = 0ull;
  double sum = 0.0, sumsq = 0.0;
};

// one element, given as an f64 pattern and whether it is finite
__device__ __forceinline__ void stats_elem(unsigned long long b, bool finite,
                                           StatsLane& a) {
  const unsigned long long key =
      b ^ ((b >> 63) ? ~0ull : 0x8000000000000000ull);
  const unsigned long long klo = finite ? key : ~0ull;
  const unsigned long long khi = finite ? key : 0ull;
  a.kmin = klo < a.kmin ? klo : a.kmin;
  a.kmax = khi > a.kmax ? khi : a.kmax;
  a.n_finite += finite;
  a.n_zero += finite & ((b << 1) == 0ull);  // +0 and -0
  const double x = finite ? __longlong_as_double((long long)b) : 0.0;
  a.sum = __dadd_rn(a.sum, x);
  a.sumsq = __dadd_rn(a.sumsq, __dmul_rn(x, x));
}

__device__ __forceinline__ void stats_f32(uint32_t u, StatsLane& a) {
  const bool finite = (u & 0x7FFFFFFFu) < 0x7F800000u;
  // the widening of a non-finite pattern is some pattern nobody looks at
  stats_elem(f32_to_f64_bits(u), finite, a);
}

__device__ __forceinline__ void stats_f64(uint32_t lo, uint32_t hi,
                                          StatsLane& a) {
  const unsigned long long b = ((unsigned long long)hi << 32) | lo;
  const bool finite = (b & 0x7FFFFFFFFFFFFFFFull) < 0x7FF0000000000000ull;
  stats_elem(b, finite, a);
}

// the elements of one loaded 32-bit word (one for f32, two for f16 / bf16)
template <uint32_t CLS>
__device__ __forceinline__ void stats_word(uint32_t w, StatsLane& a) {
  if (CLS == kScanF32) {
    stats_f32(w, a);
  } else if (CLS == kScanBF16) {
    stats_f32(w << 16, a);
    stats_f32(w & 0xFFFF0000u, a);
  } else {  // kScanF16; inf and NaN stay inf and NaN in f32
    stats_f32(f16_to_f32_bits(w & 0xFFFFu), a);
    stats_f32(f16_to_f32_bits(w >> 16), a);
  }
}

// One naturally aligned VEC-byte load (VEC >= the element size) and every
// element in it. Unlike the scan, a zero element counts here, so the one
// load that is narrower than a word (a single 16-bit element) is not
// padded.
template <int VEC, uint32_t CLS>
__device__ __forceinline__ void stats_vec(const char* p, StatsLane& a) {
  if (VEC == 16) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    if (CLS == kScanF64) {
      stats_f64(v.x, v.y, a);
      stats_f64(v.z, v.w, a);
    } else {
      stats_word<CLS>(v.x, a);
      stats_word<CLS>(v.y, a);
      stats_word<CLS>(v.z, a);
      stats_word<CLS>(v.w, a);
    }
  } else if (VEC == 8) {
    const uint2 v = *reinterpret_cast<const uint2*>(p);
    if (CLS == kScanF64) {
      stats_f64(v.x, v.y, a);
    } else {
      stats_word<CLS>(v.x, a);
      stats_word<CLS>(v.y, a);
    }
  } else if (VEC == 4) {
    if (CLS != kScanF64) stats_word<CLS>(*reinterpret_cast<const uint32_t*>(p), a);
  } else if (VEC == 2) {
    const uint32_t h = *reinterpret_cast<const uint16_t*>(p);
    if (CLS == kScanBF16) stats_f32(h << 16, a);
    else if (CLS == kScanF16) stats_f32(f16_to_f32_bits(h), a);
  }
}

// The class switch sits outside the traversal, as in scan_class; the host
// refuses vec below the element size, so those pairs are not instantiated.
template <uint32_t CLS>
__device__ __forceinline__ void stats_class(const Desc& d, uint32_t s,
                                            uint32_t e, StatsLane& a) {
  constexpr uint32_t ESZ = scan_elem_size(CLS);
  auto range = [&](auto vec) {
    constexpr int VEC = decltype(vec)::value;
    for_each_vec<VEC, 1, 4>(d, s, e, [&](unsigned long long, const char* p) {
      stats_vec<VEC, CLS>(p, a);
    });
  };
  switch (d.vec) {
    case 16: range(std::integral_constant<int, 16>{}); break;
    case 8: range(std::integral_constant<int, 8>{}); break;
    case 4:
      if constexpr (ESZ <= 4) range(std::integral_constant<int, 4>{});
      break;
    default:
      if constexpr (ESZ <= 2) range(std::integral_constant<int, 2>{});
      break;
  }
}

// the fixed wave64 tree of the two-stage sums: lane 0 ends with the result
__device__ __forceinline__ double wave_sum_fixed(double v) {
  for (int delta = 32; delta > 0; delta >>= 1) {
    v = __dadd_rn(v, __shfl_down(v, delta, 64));
  }
  return v;
}

// Stage one of a pair of two-stage f64 sums, shared by the stats and the
// compare kernel: the fixed tree per wave, the four wave results through
// `wave_sums` in wave order, and the unit's pair stored at partials[2 * wu].
// Every thread of the workgroup must call it (two barriers).
__device__ __forceinline__ void store_unit_sums(
    double (*wave_sums)[2], double* __restrict__ partials,
    unsigned long long wu, double a, double b) {
  const double wa = wave_sum_fixed(a);
  const double wb = wave_sum_fixed(b);
  if ((threadIdx.x & 63) == 0) {
    wave_sums[threadIdx.x >> 6][0] = wa;
    wave_sums[threadIdx.x >> 6][1] = wb;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double ua = wave_sums[0][0], ub = wave_sums[0][1];
    for (int w = 1; w < kBlockThreads / 64; ++w) {
      ua = __dadd_rn(ua, wave_sums[w][0]);
      ub = __dadd_rn(ub, wave_sums[w][1]);
    }
    partials[2 * wu] = ua;
    partials[2 * wu + 1] = ub;
  }
  __syncthreads();  // before the next unit's waves overwrite the LDS
}

// Stage two, for one wave: lane l adds the pairs of work units first + l,
// first + l + 64, ... below `end` in that order, the fixed tree follows,
// and lane 0 holds the two sums.
__device__ __forceinline__ void finish_unit_sums(
    const double* __restrict__ partials, unsigned long long first,
    unsigned long long end, double& a, double& b) {
  a = 0.0;
  b = 0.0;
  for (unsigned long long wu = first + threadIdx.x; wu < end; wu += 64) {
    a = __dadd_rn(a, partials[2 * wu]);
    b = __dadd_rn(b, partials[2 * wu + 1]);
  }
  a = wave_sum_fixed(a);
  b = wave_sum_fixed(b);
}

// wave64 min / max of the keys and one atomic per wave; none for a wave
// that saw no finite element
__device__ __forceinline__ void minmax_per_wave(unsigned long long* out,
                                                unsigned long long kmin,
                                                unsigned long long kmax) {
  for (int delta = 32; delta > 0; delta >>= 1) {
    const unsigned long long lo = __shfl_down(kmin, delta, 64);
    const unsigned long long hi = __shfl_down(kmax, delta, 64);
    kmin = lo < kmin ? lo : kmin;
    kmax = hi > kmax ? hi : kmax;
  }
  if ((threadIdx.x & 63) == 0 && kmax != 0ull) {
    atomicMin(&out[2], kmin);
    atomicMax(&out[3], kmax);
  }
}

// out[6*i ..]: the six words of descriptor i; the launcher sets word 2 to
// ~0 and the rest to zero. Words 4-5 are left to stats_finish_kernel;
// partials[2*wu], partials[2*wu + 1]: sum and sum of squares of work unit
// wu, every one of which is written exactly once.
__global__ __launch_bounds__(kBlockThreads) void stats_kernel(
    const Desc* __restrict__ descs, const uint32_t* __restrict__ classes,
    int n, const unsigned long long* __restrict__ wu_prefix,
    unsigned long long total_wus, unsigned long long* __restrict__ out,
    double* __restrict__ partials) {
  __shared__ double wave_sums[kBlockThreads / 64][2];
  unsigned long long n_finite = 0, n_zero = 0;
  unsigned long long kmin = ~0ull, kmax = 0ull;
  int cur = -1;
  auto flush = [&]() {
    add_per_wave(&out[6 * cur], n_finite);
    add_per_wave(&out[6 * cur + 1], n_zero);
    minmax_per_wave(&out[6 * cur], kmin, kmax);
  };
  for_each_work_unit(
      descs, n, wu_prefix, total_wus,
      [&](int owner, const Desc& d, uint32_t s, uint32_t e) {
        if (owner != cur) {
          if (cur >= 0) flush();
          n_finite = n_zero = 0;
          kmin = ~0ull;
          kmax = 0ull;
          cur = owner;
        }
        StatsLane a;
        a.kmin = kmin;
        a.kmax = kmax;
        switch (classes[owner]) {
          case kScanF64: stats_class<kScanF64>(d, s, e, a); break;
          case kScanF32: stats_class<kScanF32>(d, s, e, a); break;
          case kScanF16: stats_class<kScanF16>(d, s, e, a); break;
          default: stats_class<kScanBF16>(d, s, e, a); break;
        }
        n_finite += a.n_finite;
        n_zero += a.n_zero;
        kmin = a.kmin;
        kmax = a.kmax;
        // stage one of the sums. The owner, and so the path to here, is
        // uniform across the workgroup: every thread reaches both barriers
        store_unit_sums(wave_sums, partials,
                        wu_prefix[owner] + s / kWorkUnitBytes, a.sum, a.sumsq);
      });
  if (cur >= 0) flush();
}

// Stage two: one wave per descriptor. Lane l adds partials l, l + 64, ...
// of the descriptor's work units in that order, the fixed tree follows, and
// lane 0 stores words 4 and 5.
__global__ __launch_bounds__(64) void stats_finish_kernel(
    int n, const unsigned long long* __restrict__ wu_prefix,
    const double* __restrict__ partials, unsigned long long* __restrict__ out) {
  const int i = blockIdx.x;
  if (i >= n) return;
  double s, q;
  finish_unit_sums(partials, wu_prefix[i], wu_prefix[i + 1], s, q);
  if (threadIdx.x == 0) {
    out[6 * i + 4] = (unsigned long long)__double_as_longlong(s);
    out[6 * i + 5] = (unsigned long long)__double_as_longlong(q);
  }
}

// ---------------------------------------------------------------------------
// exponent histogram: kHistWords u64 words per descriptor, read in place and
// read-only over the stats kernel's descriptors and classes (f64, f32, f16,
// bf16):
//
//   0      n_zero: +0 and -0
//   1      n_negative: finite, non-zero, sign bit set
//   2      n_nonfinite: NaN and +-Inf
//   3 + k  finite non-zero elements with floor(log2|x|) == k - 149,
//          k = 0..276: every f32 binade, subnormal ones included, which
//          covers f16 and bf16; an f64 element outside lands in the end bin
//
// so that words[0] + words[2] + sum(words[3:]) is the element count.
//
//   - classification is integer arithmetic on the bit patterns: a normal
//     element's bin is its exponent field plus a constant, a subnormal's the
//     position of its leading mantissa bit (one clz). Zero and non-finite are
//     two selects on the same masked value, so every element ends as ONE word
//     index and one counter increment; nothing depends on the float mode
//   - the counters live in LDS, u32, in kHistCopies = 32 private copies per
//     workgroup; a lane counts in copy (lane & 31). Trained weights sit in a
//     few adjacent binades, so with one copy most of a wave's 64 lanes would
//     meet on one address in one instruction and the LDS would take them one
//     after the other; with 32 copies at most the two lanes l and l + 32 of a
//     wave can, whatever the data
//   - layout: word-major, copies interleaved, counter (w, c) at
//     bins[w * 32 + c]. The bank of an LDS dword is its index modulo the
//     number of banks, so with 32 banks a lane's bank is (w * 32 + c) % 32 =
//     lane & 31 for EVERY word w: the 32 lanes of a half wave always fall in
//     32 different banks, and bin values cannot make them collide. (With 64
//     banks the bank is 32 * (w & 1) + c, still distinct within a half wave.)
//     The copy-major layout bins[c * 280 + w] has no such property: 280 = 8
//     mod 32, so for one shared bin the copies c and c + 4 share a bank, an
//     8-way conflict on exactly the hostile input; a padded stride of 281
//     fixes one shared bin but not neighbouring bins (copy c, bin w + 1 meets
//     copy c + 1, bin w)
//   - size: 280 * 32 * 4 = 35840 bytes per workgroup, so 4 workgroups (16
//     waves, 4 per SIMD) fit the 160 KiB of a CU. 64 copies would leave 2
//     workgroups, too few waves to cover HBM latency, for a gain only where
//     lanes l and l + 32 are issued together; 16 copies would double the
//     lanes per address. With 32 the kernel's time does not depend on the
//     values at all, against 5.4x between the friendliest and the most
//     hostile input with one copy (profiles/tensor_hist_measurements.md)
//   - n_negative is not a second LDS increment per element (half of all
//     elements are negative): a lane keeps it in a register and adds it to
//     word 1 of its own copy when the counters are flushed
//   - the counters are carried from one work unit to the next while the
//     workgroup stays on one descriptor. When the owner changes, and at the
//     end: barrier; thread t sums word t, t + 256, ... over the 32 copies,
//     clears what it read, and adds a non-zero total to out[280 * owner + w]
//     with one u64 atomic; barrier. The owner is a function of blockIdx and
//     the tables alone, so it is uniform across the workgroup and so is every
//     path to a barrier
//   - a u32 counter cannot wrap: check_descs keeps a descriptor under 4 GiB,
//     an element has at least 2 bytes, so one descriptor has fewer than 2^31
//     elements, and the counters are flushed per descriptor at the latest.
//     The same bound holds for a lane's n_negative register
//   - every word is an integer count added with integer atomics: any grid,
//     any batch order and any max_grid give the same bits
// ---------------------------------------------------------------------------

constexpr uint32_t kHistWords = 280;
constexpr uint32_t kHistBins = kHistWords - 3;  // k = 0..276
constexpr uint32_t kHistCopies = 32;

// what one lane keeps: its copy of the counters (word w at mine[w * 32]) and
// its negative elements since the last flush
struct HistLane {
  uint32_t* mine;
  uint32_t n_negative;
};

// One element, as its pattern without the sign (`a`), the first non-finite
// pattern of its format and its word among the bins.
__device__ __forceinline__ void hist_elem(uint32_t a, uint32_t sign,
                                          uint32_t first_nonfinite,
                                          uint32_t bin_word, HistLane& h) {
  const bool finite = a < first_nonfinite;
  uint32_t w = finite ? bin_word : 2u;
  w = a == 0u ? 0u : w;
  h.n_negative += sign & (uint32_t)(finite & (a != 0u));
  atomicAdd(&h.mine[w * kHistCopies], 1u);  // ds_add_u32, no return value
}

// f32 pattern: exponent field E != 0 is binade E - 127, word 3 + E + 22; a
// subnormal m * 2^-149 with its leading bit at position p = 31 - clz(m) is
// binade p - 149, word 3 + p. (__clz(0) is 32; zero is selected away.)
__device__ __forceinline__ void hist_f32(uint32_t u, HistLane& h) {
  const uint32_t a = u & 0x7FFFFFFFu;
  const uint32_t exp = a >> 23;
  const uint32_t word = exp != 0u ? exp + 25u : 34u - (uint32_t)__clz((int)a);
  hist_elem(a, u >> 31, 0x7F800000u, word, h);
}

// f16 pattern: E != 0 is binade E - 15, word 3 + E + 134; a subnormal
// m * 2^-24 is binade p - 24, word 3 + p + 125
__device__ __forceinline__ void hist_f16(uint32_t u, HistLane& h) {
  const uint32_t a = u & 0x7FFFu;
  const uint32_t exp = a >> 10;
  const uint32_t word =
      exp != 0u ? exp + 137u : 159u - (uint32_t)__clz((int)a);
  hist_elem(a, (u >> 15) & 1u, 0x7C00u, word, h);
}

// f64 pattern: binade E - 1023, or p - 1074 for a subnormal, clamped to the
// f32 range -149..127
__device__ __forceinline__ void hist_f64(uint32_t lo, uint32_t hi,
                                         HistLane& h) {
  const uint32_t ahi = hi & 0x7FFFFFFFu;
  const unsigned long long a = ((unsigned long long)ahi << 32) | lo;
  const int exp = (int)(ahi >> 20);
  const int binade = exp != 0 ? exp - 1023 : 63 - __clzll((long long)a) - 1074;
  const int k = min(max(binade + 149, 0), (int)kHistBins - 1);
  // the classification needs "zero", "finite" and nothing else of the low
  // word: fold it into one bit below the high word's pattern
  const uint32_t a32 = ahi | (uint32_t)(lo != 0u);
  // Inf is 0x7FF00000 with lo == 0, every NaN is above or has lo != 0
  hist_elem(a32, hi >> 31, 0x7FF00000u, 3u + (uint32_t)k, h);
}

// the elements of one loaded 32-bit word (one for f32, two for f16 / bf16;
// a bf16 pattern is the top half of the f32 pattern of the same value)
template <uint32_t CLS>
__device__ __forceinline__ void hist_word(uint32_t w, HistLane& h) {
  if (CLS == kScanF32) {
    hist_f32(w, h);
  } else if (CLS == kScanBF16) {
    hist_f32(w << 16, h);
    hist_f32(w & 0xFFFF0000u, h);
  } else {  // kScanF16
    hist_f16(w & 0xFFFFu, h);
    hist_f16(w >> 16, h);
  }
}

// One naturally aligned VEC-byte load (VEC >= the element size) and every
// element in it. A zero element counts, so the one load narrower than a word
// (a single 16-bit element) is not padded, as in stats_vec.
template <int VEC, uint32_t CLS>
__device__ __forceinline__ void hist_vec(const char* p, HistLane& h) {
  if (VEC == 16) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    if (CLS == kScanF64) {
      hist_f64(v.x, v.y, h);
      hist_f64(v.z, v.w, h);
    } else {
      hist_word<CLS>(v.x, h);
      hist_word<CLS>(v.y, h);
      hist_word<CLS>(v.z, h);
      hist_word<CLS>(v.w, h);
    }
  } else if (VEC == 8) {
    const uint2 v = *reinterpret_cast<const uint2*>(p);
    if (CLS == kScanF64) {
      hist_f64(v.x, v.y, h);
    } else {
      hist_word<CLS>(v.x, h);
      hist_word<CLS>(v.y, h);
    }
  } else if (VEC == 4) {
    if (CLS != kScanF64) hist_word<CLS>(*reinterpret_cast<const uint32_t*>(p), h);
  } else if (VEC == 2) {
    const uint32_t e = *reinterpret_cast<const uint16_t*>(p);
    if (CLS == kScanBF16) hist_f32(e << 16, h);
    else if (CLS == kScanF16) hist_f16(e, h);
  }
}

// The class switch sits outside the traversal, as in stats_class; the host
// refuses vec below the element size, so those pairs are not instantiated.
template <uint32_t CLS>
__device__ __forceinline__ void hist_class(const Desc& d, uint32_t s,
                                           uint32_t e, HistLane& h) {
  constexpr uint32_t ESZ = scan_elem_size(CLS);
  auto range = [&](auto vec) {
    constexpr int VEC = decltype(vec)::value;
    for_each_vec<VEC, 1, 4>(d, s, e, [&](unsigned long long, const char* p) {
      hist_vec<VEC, CLS>(p, h);
    });
  };
  switch (d.vec) {
    case 16: range(std::integral_constant<int, 16>{}); break;
    case 8: range(std::integral_constant<int, 8>{}); break;
    case 4:
      if constexpr (ESZ <= 4) range(std::integral_constant<int, 4>{});
      break;
    default:
      if constexpr (ESZ <= 2) range(std::integral_constant<int, 2>{});
      break;
  }
}

// Reduce the copies into out[0 .. kHistWords) and leave them cleared. Every
// thread of the workgroup must call it (two barriers). Thread t owns words
// t, t + 256, ...: it reads and clears the 32 copies of a word starting at
// copy (t & 31), so that the lanes of a half wave, which hold 32 consecutive
// words, read 32 different banks in every step and not one.
__device__ __forceinline__ void hist_flush(uint32_t* bins, HistLane& h,
                                           unsigned long long* out) {
  if (h.n_negative != 0u) atomicAdd(&h.mine[1u * kHistCopies], h.n_negative);
  h.n_negative = 0u;
  __syncthreads();  // every lane's increments are in
  for (uint32_t w = threadIdx.x; w < kHistWords; w += kBlockThreads) {
    unsigned long long total = 0;
#pragma unroll 8
    for (uint32_t i = 0; i < kHistCopies; ++i) {
      uint32_t* p = &bins[w * kHistCopies + ((w + i) & (kHistCopies - 1u))];
      total += *p;
      *p = 0u;
    }
    if (total != 0ull) atomicAdd(&out[w], total);
  }
  __syncthreads();  // cleared before anybody counts again
}

// out[280 * i ..]: the words of descriptor i, zeroed by the launcher.
__global__ __launch_bounds__(kBlockThreads) void hist_kernel(
    const Desc* __restrict__ descs, const uint32_t* __restrict__ classes,
    int n, const unsigned long long* __restrict__ wu_prefix,
    unsigned long long total_wus, unsigned long long* __restrict__ out) {
  __shared__ uint32_t bins[kHistWords * kHistCopies];
  for (uint32_t i = threadIdx.x; i < kHistWords * kHistCopies;
       i += kBlockThreads) {
    bins[i] = 0u;
  }
  __syncthreads();
  HistLane h{&bins[threadIdx.x & (kHistCopies - 1u)], 0u};
  int cur = -1;
  for_each_work_unit(
      descs, n, wu_prefix, total_wus,
      [&](int owner, const Desc& d, uint32_t s, uint32_t e) {
        if (owner != cur) {
          // uniform: owner and cur are the same in every thread
          if (cur >= 0) hist_flush(bins, h, &out[(size_t)kHistWords * cur]);
          cur = owner;
        }
        switch (classes[owner]) {
          case kScanF64: hist_class<kScanF64>(d, s, e, h); break;
          case kScanF32: hist_class<kScanF32>(d, s, e, h); break;
          case kScanF16: hist_class<kScanF16>(d, s, e, h); break;
          default: hist_class<kScanBF16>(d, s, e, h); break;
        }
      });
  if (cur >= 0) hist_flush(bins, h, &out[(size_t)kHistWords * cur]);
}

// ---------------------------------------------------------------------------
// compare: a stored payload against live tensors, element by element, with
// BOTH sides read-only. The flat side is the payload where the storage read
// put it (the consumer's pinned host block, read once over PCIe, or a device
// buffer); the tensor side is the live strided tensor. Unpack-style
// descriptors (flat_off inside the payload, vec that divides the flat
// address too, cast codes 0, 3 and 4) and one kCmp* class per descriptor
// beside them. Six u64 words per descriptor:
//
//   0  n, elements compared (host)   3  max |v - s|, f64 bits
//   1  n_diff, bit patterns differ   4  sum (v - s)^2, f64 bits
//   2  n_nonfinite_diff              5  sum s^2, f64 bits
//
// s is the stored element brought to the live dtype (bf16/f16 stored against
// f32 live widen with the restore's bit arithmetic), v the live one; both
// widen to f64 exactly, on the bit patterns, as in the stats kernel. Words
// 3-5 are over the pairs with both sides finite; a differing pair with a
// non-finite side counts in word 2. The raw classes (integers, bool, fp8,
// complex: compared bitwise per element) fill words 0 and 1 only.
//
//   - work split: the stats kernel's. 64 KiB of STORED bytes per workgroup
//     pass, lanes across a contiguous run or a wide row, one lane per
//     narrow row; TS = 2 for the widen classes
//   - lane operation: one naturally aligned VEC-byte load of the flat side
//     and the matching load(s) of the tensor side into registers, the stored
//     words brought to the live format, and a whole-word comparison first.
//     A vector whose words all agree only adds to word 5; otherwise every
//     element is classified and accumulated without a branch (a non-finite
//     pair contributes 0.0 to the sums and 0 to the maximum). Both paths add
//     the same terms in the same order: d = v - v is +0.0 and its square
//     leaves a non-negative sum as it is. A load narrower than a word is
//     zero-padded on both sides, and a pair of zeros changes no word
//   - words 1-3 are carried from one work unit to the next while the
//     workgroup stays on one descriptor, then add_per_wave for the counters
//     and a wave64 shuffle max with ONE atomicMax per wave for word 3: the
//     u64 pattern of a non-negative f64 is monotone in its value
//   - words 4-5 go through the fixed-shape two-stage reduction of the stats
//     kernel (store_unit_sums, then compare_finish_kernel on the same
//     stream): no word depends on the grid, the order of workgroups or the
//     descriptor's place in the batch
// ---------------------------------------------------------------------------

struct CmpLane {
  uint32_t n_diff = 0, n_nonfinite = 0;
  unsigned long long kmax = 0ull;
  double sq = 0.0, ref = 0.0;
};

// one pair with equal bits: only the reference sum moves
__device__ __forceinline__ void cmp_same(unsigned long long sb, bool finite,
                                         CmpLane& a) {
  const double s = finite ? __longlong_as_double((long long)sb) : 0.0;
  a.ref = __dadd_rn(a.ref, __dmul_rn(s, s));
}

// one pair, given as f64 patterns, whether each side is finite and whether
// the native bit patterns differ
__device__ __forceinline__ void cmp_pair(unsigned long long sb, bool s_fin,
                                         unsigned long long vb, bool v_fin,
                                         bool differ, CmpLane& a) {
  const bool both = s_fin & v_fin;
  a.n_diff += differ;
  a.n_nonfinite += differ & !both;
  const double s = both ? __longlong_as_double((long long)sb) : 0.0;
  const double v = both ? __longlong_as_double((long long)vb) : 0.0;
  const double d = __dsub_rn(v, s);
  const unsigned long long k =
      (unsigned long long)__double_as_longlong(d) & 0x7FFFFFFFFFFFFFFFull;
  a.kmax = k > a.kmax ? k : a.kmax;
  a.sq = __dadd_rn(a.sq, __dmul_rn(d, d));
  a.ref = __dadd_rn(a.ref, __dmul_rn(s, s));
}

__device__ __forceinline__ bool f32_finite(uint32_t u) {
  return (u & 0x7FFFFFFFu) < 0x7F800000u;
}

// V bytes (16/8/4/2/1, naturally aligned) into w[0..3], zero-padded
template <int V>
__device__ __forceinline__ void load_words(const char* p, uint32_t* w) {
  w[0] = w[1] = w[2] = w[3] = 0u;
  if (V == 16) {
    const uint4 a = *reinterpret_cast<const uint4*>(p);
    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
  } else if (V == 8) {
    const uint2 a = *reinterpret_cast<const uint2*>(p);
    w[0] = a.x; w[1] = a.y;
  } else if (V == 4) {
    w[0] = *reinterpret_cast<const uint32_t*>(p);
  } else if (V == 2) {
    w[0] = *reinterpret_cast<const uint16_t*>(p);
  } else {
    w[0] = *reinterpret_cast<const unsigned char*>(p);
  }
}

// the elements of one word of the live format: stored word s, live word t.
// SAME: the caller found every word of the vector equal
template <uint32_t CLS, bool SAME>
__device__ __forceinline__ void cmp_word(uint32_t s, uint32_t t, CmpLane& a) {
  if (CLS == kScanF32) {
    if (SAME) {
      cmp_same(f32_to_f64_bits(s), f32_finite(s), a);
    } else {
      cmp_pair(f32_to_f64_bits(s), f32_finite(s), f32_to_f64_bits(t),
               f32_finite(t), s != t, a);
    }
  } else {  // two 16-bit elements; inf and NaN stay inf and NaN in f32
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint32_t sh = (s >> (16 * h)) & 0xFFFFu;
      const uint32_t th = (t >> (16 * h)) & 0xFFFFu;
      const uint32_t s32 =
          CLS == kScanBF16 ? bf16_to_f32_bits(sh) : f16_to_f32_bits(sh);
      if (SAME) {
        cmp_same(f32_to_f64_bits(s32), f32_finite(s32), a);
      } else {
        const uint32_t t32 =
            CLS == kScanBF16 ? bf16_to_f32_bits(th) : f16_to_f32_bits(th);
        cmp_pair(f32_to_f64_bits(s32), f32_finite(s32), f32_to_f64_bits(t32),
                 f32_finite(t32), sh != th, a);
      }
    }
  }
}

template <bool SAME>
__device__ __forceinline__ void cmp_f64(uint32_t slo, uint32_t shi,
                                        uint32_t tlo, uint32_t thi,
                                        CmpLane& a) {
  const unsigned long long sb = ((unsigned long long)shi << 32) | slo;
  const unsigned long long tb = ((unsigned long long)thi << 32) | tlo;
  const bool s_fin = (sb & 0x7FFFFFFFFFFFFFFFull) < 0x7FF0000000000000ull;
  if (SAME) {
    cmp_same(sb, s_fin, a);
  } else {
    const bool t_fin = (tb & 0x7FFFFFFFFFFFFFFFull) < 0x7FF0000000000000ull;
    cmp_pair(sb, s_fin, tb, t_fin, sb != tb, a);
  }
}

// number of elements of ESZ bytes that are non-zero in the NW words of x
// (the XOR of the two sides)
template <uint32_t ESZ, int NW>
__device__ __forceinline__ uint32_t raw_diff_count(const uint32_t* x) {
  uint32_t n = 0;
  if (ESZ == 1 || ESZ == 2) {
    // top bit of each element set where the element is non-zero
    const uint32_t low = ESZ == 1 ? 0x7F7F7F7Fu : 0x7FFF7FFFu;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      n += __popc((((x[i] & low) + low) | x[i]) & ~low);
    }
  } else {
    constexpr int WPE = ESZ / 4;  // words per element
#pragma unroll
    for (int i = 0; i < NW; i += WPE) {
      uint32_t any = 0;
#pragma unroll
      for (int k = 0; k < WPE; ++k) any |= x[i + k];
      n += any != 0u;
    }
  }
  return n;
}

// One flat vector of VEC stored bytes against the tensor bytes it stands
// for (VEC of them, 2*VEC under a widen class).
template <int VEC, uint32_t CLS>
__device__ __forceinline__ void compare_vec(const char* flat, const char* ten,
                                            CmpLane& a) {
  constexpr bool WIDEN = CLS == kCmpBF16toF32 || CLS == kCmpF16toF32;
  constexpr int FW = VEC >= 4 ? VEC / 4 : 1;  // flat words
  constexpr int NW = WIDEN ? 2 * FW : FW;     // words of the live format
  uint32_t f[4], s[8], t[8];
  load_words<VEC>(flat, f);
  if constexpr (WIDEN) {
    // the restore's widening, on the registers just loaded
#pragma unroll
    for (int i = 0; i < FW; ++i) {
      const uint2 p = widen_pair(f[i], cmp_cast_code(CLS));
      s[2 * i] = p.x;
      s[2 * i + 1] = p.y;
    }
    if constexpr (VEC == 16) {
      load_words<16>(ten, t);
      load_words<16>(ten + 16, t + 4);
    } else {
      load_words<2 * VEC>(ten, t);
    }
  } else {
#pragma unroll
    for (int i = 0; i < FW; ++i) s[i] = f[i];
    load_words<VEC>(ten, t);
  }
  uint32_t x[NW];
  uint32_t any = 0;
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    x[i] = s[i] ^ t[i];
    any |= x[i];
  }
  if constexpr (CLS >= kCmpRaw1 && CLS <= kCmpRaw16) {
    a.n_diff += raw_diff_count<cmp_elem_size(CLS), NW>(x);
  } else if constexpr (CLS == kScanF64) {
    if (any == 0u) {
#pragma unroll
      for (int i = 0; i < NW; i += 2) cmp_f64<true>(s[i], s[i + 1], 0, 0, a);
    } else {
#pragma unroll
      for (int i = 0; i < NW; i += 2) {
        cmp_f64<false>(s[i], s[i + 1], t[i], t[i + 1], a);
      }
    }
  } else {
    constexpr uint32_t LIVE = WIDEN ? kScanF32 : CLS;
    if (any == 0u) {
#pragma unroll
      for (int i = 0; i < NW; ++i) cmp_word<LIVE, true>(s[i], 0, a);
    } else {
#pragma unroll
      for (int i = 0; i < NW; ++i) cmp_word<LIVE, false>(s[i], t[i], a);
    }
  }
}

// The class switch sits outside the traversal, as in scan_class; the host
// refuses vec below the stored element size, so those pairs are not
// instantiated.
template <uint32_t CLS>
__device__ __forceinline__ void compare_class(const Desc& d, const char* flat,
                                              uint32_t s, uint32_t e,
                                              CmpLane& a) {
  constexpr uint32_t ESZ = cmp_elem_size(CLS);
  constexpr int TS = cmp_cast_code(CLS) != kCastNone ? 2 : 1;
  auto range = [&](auto vec) {
    constexpr int VEC = decltype(vec)::value;
    for_each_vec<VEC, TS>(d, s, e, [&](unsigned long long i, const char* p) {
      compare_vec<VEC, CLS>(flat + i, p, a);
    });
  };
  switch (d.vec) {
    case 16: range(std::integral_constant<int, 16>{}); break;
    case 8:
      if constexpr (ESZ <= 8) range(std::integral_constant<int, 8>{});
      break;
    case 4:
      if constexpr (ESZ <= 4) range(std::integral_constant<int, 4>{});
      break;
    case 2:
      if constexpr (ESZ <= 2) range(std::integral_constant<int, 2>{});
      break;
    default:
      if constexpr (ESZ <= 1) range(std::integral_constant<int, 1>{});
      break;
  }
}

// out[6*i ..]: the six words of descriptor i, zeroed by the launcher; word 0
// is the host's and words 4-5 are left to compare_finish_kernel.
// partials[2*wu], partials[2*wu + 1]: the two sums of work unit wu, every
// one of which is written exactly once.
__global__ __launch_bounds__(kBlockThreads) void compare_kernel(
    const Desc* __restrict__ descs, const uint32_t* __restrict__ classes,
    int n, const unsigned long long* __restrict__ wu_prefix,
    unsigned long long total_wus, const char* __restrict__ flat_base,
    unsigned long long* __restrict__ out, double* __restrict__ partials) {
  __shared__ double wave_sums[kBlockThreads / 64][2];
  unsigned long long n_diff = 0, n_nonfinite = 0, kmax = 0;
  int cur = -1;
  auto flush = [&]() {
    add_per_wave(&out[6 * cur + 1], n_diff);
    add_per_wave(&out[6 * cur + 2], n_nonfinite);
    for (int delta = 32; delta > 0; delta >>= 1) {
      const unsigned long long o = __shfl_down(kmax, delta, 64);
      kmax = o > kmax ? o : kmax;
    }
    if ((threadIdx.x & 63) == 0 && kmax != 0ull) {
      atomicMax(&out[6 * cur + 3], kmax);
    }
  };
  for_each_work_unit(
      descs, n, wu_prefix, total_wus,
      [&](int owner, const Desc& d, uint32_t s, uint32_t e) {
        if (owner != cur) {
          if (cur >= 0) flush();
          n_diff = n_nonfinite = kmax = 0;
          cur = owner;
        }
        CmpLane a;
        a.kmax = kmax;
        const char* flat = flat_base + d.flat_off;
        switch (classes[owner]) {
          case kScanF64: compare_class<kScanF64>(d, flat, s, e, a); break;
          case kScanF32: compare_class<kScanF32>(d, flat, s, e, a); break;
          case kScanF16: compare_class<kScanF16>(d, flat, s, e, a); break;
          case kScanBF16: compare_class<kScanBF16>(d, flat, s, e, a); break;
          case kCmpRaw1: compare_class<kCmpRaw1>(d, flat, s, e, a); break;
          case kCmpRaw2: compare_class<kCmpRaw2>(d, flat, s, e, a); break;
          case kCmpRaw4: compare_class<kCmpRaw4>(d, flat, s, e, a); break;
          case kCmpRaw8: compare_class<kCmpRaw8>(d, flat, s, e, a); break;
          case kCmpRaw16: compare_class<kCmpRaw16>(d, flat, s, e, a); break;
          case kCmpBF16toF32:
            compare_class<kCmpBF16toF32>(d, flat, s, e, a);
            break;
          default: compare_class<kCmpF16toF32>(d, flat, s, e, a); break;
        }
        n_diff += a.n_diff;
        n_nonfinite += a.n_nonfinite;
        kmax = a.kmax;
        // the owner, and so the path to here, is uniform across the
        // workgroup: every thread reaches both barriers
        store_unit_sums(wave_sums, partials,
                        wu_prefix[owner] + s / kWorkUnitBytes, a.sq, a.ref);
      });
  if (cur >= 0) flush();
}

// Stage two of words 4-5: one wave per descriptor.
__global__ __launch_bounds__(64) void compare_finish_kernel(
    int n, const unsigned long long* __restrict__ wu_prefix,
    const double* __restrict__ partials, unsigned long long* __restrict__ out) {
  const int i = blockIdx.x;
  if (i >= n) return;
  double sq, ref;
  finish_unit_sums(partials, wu_prefix[i], wu_prefix[i + 1], sq, ref);
  if (threadIdx.x == 0) {
    out[6 * i + 4] = (unsigned long long)__double_as_longlong(sq);
    out[6 * i + 5] = (unsigned long long)__double_as_longlong(ref);
  }
}

// ---------------------------------------------------------------------------
// host-side op management
// ---------------------------------------------------------------------------

// The HIP half of a launch-table ring (table_ring.h has the policy): slot
// i is host + i * slot_bytes, dev + i * slot_bytes and ev[i].
struct HipTableRing {
  TableRing policy{kTableRingSlots, kTableRingSlotBytes};
  char* host = nullptr;  // pinned
  char* dev = nullptr;
  hipEvent_t ev[kTableRingSlots] = {};

  void allocate() {
    const size_t bytes = policy.slots() * policy.slot_bytes();
    HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&host), bytes,
                            hipHostMallocDefault));
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&dev), bytes));
    for (hipEvent_t& e : ev) {
      HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
  }

  // whatever allocate() got as far as creating; only for a context whose
  // set-up failed, a finished one lives as long as the process
  void release() {
    for (hipEvent_t& e : ev) {
      if (e != nullptr) (void)hipEventDestroy(e);
      e = nullptr;
    }
    if (dev != nullptr) (void)hipFree(dev);
    if (host != nullptr) (void)hipHostFree(host);
    dev = host = nullptr;
  }
};

// Lives for the life of the process once created: streams and rings are
// allocated once per device.
struct DeviceCtx {
  hipStream_t d2h_stream = nullptr;
  hipStream_t h2d_stream = nullptr;
  hipStream_t verify_stream = nullptr;  // lazily created (psum64_dev)
  HipTableRing d2h_ring;
  HipTableRing h2d_ring;
};

struct Op {
  hipEvent_t ev = nullptr;
  int device = 0;
};

// g_mu guards the three maps below and nothing else; the launch entry
// points run without the GIL, so several threads get here at once
std::mutex g_mu;
std::unordered_map<int, std::unique_ptr<DeviceCtx>> g_ctx;
std::unordered_map<long long, Op> g_ops;
long long g_next_handle = 1;

DeviceCtx& get_ctx(int device) {
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_ctx.find(device);
  if (it == g_ctx.end()) {
    HIP_CHECK(hipSetDevice(device));
    auto ctx = std::make_unique<DeviceCtx>();
    try {
      HIP_CHECK(
          hipStreamCreateWithFlags(&ctx->d2h_stream, hipStreamNonBlocking));
      HIP_CHECK(
          hipStreamCreateWithFlags(&ctx->h2d_stream, hipStreamNonBlocking));
      ctx->d2h_ring.allocate();
      ctx->h2d_ring.allocate();
    } catch (...) {
      // nothing of a half-built context stays behind: the next call starts
      // from scratch
      ctx->d2h_ring.release();
      ctx->h2d_ring.release();
      if (ctx->d2h_stream != nullptr) (void)hipStreamDestroy(ctx->d2h_stream);
      if (ctx->h2d_stream != nullptr) (void)hipStreamDestroy(ctx->h2d_stream);
      throw;
    }
    it = g_ctx.emplace(device, std::move(ctx)).first;
  }
  return *it->second;
}

long long register_op(hipEvent_t ev, int device) {
  std::lock_guard<std::mutex> lk(g_mu);
  long long h = g_next_handle++;
  Op op;
  op.ev = ev;
  op.device = device;
  g_ops.emplace(h, op);
  return h;
}

void chain_after(hipStream_t side, uintptr_t producer_stream, int device) {
  // make the side stream wait for work already enqueued on the producer's
  // stream (the training step that materialized the tensors)
  hipEvent_t dep;
  HIP_CHECK(hipEventCreateWithFlags(&dep, hipEventDisableTiming));
  hipError_t e =
      hipEventRecord(dep, reinterpret_cast<hipStream_t>(producer_stream));
  if (e == hipSuccess) {
    e = hipStreamWaitEvent(side, dep, 0);
  }
  (void)hipEventDestroy(dep);  // stream holds its own reference
  if (e != hipSuccess) {
    throw std::runtime_error(std::string("HIP error chaining streams: ") +
                             hipGetErrorString(e));
  }
}

// The environment is read with the GIL held (os.environ writes hold it
// too), before an entry point releases it.
std::string env_or_empty(const char* name) {
  const char* v = getenv(name);
  return v ? std::string(v) : std::string();
}

// Bring `tables` to the device and call enqueue_kernel(device copy) behind
// the upload on `stream`: through a slot of `ring` (nothing waits for the
// stream), or, for a table larger than a slot, through an allocation of its
// own and a copy that does wait.
template <typename Enqueue>
void enqueue_with_tables(HipTableRing& ring, hipStream_t stream,
                         const LaunchTables& tables, Enqueue enqueue_kernel) {
  const size_t table_bytes = tables.host.size();
  const size_t slot_bytes = ring.policy.slot_bytes();
  const bool ringed = ring.policy.launch(
      table_bytes,
      [&](int slot) { HIP_CHECK(hipEventSynchronize(ring.ev[slot])); },
      [&](int slot) {
        char* h_tables = ring.host + slot * slot_bytes;
        char* d_tables = ring.dev + slot * slot_bytes;
        std::memcpy(h_tables, tables.host.data(), table_bytes);
        try {
          // out of pinned memory: enqueued, not waited for
          HIP_CHECK(hipMemcpyAsync(d_tables, h_tables, table_bytes,
                                   hipMemcpyHostToDevice, stream));
          enqueue_kernel(d_tables);
          HIP_CHECK(hipEventRecord(ring.ev[slot], stream));
        } catch (...) {
          // the slot goes back unrecorded: nothing may still read it
          (void)hipStreamSynchronize(stream);
          throw;
        }
      });
  if (!ringed) {
    // A table larger than a slot (a slab of hundreds of members): a device
    // allocation of its own and a copy out of pageable memory, which waits
    // for the stream. The synchronise makes that explicit, so the host
    // image may go out of scope whatever the runtime did with it.
    void* scratch = nullptr;
    HIP_CHECK(hipMallocAsync(&scratch, table_bytes, stream));
    hipError_t err = hipMemcpyAsync(scratch, tables.host.data(), table_bytes,
                                    hipMemcpyHostToDevice, stream);
    const hipError_t sync_err = hipStreamSynchronize(stream);
    if (err == hipSuccess) err = sync_err;
    if (err == hipSuccess) {
      try {
        enqueue_kernel(scratch);
      } catch (...) {
        (void)hipFreeAsync(scratch, stream);
        throw;
      }
    }
    const hipError_t free_err = hipFreeAsync(scratch, stream);
    if (err == hipSuccess) err = free_err;
    HIP_CHECK(err);
  }
}

// One launcher for the three copy entry points. `kind` picks the rules
// check_descs applies and the kernel family: Gather runs pack_kernel on
// the D2H side stream, Scatter and Unpack run unpack_kernel on the H2D
// one (Scatter never casts or hashes). Called without the GIL, from any
// number of threads: nothing here waits for work queued on the stream,
// except for a ring slot that is still in use sixteen launches later and
// for a table too large for a slot.
long long launch_pack(const std::vector<unsigned long long>& flat, int n,
                      DescKind kind, uintptr_t slab_ptr, uintptr_t pinned_ptr,
                      unsigned long long total_bytes, uintptr_t producer_stream,
                      int device, const std::string& grid_env,
                      uintptr_t hash_out_ptr = 0,
                      unsigned long long hash_byte0 = 0) {
  // everything is refused here, before the GPU is touched
  const std::vector<Desc> descs = parse_descs(flat, n);
  const FlatSide flat_side{slab_ptr, pinned_ptr, total_bytes, hash_byte0};
  check_descs(descs, kind, &flat_side);
  const bool gather = kind == DescKind::Gather;
  bool any_cast = false, any_mx = false;
  for (const Desc& d : descs) {
    any_cast = any_cast || d.cast != kCastNone;
    any_mx = any_mx || is_mx_cast(d.cast);
  }

  HIP_CHECK(hipSetDevice(device));
  DeviceCtx& ctx = get_ctx(device);
  hipStream_t stream = gather ? ctx.d2h_stream : ctx.h2d_stream;

  const std::vector<unsigned long long> wu_prefix = wu_prefix_of(descs);
  const unsigned long long total_wus = wu_prefix[n];

  // flat side: device slab if provided, else the pinned host buffer
  // (device-addressable) for direct PCIe writes/reads
  char* flat_base;
  if (slab_ptr != 0) {
    flat_base = reinterpret_cast<char*>(slab_ptr);
  } else {
    void* dev_ptr = nullptr;
    hipError_t err = hipHostGetDevicePointer(
        &dev_ptr, reinterpret_cast<void*>(pinned_ptr), 0);
    flat_base = reinterpret_cast<char*>(
        err == hipSuccess && dev_ptr ? dev_ptr
                                     : reinterpret_cast<void*>(pinned_ptr));
  }

  chain_after(stream, producer_stream, device);

  // Grid cap. Direct mode is PCIe-bound: 128 workgroups already sustain
  // the measured ~51 GB/s host-link ceiling (grid sweep, profiles/), so a
  // small grid leaves the CUs to overlapped training compute. Slab mode
  // gathers at HBM speed and wants the chip filled (all 8 XCDs). The
  // restore kernel's reads of pinned memory behave the same way: 128-256
  // workgroups reach the link rate, 1024+ lose a few percent.
  const bool direct_mode = (slab_ptr == 0);
  const unsigned int grid =
      grid_for(total_wus, direct_mode ? 256ull : 16384ull,
               grid_env.empty() ? nullptr : grid_env.c_str());
  unsigned long long* hash_out =
      reinterpret_cast<unsigned long long*>(hash_out_ptr);
  const bool hash = hash_out != nullptr;

  // descriptors + prefix sums: one host image, one copy
  const LaunchTables tables(descs, wu_prefix);

  // everything that follows the table upload on the stream, up to and
  // including the kernel that reads the tables at `d_tables`
  auto enqueue_kernel = [&](const void* d_tables) {
    const Desc* d_descs = tables.descs(d_tables);
    const unsigned long long* d_prefix = tables.prefix(d_tables);
    if (!gather && slab_ptr != 0) {
      // restore via slab: H2D copy first, then scatter out of the slab
      HIP_CHECK(hipMemcpyAsync(reinterpret_cast<void*>(slab_ptr),
                               reinterpret_cast<void*>(pinned_ptr),
                               total_bytes, hipMemcpyHostToDevice, stream));
    }
    if (gather) {
      auto kernel = any_mx     ? (hash ? pack_mx_kernel<true>
                                       : pack_mx_kernel<false>)
                    : any_cast ? (hash ? pack_kernel<true, true>
                                       : pack_kernel<false, true>)
                               : (hash ? pack_kernel<true, false>
                                       : pack_kernel<false, false>);
      hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlockThreads), 0, stream,
                         d_descs, n, d_prefix, total_wus, flat_base, hash_out);
    } else {
      auto kernel = any_mx     ? (hash ? unpack_mx_kernel<true>
                                       : unpack_mx_kernel<false>)
                    : any_cast ? (hash ? unpack_kernel<true, true>
                                       : unpack_kernel<false, true>)
                               : (hash ? unpack_kernel<true, false>
                                       : unpack_kernel<false, false>);
      hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlockThreads), 0, stream,
                         d_descs, n, d_prefix, total_wus,
                         static_cast<const char*>(flat_base), hash_out,
                         hash_byte0);
    }
    HIP_CHECK(hipGetLastError());
  };

  enqueue_with_tables(gather ? ctx.d2h_ring : ctx.h2d_ring, stream, tables,
                      enqueue_kernel);

  if (gather && slab_ptr != 0) {
    // slab mode: one SDMA copy moves the packed slab to pinned host memory
    HIP_CHECK(hipMemcpyAsync(reinterpret_cast<void*>(pinned_ptr),
                             reinterpret_cast<void*>(slab_ptr), total_bytes,
                             hipMemcpyDeviceToHost, stream));
  }

  hipEvent_t ev;
  HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  const hipError_t rec_err = hipEventRecord(ev, stream);
  if (rec_err != hipSuccess) {
    (void)hipEventDestroy(ev);
    HIP_CHECK(rec_err);
  }
  return register_op(ev, device);
}

// The blocking launch of the entry points that read tensors in place and
// bring a few words per descriptor back (scan_nonfinite,
// fingerprint_tensors). Called with the GIL held, after everything that
// needs it (argument conversion, the environment); releases it for all
// GPU work. Runs on the D2H side stream, after the producer's. One device
// allocation holds `tables` and `n_results` zeroed u64 behind them;
// `launch(d_tables, d_results, stream)` enqueues the kernel. A HIP error
// is thrown with `what` in front. With `init` (n_results words) the results
// start from those values and not from zero; `scratch_bytes` more bytes of
// the same allocation, uninitialised, follow the results at
// d_results + n_results and never come back to the host.
template <typename Launch>
std::vector<unsigned long long> read_launch(
    const LaunchTables& tables, size_t n_results, uintptr_t producer_stream,
    int device, const char* what, Launch launch,
    const std::vector<unsigned long long>* init = nullptr,
    size_t scratch_bytes = 0) {
  std::vector<unsigned long long> results =
      init != nullptr ? *init : std::vector<unsigned long long>(n_results, 0);
  const size_t table_bytes = tables.host.size();
  const size_t result_bytes = sizeof(unsigned long long) * n_results;

  py::gil_scoped_release release;
  HIP_CHECK(hipSetDevice(device));
  DeviceCtx& ctx = get_ctx(device);
  hipStream_t stream = ctx.d2h_stream;
  chain_after(stream, producer_stream, device);

  void* scratch = nullptr;
  HIP_CHECK(hipMallocAsync(&scratch,
                           table_bytes + result_bytes + scratch_bytes, stream));
  unsigned long long* d_results = reinterpret_cast<unsigned long long*>(
      static_cast<char*>(scratch) + table_bytes);

  // enqueue everything, then synchronise whatever happened: the host
  // buffers (`tables`, `results`) must outlive the copies that read and
  // write them
  hipError_t err =
      init != nullptr
          ? hipMemcpyAsync(d_results, results.data(), result_bytes,
                           hipMemcpyHostToDevice, stream)
          : hipMemsetAsync(d_results, 0, result_bytes, stream);
  if (err == hipSuccess) {
    err = hipMemcpyAsync(scratch, tables.host.data(), table_bytes,
                         hipMemcpyHostToDevice, stream);
  }
  if (err == hipSuccess) {
    launch(scratch, d_results, stream);
    err = hipGetLastError();
  }
  if (err == hipSuccess) {
    err = hipMemcpyAsync(results.data(), d_results, result_bytes,
                         hipMemcpyDeviceToHost, stream);
  }
  (void)hipFreeAsync(scratch, stream);
  const hipError_t sync_err = hipStreamSynchronize(stream);
  if (err == hipSuccess) err = sync_err;
  if (err != hipSuccess) {
    throw std::runtime_error(std::string(what) + hipGetErrorString(err));
  }
  return results;
}
}  // namespace

// ---------------------------------------------------------------------------
// python API
// ---------------------------------------------------------------------------

static long long d2h_copy(uintptr_t src, uintptr_t dst_pinned,
                          unsigned long long nbytes, uintptr_t producer_stream,
                          int device) {
  py::gil_scoped_release release;
  HIP_CHECK(hipSetDevice(device));
  DeviceCtx& ctx = get_ctx(device);
  chain_after(ctx.d2h_stream, producer_stream, device);
  HIP_CHECK(hipMemcpyAsync(reinterpret_cast<void*>(dst_pinned),
                           reinterpret_cast<void*>(src), nbytes,
                           hipMemcpyDeviceToHost, ctx.d2h_stream));
  hipEvent_t ev;
  HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  const hipError_t rec_err = hipEventRecord(ev, ctx.d2h_stream);
  if (rec_err != hipSuccess) {
    (void)hipEventDestroy(ev);
    HIP_CHECK(rec_err);
  }
  return register_op(ev, device);
}

// The three launch entry points: arguments are converted and the
// environment read with the GIL held, everything else runs without it. A
// refusal or a HIP error is a C++ exception; the GIL is taken back while
// it unwinds, before pybind11 turns it into the Python one.
static long long pack_d2h(const std::vector<unsigned long long>& flat, int n,
                          uintptr_t slab_ptr, uintptr_t pinned_ptr,
                          unsigned long long total_bytes,
                          uintptr_t producer_stream, int device,
                          uintptr_t hash_out_ptr = 0) {
  const std::string grid_env = env_or_empty("TSAMD_PACK_GRID");
  py::gil_scoped_release release;
  return launch_pack(flat, n, DescKind::Gather, slab_ptr, pinned_ptr,
                     total_bytes, producer_stream, device, grid_env,
                     hash_out_ptr);
}

static long long scatter_h2d(const std::vector<unsigned long long>& flat, int n,
                             uintptr_t slab_ptr, uintptr_t pinned_ptr,
                             unsigned long long total_bytes,
                             uintptr_t producer_stream, int device) {
  const std::string grid_env = env_or_empty("TSAMD_PACK_GRID");
  py::gil_scoped_release release;
  return launch_pack(flat, n, DescKind::Scatter, slab_ptr, pinned_ptr,
                     total_bytes, producer_stream, device, grid_env);
}

static long long unpack_h2d(const std::vector<unsigned long long>& flat,
                            int n, uintptr_t slab_ptr, uintptr_t pinned_ptr,
                            unsigned long long total_bytes,
                            uintptr_t producer_stream, int device,
                            uintptr_t hash_out_ptr = 0,
                            unsigned long long hash_byte0 = 0) {
  const std::string grid_env = env_or_empty("TSAMD_PACK_GRID");
  py::gil_scoped_release release;
  return launch_pack(flat, n, DescKind::Unpack, slab_ptr, pinned_ptr,
                     total_bytes, producer_stream, device, grid_env,
                     hash_out_ptr, hash_byte0);
}

// ---------------------------------------------------------------------------
// device-side psum64 of a flat contiguous buffer (restore verification at
// HBM speed: CPU psum64 runs at a few GB/s per thread and would bottleneck
// a 50 GB/s warm restore; this kernel reads the just-H2D'd bytes once).
// byte0 = file byte offset of base[0]; must be 8-aligned.
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(kBlockThreads) void psum_flat_kernel(
    const char* base, unsigned long long nbytes, unsigned long long byte0,
    unsigned long long* out) {
  unsigned long long acc = 0;
  unsigned long long tid =
      (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long nthreads = (unsigned long long)gridDim.x * blockDim.x;
  unsigned long long nwords = nbytes >> 3;
  unsigned long long w0 = byte0 >> 3;
  const unsigned long long* words =
      reinterpret_cast<const unsigned long long*>(base);
  for (unsigned long long w = tid; w < nwords; w += nthreads) {
    acc += words[w] * psum_mult(w0 + w);
  }
  if (tid == 0) {
    // tail (< 8 bytes): lane-shifted into its word, like the CPU verifier
    for (unsigned long long b = nwords << 3; b < nbytes; ++b) {
      unsigned long long v = (unsigned char)base[b];
      acc += (v << (8 * ((byte0 + b) & 7))) * psum_mult((byte0 + b) >> 3);
    }
  }
  __shared__ unsigned long long sh[kBlockThreads];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int s = kBlockThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    atomicAdd(out, sh[0]);
  }
}

static unsigned long long psum64_dev(uintptr_t ptr, unsigned long long nbytes,
                                     unsigned long long byte0,
                                     uintptr_t producer_stream, int device) {
  if (byte0 % 8 != 0) {
    throw std::runtime_error("psum64_dev: byte0 must be 8-aligned");
  }
  if (ptr % 8 != 0) {
    throw std::runtime_error("psum64_dev: buffer must be 8-aligned");
  }
  HIP_CHECK(hipSetDevice(device));
  // The caller guarantees the bytes are already materialized (the H2D
  // copy that produced them was synchronous), so NO dependency on any
  // other stream is needed. A dedicated non-blocking stream keeps the
  // final sync scoped to this ~0.1 ms reduction alone — syncing the
  // caller's (legacy default) stream instead convoyed on every other
  // consumer thread's queued work and cost a 13x restore slowdown.
  (void)producer_stream;
  hipStream_t stream;
  {
    DeviceCtx& ctx = get_ctx(device);
    std::lock_guard<std::mutex> lk(g_mu);
    if (ctx.verify_stream == nullptr) {
      HIP_CHECK(hipStreamCreateWithFlags(&ctx.verify_stream,
                                         hipStreamNonBlocking));
    }
    stream = ctx.verify_stream;
  }
  unsigned long long* out = nullptr;
  HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&out), 8, stream));
  HIP_CHECK(hipMemsetAsync(out, 0, 8, stream));
  // HBM-bound reduction: 2048 workgroups fill all 8 XCDs with slack
  unsigned int grid = 2048;
  if (nbytes < (1u << 22)) grid = 64;
  hipLaunchKernelGGL(psum_flat_kernel, dim3(grid), dim3(kBlockThreads), 0,
                     stream, reinterpret_cast<const char*>(ptr), nbytes,
                     byte0, out);
  HIP_CHECK(hipGetLastError());
  unsigned long long host_out = 0;
  HIP_CHECK(hipMemcpyAsync(&host_out, out, 8, hipMemcpyDeviceToHost, stream));
  HIP_CHECK(hipFreeAsync(out, stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  return host_out;
}

// ---------------------------------------------------------------------------
// non-finite scan of N strided device tensors in one launch (blocking).
// `flat` holds gather-style descriptor rows (cast 0, flat_off ignored),
// `classes` one kScan* code per descriptor. Returns 2*n counts: NaN then
// Inf elements of each descriptor.
// ---------------------------------------------------------------------------

static std::vector<unsigned long long> scan_nonfinite(
    const std::vector<unsigned long long>& flat,
    const std::vector<uint32_t>& classes, int n, uintptr_t producer_stream,
    int device) {
  // refused before the GPU is touched: every vector load the kernel will
  // make is naturally aligned, covers whole elements and stays inside the
  // rows the descriptor names
  const std::vector<Desc> descs = parse_descs(flat, n);
  check_descs(descs, DescKind::Scan, nullptr, &classes);
  const size_t n_counts = 2 * (size_t)n;

  const std::vector<unsigned long long> wu_prefix = wu_prefix_of(descs);
  const unsigned long long total_wus = wu_prefix[n];
  if (total_wus == 0) return std::vector<unsigned long long>(n_counts, 0);

  // descriptors | prefix sums | classes
  const LaunchTables tables(descs, wu_prefix, classes.data(),
                            sizeof(uint32_t) * n);

  // HBM-bound read: fill the chip like the slab-mode gather does
  const unsigned int grid =
      grid_for(total_wus, 16384ull, getenv("TSAMD_PACK_GRID"));

  return read_launch(
      tables, n_counts, producer_stream, device, "scan_nonfinite: ",
      [&](const void* d_tables, unsigned long long* d_counts,
          hipStream_t stream) {
        hipLaunchKernelGGL(
            scan_kernel, dim3(grid), dim3(kBlockThreads), 0, stream,
            tables.descs(d_tables),
            static_cast<const uint32_t*>(tables.extra(d_tables)), n,
            tables.prefix(d_tables), total_wus, d_counts);
      });
}

// ---------------------------------------------------------------------------
// fingerprints of N strided device tensors in one launch (blocking).
// `flat` holds gather-style descriptor rows (cast codes 0..2); flat_off is
// the file offset the descriptor's first stored byte is hashed at. Returns
// one psum64 per descriptor.
// ---------------------------------------------------------------------------

static std::vector<unsigned long long> fingerprint_tensors(
    const std::vector<unsigned long long>& flat, int n,
    uintptr_t producer_stream, int device) {
  // refused before the GPU is touched
  const std::vector<Desc> descs = parse_descs(flat, n);
  check_descs(descs, DescKind::Fingerprint);

  const std::vector<unsigned long long> wu_prefix = wu_prefix_of(descs);
  const unsigned long long total_wus = wu_prefix[n];
  if (total_wus == 0) return std::vector<unsigned long long>((size_t)n, 0);

  // descriptors | prefix sums
  const LaunchTables tables(descs, wu_prefix);

  // HBM-bound read. 2048 workgroups fill all 8 XCDs and keep a workgroup
  // on one large tensor for many work units, so that its sums are carried
  // and not added atomically; many small tensors are indifferent to the
  // cap (grid sweep in profiles/replicated_check_measurements.md)
  const unsigned int grid =
      grid_for(total_wus, 2048ull, getenv("TSAMD_PACK_GRID"));

  return read_launch(
      tables, (size_t)n, producer_stream, device, "fingerprint_tensors: ",
      [&](const void* d_tables, unsigned long long* d_sums,
          hipStream_t stream) {
        hipLaunchKernelGGL(fingerprint_kernel, dim3(grid),
                           dim3(kBlockThreads), 0, stream,
                           tables.descs(d_tables), n, tables.prefix(d_tables),
                           total_wus, d_sums);
      });
}

// ---------------------------------------------------------------------------
// value statistics of N strided device tensors (blocking): one launch of
// stats_kernel and one of stats_finish_kernel. `flat` holds scan-style
// descriptor rows (cast 0, flat_off ignored), `classes` one of the first
// four kScan* codes per descriptor. Returns 6*n words (see stats_kernel);
// a descriptor without finite elements keeps 0, 0, ~0, 0, +0.0, +0.0.
// `max_grid` > 0 bounds the workgroups of the first kernel below the cap: a
// save beside heavy training may want fewer CUs taken, and no word depends
// on it.
// ---------------------------------------------------------------------------

static std::vector<unsigned long long> tensor_stats(
    const std::vector<unsigned long long>& flat, int n,
    const std::vector<uint32_t>& classes, int device,
    uintptr_t producer_stream, unsigned int max_grid) {
  // refused before the GPU is touched, under the scan's rules
  const std::vector<Desc> descs = parse_descs(flat, n);
  check_descs(descs, DescKind::Stats, nullptr, &classes);

  std::vector<unsigned long long> init(6 * (size_t)n, 0);
  for (size_t i = 0; i < (size_t)n; ++i) init[6 * i + 2] = ~0ull;

  const std::vector<unsigned long long> wu_prefix = wu_prefix_of(descs);
  const unsigned long long total_wus = wu_prefix[n];
  if (total_wus == 0) return init;

  // descriptors | prefix sums | classes
  const LaunchTables tables(descs, wu_prefix, classes.data(),
                            sizeof(uint32_t) * n);

  // An HBM read with f64 work behind every element. 2048 workgroups put
  // eight on each of the 256 CUs, and keep a workgroup on one large tensor
  // for many work units, so that words 0-3 are carried and cost one round
  // of atomics per tensor, not one per unit. TSAMD_PACK_GRID replaces the
  // cap only when the caller names no bound of its own.
  constexpr unsigned long long kStatsGridCap = 2048;
  const unsigned int grid =
      max_grid > 0
          ? grid_for(total_wus,
                     max_grid < kStatsGridCap ? max_grid : kStatsGridCap,
                     nullptr)
          : grid_for(total_wus, kStatsGridCap, getenv("TSAMD_PACK_GRID"));

  return read_launch(
      tables, init.size(), producer_stream, device, "tensor_stats: ",
      [&](const void* d_tables, unsigned long long* d_out,
          hipStream_t stream) {
        // the partial sums of stage one: two doubles per work unit, behind
        // the results in the same allocation
        double* d_partials = reinterpret_cast<double*>(d_out + init.size());
        hipLaunchKernelGGL(
            stats_kernel, dim3(grid), dim3(kBlockThreads), 0, stream,
            tables.descs(d_tables),
            static_cast<const uint32_t*>(tables.extra(d_tables)), n,
            tables.prefix(d_tables), total_wus, d_out, d_partials);
        hipLaunchKernelGGL(stats_finish_kernel, dim3((unsigned int)n),
                           dim3(64), 0, stream, n, tables.prefix(d_tables),
                           static_cast<const double*>(d_partials), d_out);
      },
      &init, (size_t)total_wus * 2 * sizeof(double));
}

// ---------------------------------------------------------------------------
// exponent histograms of N strided device tensors (blocking): one launch of
// hist_kernel. `flat` and `classes` are tensor_stats' and are validated
// under its rules (DescKind::Stats: no rule differs, so a refusal reads
// "tensor_stats: ..."). Returns 280*n words (see hist_kernel), all zero for a
// descriptor without elements. `max_grid` > 0 bounds the workgroups below
// the cap; no word depends on it.
// ---------------------------------------------------------------------------

static std::vector<unsigned long long> tensor_hist(
    const std::vector<unsigned long long>& flat, int n,
    const std::vector<uint32_t>& classes, int device,
    uintptr_t producer_stream, unsigned int max_grid) {
  const std::vector<Desc> descs = parse_descs(flat, n);
  check_descs(descs, DescKind::Stats, nullptr, &classes);

  const size_t n_results = (size_t)kHistWords * (size_t)n;
  const std::vector<unsigned long long> wu_prefix = wu_prefix_of(descs);
  const unsigned long long total_wus = wu_prefix[n];
  if (total_wus == 0) return std::vector<unsigned long long>(n_results, 0);

  // descriptors | prefix sums | classes
  const LaunchTables tables(descs, wu_prefix, classes.data(),
                            sizeof(uint32_t) * n);

  // 35 KiB of LDS per workgroup lets four be resident on each of the 256
  // CUs: 1024 workgroups fill the device exactly once. More would only
  // queue behind them, and each workgroup pays for its counters per
  // descriptor it visits: a clear and a reduction of 8960 LDS words and up
  // to 280 global atomics. With the cap at one resident round a workgroup
  // stays on a large tensor for as many work units as possible and the
  // global atomics per tensor are bounded by 1024 * (occupied bins).
  // TSAMD_PACK_GRID replaces the cap only when the caller names no bound.
  constexpr unsigned long long kHistGridCap = 1024;
  const unsigned int grid =
      max_grid > 0
          ? grid_for(total_wus,
                     max_grid < kHistGridCap ? max_grid : kHistGridCap,
                     nullptr)
          : grid_for(total_wus, kHistGridCap, getenv("TSAMD_PACK_GRID"));

  return read_launch(
      tables, n_results, producer_stream, device, "tensor_hist: ",
      [&](const void* d_tables, unsigned long long* d_out,
          hipStream_t stream) {
        hipLaunchKernelGGL(
            hist_kernel, dim3(grid), dim3(kBlockThreads), 0, stream,
            tables.descs(d_tables),
            static_cast<const uint32_t*>(tables.extra(d_tables)), n,
            tables.prefix(d_tables), total_wus, d_out);
      });
}

// ---------------------------------------------------------------------------
// a stored payload against N live strided device tensors (blocking): one
// launch of compare_kernel and one of compare_finish_kernel for all the
// members of one read. `flat` holds unpack-style descriptor rows (flat_off
// inside the payload, cast codes 0, 3, 4), `classes` one kCmp* code per
// descriptor; the payload is `total_bytes` at `flat_ptr`: pinned host
// memory, read in place over PCIe, when `flat_on_host`, else device memory.
// Runs on the H2D side stream behind the producer's, tables through that
// stream's ring like a restore scatter. Returns 6*n words (see
// compare_kernel), word 0 filled in here.
// ---------------------------------------------------------------------------

static std::vector<unsigned long long> compare_tensors(
    const std::vector<unsigned long long>& flat, int n,
    const std::vector<uint32_t>& classes, uintptr_t flat_ptr,
    bool flat_on_host, unsigned long long total_bytes,
    uintptr_t producer_stream, int device) {
  // refused before the GPU is touched
  const std::vector<Desc> descs = parse_descs(flat, n);
  const FlatSide flat_side{0, flat_ptr, total_bytes, 0};
  check_descs(descs, DescKind::Compare, &flat_side, &classes);

  std::vector<unsigned long long> results(6 * (size_t)n, 0);
  for (size_t i = 0; i < (size_t)n; ++i) {
    results[6 * i] = descs[i].nbytes / cmp_elem_size(classes[i]);
  }
  const std::vector<unsigned long long> wu_prefix = wu_prefix_of(descs);
  const unsigned long long total_wus = wu_prefix[n];
  if (total_wus == 0) return results;

  // descriptors | prefix sums | classes
  const LaunchTables tables(descs, wu_prefix, classes.data(),
                            sizeof(uint32_t) * n);
  // Out of pinned memory the kernel is PCIe-bound like the direct restore
  // scatter, and 256 workgroups reach the link rate; out of HBM it is the
  // stats kernel's read with f64 work behind it
  const unsigned int grid = grid_for(total_wus, flat_on_host ? 256ull : 2048ull,
                                     getenv("TSAMD_PACK_GRID"));
  const size_t result_bytes = sizeof(unsigned long long) * results.size();
  const size_t partial_bytes = (size_t)total_wus * 2 * sizeof(double);

  py::gil_scoped_release release;
  HIP_CHECK(hipSetDevice(device));
  DeviceCtx& ctx = get_ctx(device);
  hipStream_t stream = ctx.h2d_stream;
  const char* flat_base = reinterpret_cast<const char*>(flat_ptr);
  if (flat_on_host) {
    void* dev_ptr = nullptr;
    if (hipHostGetDevicePointer(&dev_ptr, reinterpret_cast<void*>(flat_ptr),
                                0) == hipSuccess &&
        dev_ptr != nullptr) {
      flat_base = static_cast<const char*>(dev_ptr);
    }
  }
  chain_after(stream, producer_stream, device);

  // results, then the partial sums of stage one, in one allocation
  void* scratch = nullptr;
  HIP_CHECK(hipMallocAsync(&scratch, result_bytes + partial_bytes, stream));
  unsigned long long* d_out = static_cast<unsigned long long*>(scratch);
  double* d_partials = reinterpret_cast<double*>(d_out + results.size());
  hipError_t err = hipMemsetAsync(d_out, 0, result_bytes, stream);
  std::string refusal;
  if (err == hipSuccess) {
    try {
      enqueue_with_tables(ctx.h2d_ring, stream, tables, [&](const void* d_tables) {
        hipLaunchKernelGGL(
            compare_kernel, dim3(grid), dim3(kBlockThreads), 0, stream,
            tables.descs(d_tables),
            static_cast<const uint32_t*>(tables.extra(d_tables)), n,
            tables.prefix(d_tables), total_wus, flat_base, d_out, d_partials);
        hipLaunchKernelGGL(compare_finish_kernel, dim3((unsigned int)n),
                           dim3(64), 0, stream, n, tables.prefix(d_tables),
                           static_cast<const double*>(d_partials), d_out);
        HIP_CHECK(hipGetLastError());
      });
    } catch (const std::exception& e) {
      refusal = e.what();
    }
  }
  // words 1-5 come back; word 0 is the host's. Whatever happened, the
  // stream is drained before `results` and the scratch go away
  std::vector<unsigned long long> got(results.size(), 0);
  if (err == hipSuccess && refusal.empty()) {
    err = hipMemcpyAsync(got.data(), d_out, result_bytes,
                         hipMemcpyDeviceToHost, stream);
  }
  (void)hipFreeAsync(scratch, stream);
  const hipError_t sync_err = hipStreamSynchronize(stream);
  if (!refusal.empty()) throw std::runtime_error("compare_tensors: " + refusal);
  if (err == hipSuccess) err = sync_err;
  if (err != hipSuccess) {
    throw std::runtime_error(std::string("compare_tensors: ") +
                             hipGetErrorString(err));
  }
  for (size_t i = 0; i < got.size(); ++i) {
    if (i % 6 != 0) results[i] = got[i];
  }
  return results;
}

// Host-side psum64 (single pass, std::thread-parallel): the
// python-level vectorized implementations burn ~10 full memory passes
// on splitmix temporaries (~0.2-0.3 GB/s); this one runs at memcpy-ish
// rate and keeps CPU-target verified restores cheap.
static unsigned long long psum64_host(py::buffer b,
                                      unsigned long long word_base) {
  py::buffer_info info = b.request();
  const unsigned char* base = static_cast<const unsigned char*>(info.ptr);
  unsigned long long nbytes =
      (unsigned long long)info.size * (unsigned long long)info.itemsize;
  unsigned long long nwords = nbytes >> 3;
  unsigned int nthreads = std::thread::hardware_concurrency();
  if (nthreads == 0) nthreads = 4;
  if (nwords < (1u << 16)) nthreads = 1;
  std::vector<unsigned long long> partial(nthreads, 0);
  std::vector<std::thread> workers;
  unsigned long long per = nwords / nthreads;
  py::gil_scoped_release release;
  for (unsigned int t = 0; t < nthreads; ++t) {
    unsigned long long lo = t * per;
    unsigned long long hi = (t + 1 == nthreads) ? nwords : lo + per;
    workers.emplace_back([=, &partial]() {
      unsigned long long acc = 0;
      const unsigned long long* w =
          reinterpret_cast<const unsigned long long*>(base);
      // byte-wise memcpy load when base is unaligned (never in practice:
      // python buffers are malloc-aligned)
      for (unsigned long long i = lo; i < hi; ++i) {
        unsigned long long v;
        memcpy(&v, w + i, 8);
        acc += v * psum_mult(word_base + i);
      }
      partial[t] = acc;
    });
  }
  for (auto& th : workers) th.join();
  unsigned long long total = 0;
  for (auto p : partial) total += p;
  // tail bytes (<8), lane-shifted like the kernel/CPU verifier
  for (unsigned long long bpos = nwords << 3; bpos < nbytes; ++bpos) {
    unsigned long long v = base[bpos];
    unsigned long long file_b = (word_base << 3) + bpos;
    total += (v << (8 * (file_b & 7))) * psum_mult(file_b >> 3);
  }
  return total;
}

// Storage payload write (ops/hip/file_sink.h): open, pwrite loop, optional
// fsync and close in one GIL-free call. Returns true when the existing
// file's pages were reused (no O_TRUNC).
static bool file_write(py::object path, py::object buf, bool fsync,
                       long long chunk_bytes, bool reuse) {
  if (chunk_bytes <= 0) {
    throw py::value_error("file_write: chunk_bytes must be positive");
  }
  // str / bytes / os.PathLike -> filesystem-encoded bytes
  PyObject* fs_bytes = nullptr;
  if (!PyUnicode_FSConverter(path.ptr(), &fs_bytes)) {
    throw py::error_already_set();
  }
  std::string cpath(PyBytes_AS_STRING(fs_bytes),
                    (size_t)PyBytes_GET_SIZE(fs_bytes));
  Py_DECREF(fs_bytes);
  // PyBUF_SIMPLE: any C-contiguous exporter, read-only ones included;
  // a non-contiguous view raises BufferError here
  Py_buffer view;
  if (PyObject_GetBuffer(buf.ptr(), &view, PyBUF_SIMPLE) != 0) {
    throw py::error_already_set();
  }
  tsamd::SinkResult res;
  {
    py::gil_scoped_release release;
    res = tsamd::file_write(cpath, view.buf, (size_t)view.len, fsync,
                            (size_t)chunk_bytes, reuse);
  }
  PyBuffer_Release(&view);
  if (res.err) {
    errno = res.err;
    PyErr_SetFromErrnoWithFilenameObject(PyExc_OSError, path.ptr());
    throw py::error_already_set();
  }
  return res.reused;
}

static void op_wait(long long handle) {
  hipEvent_t ev = nullptr;
  int device = 0;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_ops.find(handle);
    if (it == g_ops.end()) return;  // already waited
    ev = it->second.ev;
    device = it->second.device;
  }
  hipError_t e;
  {
    py::gil_scoped_release release;
    e = hipEventSynchronize(ev);
  }
  {
    // erase even on failure so the op map and event never leak
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_ops.find(handle);
    if (it != g_ops.end()) {
      (void)hipEventDestroy(it->second.ev);
      g_ops.erase(it);
    }
  }
  if (e != hipSuccess) {
    throw std::runtime_error(std::string("hipEventSynchronize: ") +
                             hipGetErrorString(e));
  }
}

static bool op_query(long long handle) {
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_ops.find(handle);
  if (it == g_ops.end()) return true;
  return hipEventQuery(it->second.ev) == hipSuccess;
}

static size_t pending_ops() {
  std::lock_guard<std::mutex> lk(g_mu);
  return g_ops.size();
}

static bool is_managed_ptr(uintptr_t ptr) {
  hipPointerAttribute_t attr;
  hipError_t e =
      hipPointerGetAttributes(&attr, reinterpret_cast<void*>(ptr));
  if (e != hipSuccess) {
    (void)hipGetLastError();  // clear
    return false;
  }
  return attr.type == hipMemoryTypeManaged;
}

static int device_count() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// -- UVM (managed memory) ----------------------------------------------------

static uintptr_t managed_alloc(unsigned long long nbytes, int device) {
  HIP_CHECK(hipSetDevice(device));
  void* ptr = nullptr;
  HIP_CHECK(hipMallocManaged(&ptr, nbytes, hipMemAttachGlobal));
  return reinterpret_cast<uintptr_t>(ptr);
}

static void managed_free(uintptr_t ptr) {
  HIP_CHECK(hipFree(reinterpret_cast<void*>(ptr)));
}

static void managed_advise_preferred_cpu(uintptr_t ptr,
                                         unsigned long long nbytes) {
  // embedding-table pattern: keep pages host-resident, GPU reads over PCIe
  hipError_t e = hipMemAdvise(reinterpret_cast<void*>(ptr), nbytes,
                              hipMemAdviseSetPreferredLocation,
                              hipCpuDeviceId);
  (void)e;  // advisory only
}

static void managed_prefetch(uintptr_t ptr, unsigned long long nbytes,
                             int device) {
  // device = -1 prefetches to the CPU
  DeviceCtx& ctx = get_ctx(device >= 0 ? device : 0);
  hipError_t e = hipMemPrefetchAsync(
      reinterpret_cast<void*>(ptr), nbytes,
      device >= 0 ? device : hipCpuDeviceId, ctx.h2d_stream);
  (void)e;  // advisory only
  (void)hipStreamSynchronize(ctx.h2d_stream);
}

PYBIND11_MODULE(_csnap, m) {
  m.doc() = "torchsnapshot_amd HIP staging engine (gfx950)";
  m.def("d2h_copy", &d2h_copy, "async D2H copy on the side stream");
  m.def("pack_d2h", &pack_d2h,
        "gather-pack tensors into a slab and copy it to pinned host memory",
        py::arg("flat"), py::arg("n"), py::arg("slab_ptr"),
        py::arg("pinned_ptr"), py::arg("total_bytes"),
        py::arg("producer_stream"), py::arg("device"),
        py::arg("hash_out_ptr") = 0);
  m.def("scatter_h2d", &scatter_h2d,
        "copy pinned host bytes to device and scatter into strided tensors");
  m.def("unpack_h2d", &unpack_h2d,
        "restore scatter: pinned host bytes (read in place, or through a "
        "device slab when slab_ptr != 0) into strided tensors, widening "
        "bf16/f16 -> f32 per descriptor; hash_out_ptr != 0 also accumulates "
        "each descriptor's psum64 at file offset hash_byte0 + flat_off",
        py::arg("flat"), py::arg("n"), py::arg("slab_ptr"),
        py::arg("pinned_ptr"), py::arg("total_bytes"),
        py::arg("producer_stream"), py::arg("device"),
        py::arg("hash_out_ptr") = 0, py::arg("hash_byte0") = 0);
  m.def("psum64_host", &psum64_host,
        "single-pass threaded host psum64 of a buffer",
        py::arg("buf"), py::arg("word_base") = 0);
  m.def("psum64_dev", &psum64_dev,
        "psum64 of a flat contiguous device buffer (blocking)",
        py::arg("ptr"), py::arg("nbytes"), py::arg("byte0"),
        py::arg("producer_stream"), py::arg("device"));
  m.def("scan_nonfinite", &scan_nonfinite,
        "count NaN and Inf elements of strided device tensors in one launch "
        "(blocking); returns [nan_0, inf_0, nan_1, inf_1, ...]",
        py::arg("flat"), py::arg("classes"), py::arg("n"),
        py::arg("producer_stream"), py::arg("device"));
  m.def("fingerprint_tensors", &fingerprint_tensors,
        "psum64 of the stored bytes of strided device tensors, read in place "
        "in one launch (blocking); one value per descriptor, hashed at file "
        "offset flat_off",
        py::arg("flat"), py::arg("n"), py::arg("producer_stream"),
        py::arg("device"));
  m.def("tensor_stats", &tensor_stats,
        "value statistics of strided device tensors over their finite "
        "elements, read in place (blocking); six words per descriptor: "
        "n_finite, n_zero, min key, max key, sum and sum of squares as f64 "
        "bits; max_grid > 0 bounds the workgroups",
        py::arg("flat"), py::arg("n"), py::arg("classes"), py::arg("device"),
        py::arg("stream"), py::arg("max_grid") = 0);
  m.def("tensor_hist", &tensor_hist,
        "exponent histograms of strided device tensors, read in place "
        "(blocking); 280 words per descriptor: n_zero, n_negative, "
        "n_nonfinite, then the count of finite non-zero elements per binade "
        "floor(log2|x|) = -149..127; max_grid > 0 bounds the workgroups",
        py::arg("flat"), py::arg("n"), py::arg("classes"), py::arg("device"),
        py::arg("stream"), py::arg("max_grid") = 0);
  m.def("compare_tensors", &compare_tensors,
        "compare a stored payload, read in place from pinned host memory "
        "(flat_on_host) or from device memory, with live strided device "
        "tensors (blocking); six words per descriptor: n, n_diff, "
        "n_nonfinite_diff, and max |v - s|, sum (v - s)^2, sum s^2 as f64 "
        "bits over the pairs with both sides finite",
        py::arg("flat"), py::arg("n"), py::arg("classes"),
        py::arg("flat_ptr"), py::arg("flat_on_host"), py::arg("total_bytes"),
        py::arg("stream"), py::arg("device"));
  m.def("file_write", &::file_write,  // not tsamd::file_write
       
        "write a buffer to a file (GIL released); reuse=True overwrites an "
        "existing file of >= 1 MiB payload in place instead of truncating",
        py::arg("path"), py::arg("buf"), py::arg("fsync") = false,
        py::arg("chunk_bytes") = 256ll * 1024 * 1024, py::arg("reuse") = true);
  m.def("wait", &op_wait, "block until an op completes");
  m.def("query", &op_query, "poll an op");
  m.def("pending_ops", &pending_ops,
        "number of launched ops that have not been waited for");
  m.def("table_ring_slots", []() { return tsamd::kTableRingSlots; },
        "slots of each launch-table ring (one ring per device and side "
        "stream)");
  m.def("table_ring_slot_bytes",
        []() { return (unsigned long long)tsamd::kTableRingSlotBytes; },
        "largest launch table (descriptors + prefix sums) that goes through "
        "a ring slot; a larger one takes the blocking fallback");
  m.def("is_managed_ptr", &is_managed_ptr);
  m.def("device_count", &device_count);
  m.def("managed_alloc", &managed_alloc, "hipMallocManaged");
  m.def("managed_free", &managed_free);
  m.def("managed_advise_preferred_cpu", &managed_advise_preferred_cpu);
  m.def("managed_prefetch", &managed_prefetch);
}
