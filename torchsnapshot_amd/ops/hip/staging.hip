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
//   - scan kernel: NaN / Inf counts per tensor over the same descriptors,
//     read-only, one launch for the whole state (the nonfinite= policy)
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
//     widen_vec, scan_vec. Each kernel family differs only in this
//   - add_per_wave: wave64 reduction and one atomic per wave, for the u64
//     hashes and the u32 counters alike
//   - on the host (desc_check.h): parse_descs + check_descs validate every
//     descriptor before the GPU is touched; wu_prefix_of, grid_for and
//     LaunchTables are the launch prologue of both launchers
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

// Convert 2*VEC source bytes at `src` into VEC bytes at `flat`. Every load
// and store is naturally aligned to its own width (the host picks vec so).
// When HASH, returns the psum64 contribution of the STORED bytes.
template <int VEC, bool HASH>
__device__ inline unsigned long long cast_vec(char* flat, const char* src,
                                              uint32_t code,
                                              unsigned long long file_off) {
  unsigned long long h = 0;
  if (VEC == 16) {
    const uint4 a = *reinterpret_cast<const uint4*>(src);
    const uint4 b = *reinterpret_cast<const uint4*>(src + 16);
    uint4 o;
    o.x = cast_pair(a.x, a.y, code);
    o.y = cast_pair(a.z, a.w, code);
    o.z = cast_pair(b.x, b.y, code);
    o.w = cast_pair(b.z, b.w, code);
    *reinterpret_cast<uint4*>(flat) = o;
    if (HASH) {
      unsigned long long w = file_off >> 3;
      h += (((unsigned long long)o.y << 32) | o.x) * psum_mult(w);
      h += (((unsigned long long)o.w << 32) | o.z) * psum_mult(w + 1);
    }
  } else if (VEC == 8) {
    const uint4 a = *reinterpret_cast<const uint4*>(src);
    uint2 o;
    o.x = cast_pair(a.x, a.y, code);
    o.y = cast_pair(a.z, a.w, code);
    *reinterpret_cast<uint2*>(flat) = o;
    if (HASH) {
      h += (((unsigned long long)o.y << 32) | o.x) * psum_mult(file_off >> 3);
    }
  } else if (VEC == 4) {
    const uint2 a = *reinterpret_cast<const uint2*>(src);
    const uint32_t o = cast_pair(a.x, a.y, code);
    *reinterpret_cast<uint32_t*>(flat) = o;
    if (HASH) {
      h += ((unsigned long long)o << (8 * (file_off & 7))) *
           psum_mult(file_off >> 3);
    }
  } else {
    const uint32_t a = *reinterpret_cast<const uint32_t*>(src);
    const uint32_t o = (code == kCastBF16 ? f32_to_bf16_bits(a)
                                          : f32_to_f16_bits(a)) & 0xFFFFu;
    *reinterpret_cast<uint16_t*>(flat) = (uint16_t)o;
    if (HASH) {
      h += ((unsigned long long)o << (8 * (file_off & 7))) *
           psum_mult(file_off >> 3);
    }
  }
  return h;
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
        unsigned long long h = 0;
        if (CAST && d.cast != kCastNone) {
          switch (d.vec) {
            case 16: h = cast_range<16, HASH>(d, flat_base, s, e); break;
            case 8: h = cast_range<8, HASH>(d, flat_base, s, e); break;
            case 4: h = cast_range<4, HASH>(d, flat_base, s, e); break;
            default: h = cast_range<2, HASH>(d, flat_base, s, e); break;
          }
        } else {
          switch (d.vec) {
            case 16: h = gather_range<16, HASH>(d, flat_base, s, e); break;
            case 8: h = gather_range<8, HASH>(d, flat_base, s, e); break;
            case 4: h = gather_range<4, HASH>(d, flat_base, s, e); break;
            case 2: h = gather_range<2, HASH>(d, flat_base, s, e); break;
            default: h = gather_range<1, HASH>(d, flat_base, s, e); break;
          }
        }
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
        const unsigned long long ho = hash_byte0 + d.flat_off;
        const char* fb = flat_base;
        unsigned long long h = 0;
        if (WIDEN && d.cast != kCastNone) {
          switch (d.vec) {
            case 16: h = widen_range<16, HASH>(d, fb, s, e, ho); break;
            case 8: h = widen_range<8, HASH>(d, fb, s, e, ho); break;
            case 4: h = widen_range<4, HASH>(d, fb, s, e, ho); break;
            default: h = widen_range<2, HASH>(d, fb, s, e, ho); break;
          }
        } else {
          switch (d.vec) {
            case 16: h = scatter_range<16, HASH>(d, fb, s, e, ho); break;
            case 8: h = scatter_range<8, HASH>(d, fb, s, e, ho); break;
            case 4: h = scatter_range<4, HASH>(d, fb, s, e, ho); break;
            case 2: h = scatter_range<2, HASH>(d, fb, s, e, ho); break;
            default: h = scatter_range<1, HASH>(d, fb, s, e, ho); break;
          }
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
  bool any_cast = false;
  for (const Desc& d : descs) any_cast = any_cast || d.cast != kCastNone;

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
  const size_t table_bytes = tables.host.size();

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
      auto kernel = any_cast ? (hash ? pack_kernel<true, true>
                                     : pack_kernel<false, true>)
                             : (hash ? pack_kernel<true, false>
                                     : pack_kernel<false, false>);
      hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlockThreads), 0, stream,
                         d_descs, n, d_prefix, total_wus, flat_base, hash_out);
    } else {
      auto kernel = any_cast ? (hash ? unpack_kernel<true, true>
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

  HipTableRing& ring = gather ? ctx.d2h_ring : ctx.h2d_ring;
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
  std::vector<unsigned long long> counts(2 * (size_t)n, 0);

  const std::vector<unsigned long long> wu_prefix = wu_prefix_of(descs);
  const unsigned long long total_wus = wu_prefix[n];
  if (total_wus == 0) return counts;

  // one device allocation: descriptors | prefix sums | classes | counters
  const LaunchTables tables(descs, wu_prefix, classes.data(),
                            sizeof(uint32_t) * n);
  const size_t count_bytes = sizeof(unsigned long long) * 2 * n;

  // HBM-bound read: fill the chip like the slab-mode gather does
  const unsigned int grid =
      grid_for(total_wus, 16384ull, getenv("TSAMD_PACK_GRID"));

  py::gil_scoped_release release;
  HIP_CHECK(hipSetDevice(device));
  DeviceCtx& ctx = get_ctx(device);
  hipStream_t stream = ctx.d2h_stream;
  chain_after(stream, producer_stream, device);

  void* scratch = nullptr;
  HIP_CHECK(hipMallocAsync(&scratch, tables.host.size() + count_bytes, stream));
  unsigned long long* d_counts = reinterpret_cast<unsigned long long*>(
      reinterpret_cast<char*>(scratch) + tables.host.size());

  // enqueue everything, then synchronise whatever happened: the host
  // buffers above must outlive the copies that read and write them
  hipError_t err = hipMemsetAsync(d_counts, 0, count_bytes, stream);
  if (err == hipSuccess) {
    err = hipMemcpyAsync(scratch, tables.host.data(), tables.host.size(),
                         hipMemcpyHostToDevice, stream);
  }
  if (err == hipSuccess) {
    hipLaunchKernelGGL(scan_kernel, dim3(grid), dim3(kBlockThreads), 0, stream,
                       tables.descs(scratch),
                       static_cast<const uint32_t*>(tables.extra(scratch)), n,
                       tables.prefix(scratch), total_wus, d_counts);
    err = hipGetLastError();
  }
  if (err == hipSuccess) {
    err = hipMemcpyAsync(counts.data(), d_counts, count_bytes,
                         hipMemcpyDeviceToHost, stream);
  }
  (void)hipFreeAsync(scratch, stream);
  const hipError_t sync_err = hipStreamSynchronize(stream);
  if (err == hipSuccess) err = sync_err;
  if (err != hipSuccess) {
    throw std::runtime_error(std::string("scan_nonfinite: ") +
                             hipGetErrorString(err));
  }
  return counts;
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
