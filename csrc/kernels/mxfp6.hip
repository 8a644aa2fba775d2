// bf16 <-> MXFP6 (OCP e2m3 codes, 24 bytes per 32 elements, one E8M0 scale byte
// per 32 elements) pack/unpack in the layout of core/mxfp6.h, bit-exact with
// its host reference, and the verify + unpack of packed layers and chunks.
//
// Shape. v_cvt_scalef32_pk32_fp6_bf16 and v_cvt_scalef32_pk32_bf16_fp6 convert
// a whole block in one lane: 16 VGPRs of bf16 against 6 dwords of codes. A wave
// works on a tile of 64 consecutive blocks (4 KiB of bf16, 1536 B of codes),
// lane l owning block l of the tile, and both sides of the tile move coalesced:
//   * bf16: four 16-B accesses per lane. Access r of lane m + 16 q covers word
//     q of block 16 r + m, so one instruction of the wave covers one whole KiB;
//     the 4x4 register transpose across the wave's rows (mxfp6_row_transpose,
//     crc32c.hip's pattern) moves between that and "lane l holds the four words
//     of block l". Accessed directly (every lane 16 B of its own 64-B block per
//     instruction) each instruction touches 16 B in every 64: the pattern that
//     cost the first fused MXFP4 kernel 100 us against 21.
//   * codes: a lane's 24 B are not a power of two, so they cross the wave
//     through a 1536-B LDS slot of the wave: lane l writes or reads its 24 B at
//     24 l (three 8-B accesses), and global memory sees three 8-B accesses per
//     lane, instruction j covering the contiguous 512 B at 512 j. 8 B is the
//     alignment the contract gives q. A wave's LDS operations run in issue
//     order, so the slot needs no barrier, only the compiler fence.
//   * scale bytes: one ordinary vector byte access per lane, 64 contiguous
//     bytes per wave.
// Stores are nontemporal (written once, read by a later pass or another GPU).
// A block's finite amax and NaN flag are found in the bit domain (mxfp6_cvt.h).
//
// Registers (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage; no
// scratch and no spills in any of them, 8 waves per SIMD): mxfp6_pack_kernel 40
// VGPRs, mxfp6_unpack_kernel<FlatGeo> 45, <LayerGeo> 48, <BatchGeo> 44; 6 KiB
// of LDS per 256-thread workgroup.
//
// Verify + unpack (mxfp6_verify_unpack, _batch): a 24-byte block does not
// divide the CRC walk's 16-B words, KiBs or 16 KiB segments, so this is not a
// visit of crc32c.hip's fused kernel. It is the CRC-only walk (crc32c_chunks /
// crc32c_batch) followed, on the same stream, by one grid-stride launch of the
// unpack kernel over all tiles of the layer or batch, its grid sized to the CUs
// the stream may use (`cus`) times the workgroups a CU holds. The packed bytes
// are read twice (2 x 25 MiB per 64 MiB source chunk against 64 MiB written).
// Nothing is allocated.
//
// The converters against core/mxfp6.h, measured on MI355X against integer code
// (bin/cvtprobe, profiles/mxfp6/cvtprobe.jsonl) for every bf16 pattern at every
// scale 2^E, E in [-126, 125] (16.5 M inputs), every code in every one of the
// 32 positions under every scale byte (16.8 M elements), and a single set
// element in each position:
//   * layout: element i of the block is bits [6i, 6i + 6) of the six dwords
//     read as one little-endian integer, dword 0 first; element 2k is the low
//     half of bf16 dword k - the layout of core/mxfp6.h, used as it is;
//   * finite values up to 7.5 * 2^E: nearest code, ties to the even code, sign
//     kept (-0 and values that round to 0 included), bf16 subnormals exact -
//     0 mismatches in 8.3 M inputs, 31 188 of them next to a code boundary;
//   * values above 7.5 * 2^E (a block whose E is capped at 125, 8.1 M inputs)
//     and +-inf: the converter saturates to +-7.5, which is the reference's
//     clamp - used as it is;
//   * NaN: e2m3 has none, the converter saturates it to +-7.5 (all 64 008
//     inputs). The reference marks the whole block instead, so the kernel finds
//     NaNs in the bit domain and writes 24 zero bytes and scale byte 0xFF: the
//     one case of pack in plain code;
//   * unpack: exact for scale bytes 0..254 - bf16-subnormal results (bytes 0
//     and 1) and overflow to +-inf beyond bf16's range (253, 254, never written
//     by pack) included, 0 mismatches. For 0xFF the converter returns NaNs, but
//     not the reference's 0x7FC0 in any of the 65 536 elements (0xFFC0 for the
//     positive code 0x12): that byte's result is a constant, selected instead
//     of converted (mxfp6_cvt.h): the one case of unpack in plain code.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels/kernels.h"
#include "kernels/mxfp6_cvt.h"

namespace dissem {
namespace kern {

namespace {

using u32x4_t = mxfp6_u32x4_t;
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));

constexpr int kTileBlocks = 64;  // blocks per wave tile: one per lane
constexpr int kWaves = 4;        // waves per workgroup
constexpr int kSlotBytes = kTileBlocks * 24;
constexpr int kWgPerCu = 8;      // 256-thread workgroups a CU holds (2048 threads)

// One tile: `nb` (1..64) blocks. q: their codes (8-B aligned), scales: their
// scale bytes, x: their bf16 (16-B aligned).
struct Tile {
  const uint8_t* q;
  const uint8_t* scales;
  uint16_t* x;
  int nb;
};

// byte offset, in the tile's bf16, of access r of this lane (see the header)
__device__ __forceinline__ int bf16_off(int lane, int r) { return (16 * r + (lane & 15)) * 64 + 16 * (lane >> 4); }

__device__ __forceinline__ void pack_tile(const uint16_t* __restrict__ x, int nb, uint8_t* __restrict__ q,
                                          uint8_t* __restrict__ scales, uint32_t* slot) {
  const int lane = threadIdx.x & 63;
  u32x4_t w[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const bool in = 16 * r + (lane & 15) < nb;
    w[r] = in ? *reinterpret_cast<const u32x4_t*>(reinterpret_cast<const uint8_t*>(x) + bf16_off(lane, r))
              : u32x4_t{0, 0, 0, 0};
  }
  mxfp6_row_transpose(w[0], w[1], w[2], w[3]);  // lane l: the four words of block l
  mxfp6_u32x16_t v;
#pragma unroll
  for (int i = 0; i < 16; ++i) v[i] = w[i >> 2][i & 3];
  uint32_t sb;
  const mxfp6_u32x6_t c = mxfp6_pack_block(v, &sb);
  u32x2_t* s2 = reinterpret_cast<u32x2_t*>(slot);
  s2[3 * lane] = u32x2_t{c[0], c[1]};
  s2[3 * lane + 1] = u32x2_t{c[2], c[3]};
  s2[3 * lane + 2] = u32x2_t{c[4], c[5]};
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int u = 64 * j + lane;  // 8-B unit of the tile's codes
    const u32x2_t d = s2[u];
    if (u < 3 * nb) __builtin_nontemporal_store(d, reinterpret_cast<u32x2_t*>(q) + u);
  }
  __builtin_amdgcn_wave_barrier();
  if (lane < nb) scales[lane] = uint8_t(sb);
}

__device__ __forceinline__ void unpack_tile(const Tile& t, uint32_t* slot) {
  const int lane = threadIdx.x & 63;
  const uint32_t sb = lane < t.nb ? uint32_t(t.scales[lane]) : 0u;
  u32x2_t* s2 = reinterpret_cast<u32x2_t*>(slot);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int u = 64 * j + lane;
    s2[u] = u < 3 * t.nb ? reinterpret_cast<const u32x2_t*>(t.q)[u] : u32x2_t{0, 0};
  }
  __builtin_amdgcn_wave_barrier();
  const u32x2_t c0 = s2[3 * lane], c1 = s2[3 * lane + 1], c2 = s2[3 * lane + 2];
  __builtin_amdgcn_wave_barrier();
  const mxfp6_u32x16_t v = mxfp6_unpack_block(mxfp6_u32x6_t{c0[0], c0[1], c1[0], c1[1], c2[0], c2[1]}, sb);
  u32x4_t w[4];
#pragma unroll
  for (int i = 0; i < 16; ++i) w[i >> 2][i & 3] = v[i];
  mxfp6_row_transpose(w[0], w[1], w[2], w[3]);  // register r of lane m + 16 q: word q of block 16 r + m
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (16 * r + (lane & 15) < t.nb)
      __builtin_nontemporal_store(w[r], reinterpret_cast<u32x4_t*>(reinterpret_cast<uint8_t*>(t.x) + bf16_off(lane, r)));
}

__global__ void __launch_bounds__(kWaves * 64) mxfp6_pack_kernel(const uint16_t* __restrict__ in, int64_t nblocks,
                                                                 uint8_t* __restrict__ q,
                                                                 uint8_t* __restrict__ scales) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kWaves * kSlotBytes / 4];
  const int wave = threadIdx.x >> 6;
  const int64_t b0 = (int64_t(blockIdx.x) * kWaves + wave) * kTileBlocks;
  if (b0 >= nblocks) return;  // wave-uniform
  const int nb = int(min(int64_t(kTileBlocks), nblocks - b0));
  pack_tile(in + b0 * 32, nb, q + b0 * 24, scales + b0, lds + wave * (kSlotBytes / 4));
}

// ---- geometry of an unpack launch: tile index -> Tile.

// n blocks at (q, scales) -> out
struct FlatGeo {
  const uint8_t* q;
  const uint8_t* scales;
  uint16_t* out;
  int64_t nblocks;
  __device__ Tile operator()(int64_t t) const {
    const int64_t b0 = t * kTileBlocks;
    return Tile{q + b0 * 24, scales + b0, out + b0 * 32, int(min(int64_t(kTileBlocks), nblocks - b0))};
  }
};

// A packed layer (core/mxfp6.h): source chunks of `tpc` whole tiles, the last one shorter.
struct LayerGeo {
  const uint8_t* packed;
  uint16_t* out;
  int64_t src_bytes, src_chunk, pchunk, tpc;
  __device__ Tile operator()(int64_t t) const {
    const int64_t c = t / tpc, b0 = (t - c * tpc) * kTileBlocks;
    const int64_t cb = min(src_chunk, src_bytes - c * src_chunk) / 64;  // blocks of this chunk
    const uint8_t* q = packed + c * pchunk;
    return Tile{q + b0 * 24, q + cb * 24 + b0, out + c * (src_chunk / 2) + b0 * 32,
                int(min(int64_t(kTileBlocks), cb - b0))};
  }
};

// Up to kCrcBatchMax independent packed chunks.
struct BatchGeo {
  int n;
  int64_t tile_base[kCrcBatchMax + 1];  // prefix sums of the items' tile counts
  const uint8_t* packed[kCrcBatchMax];
  int64_t nblocks[kCrcBatchMax];
  uint16_t* out[kCrcBatchMax];
  __device__ Tile operator()(int64_t t) const {
    int j = 0;
    while (j + 1 < n && t >= tile_base[j + 1]) ++j;  // wave-uniform, at most kCrcBatchMax steps
    const int64_t b0 = (t - tile_base[j]) * kTileBlocks;
    return Tile{packed[j] + b0 * 24, packed[j] + nblocks[j] * 24 + b0, out[j] + b0 * 32,
                int(min(int64_t(kTileBlocks), nblocks[j] - b0))};
  }
};

// Grid-stride over the tiles (a launch with one workgroup per kWaves tiles runs the loop once).
template <class Geo>
__global__ void __launch_bounds__(kWaves * 64) mxfp6_unpack_kernel(const Geo geo, int64_t tiles) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kWaves * kSlotBytes / 4];
  const int wave = threadIdx.x >> 6;
  const int64_t stride = int64_t(gridDim.x) * kWaves;
  for (int64_t t = int64_t(blockIdx.x) * kWaves + wave; t < tiles; t += stride)  // wave-uniform
    unpack_tile(geo(t), lds + wave * (kSlotBytes / 4));
}

int device_cus() {
  int dev = 0, cus = 0;
  (void)hipGetDevice(&dev);
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
  return cus;
}

// Workgroups of a grid-stride launch on a stream that may use `cus` CUs (0 = all).
unsigned stride_grid(int64_t tiles, int cus) {
  const int dc = device_cus();
  const int64_t slots = int64_t(cus > 0 ? std::min(cus, dc) : dc) * kWgPerCu;
  return unsigned(std::max<int64_t>(1, std::min(slots, (tiles + kWaves - 1) / kWaves)));
}

int64_t tiles_of(int64_t nblocks) { return (nblocks + kTileBlocks - 1) / kTileBlocks; }

int64_t packed_of(int64_t src_len) { return src_len / 64 * 25; }

}  // namespace

hipError_t mxfp6_pack(const uint16_t* bf16, int64_t n, uint8_t* q, uint8_t* scales, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (n % 32 || (reinterpret_cast<uintptr_t>(bf16) & 15) || (reinterpret_cast<uintptr_t>(q) & 7))
    return hipErrorInvalidValue;
  const int64_t nblocks = n / 32, wgs = (tiles_of(nblocks) + kWaves - 1) / kWaves;
  if (wgs > 0x7FFFFFFF) return hipErrorInvalidValue;
  mxfp6_pack_kernel<<<unsigned(wgs), kWaves * 64, 0, s>>>(bf16, nblocks, q, scales);
  return hipGetLastError();
}

hipError_t mxfp6_unpack(const uint8_t* q, const uint8_t* scales, int64_t n, uint16_t* bf16, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (n % 32 || (reinterpret_cast<uintptr_t>(bf16) & 15) || (reinterpret_cast<uintptr_t>(q) & 7))
    return hipErrorInvalidValue;
  const int64_t nblocks = n / 32, tiles = tiles_of(nblocks), wgs = (tiles + kWaves - 1) / kWaves;
  if (wgs > 0x7FFFFFFF) return hipErrorInvalidValue;
  mxfp6_unpack_kernel<FlatGeo><<<unsigned(wgs), kWaves * 64, 0, s>>>(FlatGeo{q, scales, bf16, nblocks}, tiles);
  return hipGetLastError();
}

hipError_t mxfp6_pack_chunks(const void* src, int64_t src_bytes, int64_t src_chunk, void* dst, hipStream_t s) {
  if (src_chunk <= 0 || src_chunk % 1024 || src_bytes % 64) return hipErrorInvalidValue;
  const int64_t pchunk = packed_of(src_chunk);
  for (int64_t off = 0, c = 0; off < src_bytes; off += src_chunk, ++c) {
    const int64_t n = std::min(src_chunk, src_bytes - off) / 2;
    uint8_t* out = static_cast<uint8_t*>(dst) + c * pchunk;
    hipError_t e = mxfp6_pack(reinterpret_cast<const uint16_t*>(static_cast<const uint8_t*>(src) + off), n, out,
                              out + n / 32 * 24, s);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t mxfp6_verify_unpack(const void* packed, int64_t src_bytes, int64_t src_chunk, uint16_t* out,
                               uint32_t* crc_out, void* workspace, hipStream_t s, int cus) {
  if (src_bytes <= 0) return hipSuccess;
  if (src_chunk <= 0 || src_chunk % 4096 || src_bytes % 64 || (reinterpret_cast<uintptr_t>(packed) & 15) ||
      (reinterpret_cast<uintptr_t>(out) & 15))
    return hipErrorInvalidValue;
  const int64_t pchunk = packed_of(src_chunk);
  const int64_t full = src_bytes / src_chunk, tail = src_bytes % src_chunk;
  const int64_t bytes = full * pchunk + packed_of(tail);
  if (hipError_t e = crc32c_chunks(packed, bytes, pchunk, crc_out, workspace, s, cus); e != hipSuccess) return e;
  const int64_t tpc = src_chunk / 4096, tiles = full * tpc + tiles_of(tail / 64);
  mxfp6_unpack_kernel<LayerGeo><<<stride_grid(tiles, cus), kWaves * 64, 0, s>>>(
      LayerGeo{static_cast<const uint8_t*>(packed), out, src_bytes, src_chunk, pchunk, tpc}, tiles);
  return hipGetLastError();
}

hipError_t mxfp6_verify_unpack_batch(const FusedItem* items, int n, void* workspace, hipStream_t s, int cus) {
  if (n <= 0) return hipSuccess;
  if (n > kCrcBatchMax) return hipErrorInvalidValue;
  CrcItem crc[kCrcBatchMax];
  BatchGeo g{};
  for (int i = 0; i < n; ++i) {
    const FusedItem& it = items[i];
    if (it.src_len <= 0) continue;
    if (it.src_len % 64 || (reinterpret_cast<uintptr_t>(it.out) & 15) || (reinterpret_cast<uintptr_t>(it.packed) & 15))
      return hipErrorInvalidValue;
    const int j = g.n++;
    crc[j] = CrcItem{it.packed, packed_of(it.src_len), it.crc_out};
    g.packed[j] = static_cast<const uint8_t*>(it.packed);
    g.nblocks[j] = it.src_len / 64;
    g.out[j] = it.out;
    g.tile_base[j + 1] = g.tile_base[j] + tiles_of(g.nblocks[j]);
  }
  if (g.n == 0) return hipSuccess;
  if (hipError_t e = crc32c_batch(crc, g.n, workspace, s, cus); e != hipSuccess) return e;
  const int64_t tiles = g.tile_base[g.n];
  mxfp6_unpack_kernel<BatchGeo><<<stride_grid(tiles, cus), kWaves * 64, 0, s>>>(g, tiles);
  return hipGetLastError();
}

}  // namespace kern
}  // namespace dissem
