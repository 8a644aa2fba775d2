// Launchers for the gfx950 kernels. Callable from host C++ (g++ objects); the
// kernels themselves are in csrc/kernels/*.hip, compiled for gfx950 only.
//
// All of them are single-pass streaming kernels: every input byte is read once
// and every output byte written once, 16 B per lane, with no data shared
// between workgroups. The hardware's round-robin of workgroups over the 8 XCDs
// therefore needs no remapping (there is no L2 reuse to keep on one XCD); what
// matters is enough bytes in flight per CU (HBM latency) and, for CRC32C, the
// LDS table layout (crc32c.hip). fill sizes its grid to the CU count (256)
// times the workgroups a CU holds and grid-strides beyond that; the CRC32C
// grids are described below; fp8 pack/unpack give every lane one 8-element
// group (a 64 MiB chunk is 16k workgroups, far more than the chip holds at once).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace dissem {
namespace kern {

// ---- fill.hip: counter-based random bytes (splitmix64 of (seed, u64 index)),
// 16 B per lane stores; byte-identical to kern::fill_random_host.
hipError_t fill_random(void* dst, int64_t bytes, uint64_t seed, hipStream_t s);
void fill_random_host(void* dst, int64_t bytes, uint64_t seed, int64_t offset = 0);
// Test helper: hold stream s until *flag != 0 (host-mapped) or max_iters ~3 us sleeps.
hipError_t spin_until(const uint32_t* flag, uint64_t max_iters, uint64_t* iters, hipStream_t s);

// ---- crc32c.hip: CRC32C verification (and the fused fp8 unpack) on gfx950.
// Two kernels: the CRC-only check walks (one 1024-thread workgroup per CU,
// each a contiguous range of 16 KiB segments), the fused check + unpack runs
// one segment per wave (512-thread workgroups, two per CU). Both fold a
// chunk's segments inside the same launch (device-scope atomics on one 64-bit
// {acc, count} word per item in `workspace`, 8-B aligned; crc32c.hip). A workspace must be
// zeroed ONCE (e.g. hipMemsetAsync) before its first use; every launch leaves
// it zeroed again. Launches that share a workspace must be ordered (one stream).
// `cus`: the CUs the launch's stream may use (a CU-masked verify stream): the
// walk launches one workgroup per such CU, the fused kernel sizes its grid's
// last partial round for them. 0 = the whole device.
//
// out[c] (device or host-mapped memory) receives the standard CRC32C of chunk
// c of [src, src+bytes). src 16-B aligned; chunk_bytes a multiple of 16
// unless the span is one chunk (bytes <= chunk_bytes: any length).
size_t crc32c_workspace_bytes(int64_t bytes, int64_t chunk_bytes);
// Upload the CRC tables (stream-ordered on s) ahead of time; later launches
// then never allocate or copy. Never a host-synchronous copy.
hipError_t crc32c_warm(hipStream_t s);
hipError_t crc32c_chunks(const void* src, int64_t bytes, int64_t chunk_bytes, uint32_t* out, void* workspace,
                         hipStream_t s, int cus = 0);
// Batched: the standard CRC32C of each of up to kCrcBatchMax independent
// buffers (any length, 16-B aligned) in one launch - the chunks one P2P group
// or one staging batch landed. `workspace`: crc32c_batch_workspace_bytes().
constexpr int kCrcBatchMax = 16;
struct CrcItem {
  const void* src;
  int64_t bytes;
  uint32_t* out;
};
size_t crc32c_batch_workspace_bytes();
hipError_t crc32c_batch(const CrcItem* items, int n, void* workspace, hipStream_t s, int cus = 0);

// ---- fp8.hip: bf16 -> OCP fp8 e4m3fn with one f32 scale per `block` elements
// (power-of-two scale 2^E, core/fp8.h; +-inf saturate, NaN stays NaN), and back.
hipError_t fp8_pack(const uint16_t* bf16, int64_t n, uint8_t* fp8, float* scales, int block, hipStream_t s);
hipError_t fp8_unpack(const uint8_t* fp8, const float* scales, int64_t n, uint16_t* bf16, int block, hipStream_t s);
// Whole layer into the chunked packed layout of core/fp8.h (one pack launch per chunk).
hipError_t fp8_pack_chunks(const void* src, int64_t src_bytes, int64_t src_chunk, int block, void* dst,
                           hipStream_t s);

// ---- crc32c.hip: fused verify + unpack of a packed layer: crc_out[c] = CRC32C of
// packed chunk c, out = the bf16 layer (src_bytes). One pass over the packed bytes.
// `workspace`: crc32c_workspace_bytes(packed bytes, packed chunk) bytes, zeroed once.
hipError_t fp8_verify_unpack(const void* packed, int64_t src_bytes, int64_t src_chunk, int block, uint16_t* out,
                             uint32_t* crc_out, void* workspace, hipStream_t s, int cus = 0);
// Batched: up to kCrcBatchMax independent packed chunks (each the core/fp8.h
// image of `src_len` bf16 source bytes) in one launch: CRC32C of each packed
// chunk to *crc_out, its bf16 values to out. `workspace`: crc32c_batch_workspace_bytes().
struct FusedItem {
  const void* packed;
  int64_t src_len;
  uint16_t* out;
  uint32_t* crc_out;
};
hipError_t fp8_verify_unpack_batch(const FusedItem* items, int n, int block, void* workspace, hipStream_t s,
                                   int cus = 0);

// ---- mxfp4.hip: bf16 -> MXFP4 (e2m1 codes, two per byte, element 2k in the low
// nibble; one E8M0 scale byte per 32 elements; core/mxfp4.h) and back,
// bit-exact with the host reference. n a multiple of 32; bf16 16-B, q 4-B aligned.
hipError_t mxfp4_pack(const uint16_t* bf16, int64_t n, uint8_t* q, uint8_t* scales, hipStream_t s);
hipError_t mxfp4_unpack(const uint8_t* q, const uint8_t* scales, int64_t n, uint16_t* bf16, hipStream_t s);
// Whole layer into the chunked packed layout of core/mxfp4.h (one pack launch per chunk).
hipError_t mxfp4_pack_chunks(const void* src, int64_t src_bytes, int64_t src_chunk, void* dst, hipStream_t s);

// ---- crc32c.hip: the same fused verify + unpack for MXFP4-packed layers and
// chunks (core/mxfp4.h layout; src_chunk a multiple of 4096, src_bytes and
// every src_len a multiple of 64).
hipError_t mxfp4_verify_unpack(const void* packed, int64_t src_bytes, int64_t src_chunk, uint16_t* out,
                               uint32_t* crc_out, void* workspace, hipStream_t s, int cus = 0);
hipError_t mxfp4_verify_unpack_batch(const FusedItem* items, int n, void* workspace, hipStream_t s, int cus = 0);

// ---- mxfp6.hip: bf16 -> MXFP6 (e2m3 codes, 24 bytes per 32 elements, element i
// at bits [6i, 6i + 6) of its block; one E8M0 scale byte per 32 elements;
// core/mxfp6.h) and back, bit-exact with the host reference. n a multiple of 32;
// bf16 16-B, q 8-B aligned. Nothing allocated, the caller's stream.
hipError_t mxfp6_pack(const uint16_t* bf16, int64_t n, uint8_t* q, uint8_t* scales, hipStream_t s);
hipError_t mxfp6_unpack(const uint8_t* q, const uint8_t* scales, int64_t n, uint16_t* bf16, hipStream_t s);
// Whole layer into the chunked packed layout of core/mxfp6.h (one pack launch per chunk).
hipError_t mxfp6_pack_chunks(const void* src, int64_t src_bytes, int64_t src_chunk, void* dst, hipStream_t s);
// Verify + unpack of MXFP6-packed layers and chunks: arguments, workspace and
// results as for the MXFP4 pair (src_chunk a multiple of 4096, src_bytes and
// every src_len a multiple of 64). Two launches on `s`: the CRC-only walk, then
// a grid-stride unpack sized to `cus` - the packed bytes are read twice.
hipError_t mxfp6_verify_unpack(const void* packed, int64_t src_bytes, int64_t src_chunk, uint16_t* out,
                               uint32_t* crc_out, void* workspace, hipStream_t s, int cus = 0);
hipError_t mxfp6_verify_unpack_batch(const FusedItem* items, int n, void* workspace, hipStream_t s, int cus = 0);

// ---- mxfp4_linear.hip: y[m][n] = sum_k x[m][k] * W[n][k] with W read in place
// from an MXFP4-packed layer (no bf16 copy of W): W is a row-major [N, K]
// parameter whose element 0 is element `elem_off` of the layer of `src_bytes`
// stored at `packed` in the chunked layout of core/mxfp4.h. x: bf16 [M, K],
// contiguous, 16-B aligned; y: f32 or bf16 [M, N] with a row stride of `ldy`
// elements; f32 accumulation (v_mfma_f32_16x16x32_bf16). K, elem_off multiples
// of 32, N of 16, M >= 1, the parameter inside the layer; `packed` 16-B aligned.
// Anything else: hipErrorInvalidValue. Stream-ordered, no allocation, no
// workspace: K is split over the waves of a workgroup (`split_k` of them, 1..16;
// 0 = chosen from the shape, mxfp4_linear_slices) and reduced through LDS in a
// fixed order, so equal inputs give equal bits. `row_tiles_per_wave` (0 =
// chosen from the shape; 1, 2 or 4, a divisor of N / 16; at most 2 beyond 32
// rows of x): the 16-row tiles of W a wave feeds from one x fragment. Rows of x
// beyond 64 are served by further passes over W.
//
// DecodePlan is the template instantiation and workgroup size one pass of a
// decode launcher runs: `mt` 16-row tiles of x, `nt` row tiles (gated kernels:
// pairs) per wave, `slices` waves over K. Every *_plan(m, N, K, split_k,
// row_tiles_per_wave) below is the one place its launcher takes these from, for
// a pass of m rows (1..64; anything else: {0, 0, 0}), after clipping a forced
// row_tiles_per_wave to what mt allows and slices to what registers and LDS
// hold. *_slices(M, N, K) is plan(min(M, 64), N, K, 0, 0).slices.
struct DecodePlan {
  int mt, nt, slices;
};
int mxfp4_linear_slices(int64_t M, int64_t N, int64_t K);
DecodePlan mxfp4_linear_plan(int m, int64_t N, int64_t K, int split_k, int row_tiles_per_wave);
hipError_t mxfp4_linear(const void* packed, int64_t src_bytes, int64_t src_chunk, int64_t elem_off, const uint16_t* x,
                        int64_t M, int64_t N, int64_t K, void* y, int64_t ldy, bool y_bf16, int split_k,
                        int row_tiles_per_wave, hipStream_t s);

// ---- mxfp4_swiglu.hip: y[m][n] = silu(g[m][n]) * u[m][n] with g = x * Wg^T and
// u = x * Wu^T, Wg and Wu the [N, K] parameters at elements `gate_off` and
// `up_off` of one packed layer (independent multiples of 32, in any order,
// possibly equal). Arguments, checks and accumulation are mxfp4_linear's, for
// both parameters; g and u never leave the accumulators, and with equal K
// slices they are bit for bit mxfp4_linear's f32 results. The epilogue is
// (g / (1 + expf(-g))) * u in f32, stored as f32 or as bf16 (nearest even).
// `split_k`: 0 = chosen (mxfp4_swiglu_slices), else 1..16, clamped to what the
// registers and 64 KiB of LDS allow. `row_tiles_per_wave` counts pairs of a
// gate and an up tile: 0 = chosen, 1 or 2 (a divisor of N / 16; 1 beyond 32
// rows of x). Stream-ordered, no allocation, no workspace, no atomics.
int mxfp4_swiglu_slices(int64_t M, int64_t N, int64_t K);
DecodePlan mxfp4_swiglu_plan(int m, int64_t N, int64_t K, int split_k, int row_tiles_per_wave);
hipError_t mxfp4_swiglu(const void* packed, int64_t src_bytes, int64_t src_chunk, int64_t gate_off, int64_t up_off,
                        const uint16_t* x, int64_t M, int64_t N, int64_t K, void* y, int64_t ldy, bool y_bf16,
                        int split_k, int row_tiles_per_wave, hipStream_t s);

// ---- mxfp4_tiled.hip: the same two results for many rows of x, each call ONE
// launch for any M. A workgroup owns kMxfp4TiledBM rows of x by kMxfp4TiledBN
// rows of W, stages x through LDS for its waves and dequantizes W in registers,
// so W is read and converted once per kMxfp4TiledBM rows instead of once per
// 64. Layer arguments, x, y, ldy, M, N, K, the offsets and every
// hipErrorInvalidValue case are mxfp4_linear's / mxfp4_swiglu's (there is no
// `split_k` and no `row_tiles_per_wave`); in addition ceil(M / BM) * ceil(N /
// BN) must fit a 1-D grid. K is never split: every output element has one f32
// accumulator (v_mfma_f32_16x16x32_bf16) that walks K in one fixed order, so
// y[m][n] depends only on row m of x and row n of W - the same bits for any M,
// any N and any position in the grid (batch invariance) - and g and u of the
// gated kernel are bit for bit the tiled linear's f32 results. Nothing is read
// outside x[0 : M K) and the parameters' blocks and scale bytes, nothing
// written outside y[:M, :N]. Stream-ordered, no allocation, no workspace, no atomics.
constexpr int kMxfp4TiledBM = 128, kMxfp4TiledBN = 128;
hipError_t mxfp4_linear_tiled(const void* packed, int64_t src_bytes, int64_t src_chunk, int64_t elem_off,
                              const uint16_t* x, int64_t M, int64_t N, int64_t K, void* y, int64_t ldy, bool y_bf16,
                              hipStream_t s);
hipError_t mxfp4_swiglu_tiled(const void* packed, int64_t src_bytes, int64_t src_chunk, int64_t gate_off,
                              int64_t up_off, const uint16_t* x, int64_t M, int64_t N, int64_t K, void* y, int64_t ldy,
                              bool y_bf16, hipStream_t s);

// ---- mxfp8_act.hip: bf16 x [M, K] (contiguous, 16-B aligned, K a multiple of 32)
// -> MXFP8 activations (core/mxfp8_act.h): e4m3fn codes [M, K] (8-B aligned) and one
// E8M0 scale byte per 32 values along K, [M, K / 32]; byte for byte
// mxfp8::quantize_host on every input. One launch for any M, stream-ordered, no
// allocation.
hipError_t mxfp8_quantize_rows(const uint16_t* x, int64_t M, int64_t K, uint8_t* codes, uint8_t* scales,
                               hipStream_t s);

// ---- mxfp4_mx.hip: W4A8 on the block-scaled MFMA. The contract is
// mxfp4_linear_tiled's / mxfp4_swiglu_tiled's in every respect except that x
// arrives quantized, as the codes [M, K] (contiguous, 16-B aligned) and scale
// bytes [M, K / 32] (contiguous) of mxfp8_quantize_rows: y[m][n] = sum_k x^[m][k]
// * W[n][k] with x^ = code * 2^(byte - 127), one f32 accumulator per element on
// v_mfma_scale_f32_16x16x128_f8f6f4 walking K in steps of 128 in ascending order
// (batch invariance; g and u of the gated kernel are the linear's f32 results bit
// for bit). A NaN code in x^ gives a NaN row and a weight scale byte 0xFF a NaN
// column. Nothing is read outside the two x arrays and the parameters' blocks and
// scale bytes, nothing written outside y[:M, :N]. One launch for any M,
// stream-ordered, no allocation, no workspace, no atomics.
constexpr int kMxfp4MxBM = 128, kMxfp4MxBN = 128;
hipError_t mxfp4_linear_mx(const void* packed, int64_t src_bytes, int64_t src_chunk, int64_t elem_off,
                           const uint8_t* x_codes, const uint8_t* x_scales, int64_t M, int64_t N, int64_t K, void* y,
                           int64_t ldy, bool y_bf16, hipStream_t s);
hipError_t mxfp4_swiglu_mx(const void* packed, int64_t src_bytes, int64_t src_chunk, int64_t gate_off, int64_t up_off,
                           const uint8_t* x_codes, const uint8_t* x_scales, int64_t M, int64_t N, int64_t K, void* y,
                           int64_t ldy, bool y_bf16, hipStream_t s);

// ---- fp8_linear.hip: the same product with W read in place from an fp8-packed
// layer (core/fp8.h: e4m3 codes and one power-of-two f32 scale per `block`
// elements, per source chunk; fp8::unpack_range_host defines where an element
// lies). The contract is mxfp4_linear's - x, y, ldy, M, N, K, elem_off (a
// multiple of 32), f32 accumulation on v_mfma_f32_16x16x32_bf16, `split_k`,
// `row_tiles_per_wave`, stream order, no allocation, no workspace, no atomics,
// equal inputs give equal bits - and in addition: `block` is 32, 64, 128, 256
// or 512; `src_chunk` is a multiple of 8 * block bytes (every packed chunk,
// n + 4 n / block bytes, then starts 16-B aligned); `src_bytes` a multiple of
// 2 * block; `packed` 16-B aligned. Anything else: hipErrorInvalidValue.
int fp8_linear_slices(int64_t M, int64_t N, int64_t K);
DecodePlan fp8_linear_plan(int m, int64_t N, int64_t K, int split_k, int row_tiles_per_wave);
hipError_t fp8_linear(const void* packed, int64_t src_bytes, int64_t src_chunk, int block, int64_t elem_off,
                      const uint16_t* x, int64_t M, int64_t N, int64_t K, void* y, int64_t ldy, bool y_bf16,
                      int split_k, int row_tiles_per_wave, hipStream_t s);

// ---- mxfp6_linear.hip: the same product with W read in place from an
// MXFP6-packed layer (core/mxfp6.h: 24 bytes of e2m3 codes and one E8M0 scale
// byte per 32 elements, per source chunk; mxfp6::unpack_range_host defines
// where an element lies). The contract is mxfp4_linear's - x, y, ldy, M, N, K,
// elem_off (a multiple of 32), f32 accumulation on v_mfma_f32_16x16x32_bf16,
// `split_k`, `row_tiles_per_wave`, stream order, no allocation, no workspace,
// no atomics, equal inputs give equal bits - with `src_chunk` a positive
// multiple of 1024 (every packed chunk, 25 bytes per 64, then starts 16-B
// aligned), `src_bytes` a positive multiple of 64 and `packed` 16-B aligned.
// Anything else: hipErrorInvalidValue.
int mxfp6_linear_slices(int64_t M, int64_t N, int64_t K);
DecodePlan mxfp6_linear_plan(int m, int64_t N, int64_t K, int split_k, int row_tiles_per_wave);
hipError_t mxfp6_linear(const void* packed, int64_t src_bytes, int64_t src_chunk, int64_t elem_off, const uint16_t* x,
                        int64_t M, int64_t N, int64_t K, void* y, int64_t ldy, bool y_bf16, int split_k,
                        int row_tiles_per_wave, hipStream_t s);

// ---- mxfp6_swiglu.hip, fp8_swiglu.hip: mxfp4_swiglu's y = silu(x * Wg^T) *
// (x * Wu^T) from an MXFP6- or an fp8-packed layer, Wg and Wu the [N, K]
// parameters at elements `gate_off` and `up_off` (independent multiples of 32 -
// for fp8 too, not of the block - in any order, possibly equal). Layer
// arguments, checks and accumulation are mxfp6_linear's / fp8_linear's, applied
// to both parameters; with equal K slices g and u are bit for bit that
// kernel's f32 results. Epilogue, `split_k` (0 = chosen, *_swiglu_slices; else
// 1..16, clamped), `row_tiles_per_wave` (pairs of a gate and an up tile: 0 =
// chosen, 1 or 2, a divisor of N / 16; 1 beyond 32 rows of x), stream order, no
// allocation, no workspace, no atomics: as for mxfp4_swiglu.
int mxfp6_swiglu_slices(int64_t M, int64_t N, int64_t K);
DecodePlan mxfp6_swiglu_plan(int m, int64_t N, int64_t K, int split_k, int row_tiles_per_wave);
hipError_t mxfp6_swiglu(const void* packed, int64_t src_bytes, int64_t src_chunk, int64_t gate_off, int64_t up_off,
                        const uint16_t* x, int64_t M, int64_t N, int64_t K, void* y, int64_t ldy, bool y_bf16,
                        int split_k, int row_tiles_per_wave, hipStream_t s);
int fp8_swiglu_slices(int64_t M, int64_t N, int64_t K);
DecodePlan fp8_swiglu_plan(int m, int64_t N, int64_t K, int split_k, int row_tiles_per_wave);
hipError_t fp8_swiglu(const void* packed, int64_t src_bytes, int64_t src_chunk, int block, int64_t gate_off,
                      int64_t up_off, const uint16_t* x, int64_t M, int64_t N, int64_t K, void* y, int64_t ldy,
                      bool y_bf16, int split_k, int row_tiles_per_wave, hipStream_t s);

// ---- mxfp6_tiled.hip, fp8_tiled.hip: mxfp4_tiled.hip's two kernels for many
// rows of x from an MXFP6- or an fp8-packed layer, each call ONE launch for any
// M: a workgroup owns BM rows of x by BN rows of W, stages x through LDS for its
// waves and dequantizes W in registers, so W is read and converted once per BM
// rows instead of once per 64. Layer arguments, x, y, ldy, M, N, K, `block`, the
// offsets and every hipErrorInvalidValue case are those of mxfp6_linear /
// mxfp6_swiglu / fp8_linear / fp8_swiglu (there is no `split_k` and no
// `row_tiles_per_wave`); in addition ceil(M / BM) * ceil(N / BN) (gated: BN / 2)
// must fit a 1-D grid. K is never split: every output element has one f32
// accumulator that walks K in the decode kernel's order, so the f32 results are
// bit for bit those of the decode kernel with split_k = 1, y[m][n] depends only
// on row m of x and row n of W (batch invariance), and g and u of the gated
// kernels are the tiled linear's f32 bits. Nothing is read outside x[0 : M K)
// and the parameters' codes and scales, nothing written outside y[:M, :N].
// Stream-ordered, no allocation, no workspace, no atomics.
constexpr int kMxfp6TiledBM = 128, kMxfp6TiledBN = 128, kFp8TiledBM = 128, kFp8TiledBN = 128;
hipError_t mxfp6_linear_tiled(const void* packed, int64_t src_bytes, int64_t src_chunk, int64_t elem_off,
                              const uint16_t* x, int64_t M, int64_t N, int64_t K, void* y, int64_t ldy, bool y_bf16,
                              hipStream_t s);
hipError_t mxfp6_swiglu_tiled(const void* packed, int64_t src_bytes, int64_t src_chunk, int64_t gate_off,
                              int64_t up_off, const uint16_t* x, int64_t M, int64_t N, int64_t K, void* y, int64_t ldy,
                              bool y_bf16, hipStream_t s);
hipError_t fp8_linear_tiled(const void* packed, int64_t src_bytes, int64_t src_chunk, int block, int64_t elem_off,
                            const uint16_t* x, int64_t M, int64_t N, int64_t K, void* y, int64_t ldy, bool y_bf16,
                            hipStream_t s);
hipError_t fp8_swiglu_tiled(const void* packed, int64_t src_bytes, int64_t src_chunk, int block, int64_t gate_off,
                            int64_t up_off, const uint16_t* x, int64_t M, int64_t N, int64_t K, void* y, int64_t ldy,
                            bool y_bf16, hipStream_t s);

// ---- attn_decode.hip: one decode step's attention against a KV cache in HBM.
// The caches are bf16 [B, kv_heads, capacity, d], contiguous and 16-B aligned,
// d 32, 64 or 128, capacity at most 2^20 positions; every cache index is 64-bit.
//
// attn_rope_append, ONE launch: for every sequence b with 0 <= pos[b] < capacity
// (pos int32 on the device), q_out[b, h] = rope(q[b, h]) at position pos[b]
// (q_out bf16 [B, heads, d], contiguous), k_cache[b, h, pos[b]] = rope(k[b, h])
// and v_cache[b, h, pos[b]] = v[b, h]. q, k and v are bf16 rows with unit stride
// and row strides ldq, ldk, ldv elements (three slices of one merged projection
// or three buffers). rope(x) = x * cos + rot(x) * sin in f32 from the tables cos,
// sin f32 [capacity, d]: two products and one sum, each rounded (no FMA), then
// one rounding to bf16. A pos[b] outside [0, capacity) writes nothing to the
// caches and a zero q_out row.
//
// attn_decode: y[b, h * d ...] = softmax(q[b, h] . K[b, h / group, :lens[b]] /
// sqrt(d)) V[b, h / group, :lens[b]] for q bf16 [B, heads, d] (contiguous, 16-B
// aligned), lens int32 [B] on the device with 0 <= lens[b] <= max_len <=
// capacity, group = heads / kv_heads in 1..16; y is [B, heads * d] f32 or bf16
// (the f32 result rounded to nearest even). lens[b] = 0 gives a zero row.
// Outside that promise both kernels clamp lens[b] to [0, capacity]: a negative
// one is a zero row, one above the capacity the row of the capacity; above
// max_len the row is that of the positions below lens[b] in the chunks that
// cover max_len (the combine kernel stops at the workspace's last chunk). No
// load leaves the caches, no store the workspace, and no other sequence's row
// changes. Finite scores of any size are exact in the softmax (an underflowed
// weight is exactly 0); bf16-subnormal V and f32-subnormal products are not
// flushed. Inside the valid prefix a NaN in a K row makes the rows of that (b,
// KV head)'s query heads NaN, +inf in a V element makes that d of those heads
// +inf where the position has weight and NaN (0 * inf) where its weight
// underflowed to 0; a head with a score that overflows f32 to +inf is NaN; the
// numerator sum(p~ v), p~ <= 1, is f32 and gives +-inf where it overflows
// before the division. Every other element keeps its bits. A workgroup serves one (b, KV head, chunk of
// kAttnDecodeChunk positions) and the KV head's whole group, so K and V rows are
// read once per KV head; scores and the online softmax are f32, P is rounded to
// bf16 for P V on v_mfma_f32_16x16x32_bf16; chunk partials (m, l, o) are f32 in
// `ws` (attn_decode_workspace_bytes, 16-B aligned; -1 for an unsupported shape)
// and a second launch merges them in ascending chunk order. Chunk c is positions
// [c * kAttnDecodeChunk, ...) whatever B, the other lens, max_len and capacity
// are, so row b is a function of q[b] and the valid K and V rows of b alone: the
// same bits in any batch. No position at or behind lens[b] is ever loaded.
// Stream-ordered, no allocation, no atomics. Anything else: hipErrorInvalidValue.
hipError_t attn_rope_append(const uint16_t* q, int64_t ldq, const uint16_t* k, int64_t ldk, const uint16_t* v,
                            int64_t ldv, const int32_t* pos, const float* cos, const float* sin, int64_t B,
                            int64_t heads, int64_t kv_heads, int64_t d, int64_t capacity, uint16_t* q_out,
                            uint16_t* k_cache, uint16_t* v_cache, hipStream_t s);
int64_t attn_decode_workspace_bytes(int64_t B, int64_t heads, int64_t kv_heads, int64_t d, int64_t capacity,
                                    int64_t max_len);
hipError_t attn_decode(const uint16_t* q, const uint16_t* k_cache, const uint16_t* v_cache, const int32_t* lens,
                       int64_t B, int64_t heads, int64_t kv_heads, int64_t d, int64_t capacity, int64_t max_len,
                       void* ws, int64_t ws_bytes, void* y, bool y_bf16, hipStream_t s);

}  // namespace kern
}  // namespace dissem
