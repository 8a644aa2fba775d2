// W4A8 linear and gated linear for many rows of x on the block-scaled MFMA,
// y = x^ * W^T and y = silu(x^ * Wg^T) * (x^ * Wu^T): the weights are read in place
// from an MXFP4-packed layer (core/mxfp4.h) and x^ arrives quantized to MXFP8
// (core/mxfp8_act.h: e4m3fn codes [M, K] and one E8M0 byte per 32 values,
// [M, K / 32]). Both go to v_mfma_scale_f32_16x16x128_f8f6f4 as they lie in
// memory - A = e4m3 (format 0), B = e2m1 (format 4), each with its scale byte -
// so nothing is dequantized on the VALU (the codes of x^ are only sorted into
// three classes by their exponent, see below). The tile shape, the grid and the
// pipeline are mxfp4_tiled.hip's: a workgroup owns BM = 128 rows of x by BN = 128
// rows of W, four waves, wave w owns the 16-row weight tiles 2w and 2w + 1 (gated:
// gate tile w and up tile w of the workgroup's 64 columns of y) in registers and
// applies each to all 8 row tiles of x, which is staged through LDS once per K
// step and shared by the four waves.
//
// The instruction, measured once on MI355X (csrc/tools/mxprobe.hip, output in
// profiles/mxfp4_mx/mxprobe.jsonl). Lane l = 16 g + c holds row (A) or column
// (B) c. B: nibble i (low nibble first) of the lane's 16 bytes is k = 32 g + i,
// the upper four dwords of the operand are not read, and the lane's scale byte
// reaches exactly these 32 values - a whole scale block of the packed layout.
// A is NOT 32 consecutive values: bytes 0..15 of lane group g are k = 16 g + i
// and bytes 16..31 are k = 64 + 16 g + (i - 16), while the scale of the block
// k in [32 b, 32 b + 32) still comes from the scale register of lane group b -
// so a lane carries the scale of block g of its row but the codes of two half
// blocks (of blocks g >> 1 and 2 + (g >> 1)). op_sel picks byte op_sel of the
// scale register (0 here). C/D is the bf16 form's: lane l, register i holds
// row 4 g + i, column c. A scale byte 0xFF on either side makes exactly the
// outputs of its row / column NaN, also where every code under it is zero, and
// so do the e4m3 codes 0x7F and 0xFF, also against a zero: a NaN in x is a NaN
// row and a 0xFF weight scale a NaN column with no help from the kernel.
// Scale bytes 0, 1 and 254 are 2^-127, 2^-126 and 2^127; nothing is flushed:
// products and sums that are f32 subnormals come out exact, and so does a
// subnormal C. Sums of exactly representable products below 2^24 are exact in
// any order of k - as long as the products of a group of 8 consecutive k lie
// close together: inside such a group a product 2^14 or more below the group's
// largest is dropped (2^-10 beside 2^4 is lost, beside 2^3 it is kept), while
// across groups, across scale blocks and against C an addend survives down to
// 2^-27 of the largest. One MFMA is therefore not an f32-accurate sum of its
// 128 products when one of them dominates its group: the error reaches 7 * 2^-14
// of that product, which K 2^-23 sum |x^ w^| does not cover (the down_proj of a
// decoder layer, whose input has outliers, missed it by 2.3 bounds). So the
// kernel never lets such products meet: every step runs THREE MFMAs per (row
// tile, weight tile), each with the e4m3 codes of one class of exponent field -
// f <= 5, 6..10, >= 11 - and +0 in the place of the others (split_classes).
// Within a class all bits of all products code * e2m1 lie within 2^12 of each
// other under one pair of scales, so each MFMA adds its groups exactly and what
// is left is the f32 accumulation across groups, blocks and steps.
// (core/mxfp4.h's dequantized weight is a bf16. It equals code * 2^(byte - 127),
// the value the instruction multiplies, for every code under every scale byte
// 0..254 - down to 2^-128, a bf16 subnormal - except the 12 pairs whose value
// reaches 2^128: the magnitudes 4 and 6 (nibbles 6, 7) under byte 253 and 2, 3,
// 4 and 6 (nibbles 4..7) under byte 254, either sign, which are +-inf on the
// host route and finite factors here.
// tests/test_mx_operands_host.py lists them.)
//
// K walk: steps of 128, three MFMAs (the classes, in ascending order) per (row
// tile, weight tile) per step. In step s
// lane (c, g) feeds, as B, the 16 B of q and the scale byte of block 4 s + g of
// weight row n0 + 16 j + c, and as A the codes x^[m0 + 16 t + c][128 s + 16 g ..
// + 16) and [128 s + 64 + 16 g .. + 16) with the scale byte of block 4 s + g of
// that row. The K % 128 tail is one more step of the same form whose absent
// blocks are codes 0 with scale byte 127 on both sides; they are never read
// from memory. Every output element has ONE accumulator, which takes the steps
// in ascending order and within a step the three classes: no split of K, no reduction, no atomics, no workspace.
// y[m][n] is a function of row m of x^ and row n of W alone (batch invariance,
// as for the tiled kernels), and g and u of the gated kernel are the linear's
// f32 results bit for bit.
//
// x^ in LDS: an image of a step is 128 rows x 128 B of codes, fragment-ordered,
// and 128 x 4 scale bytes. Piece (t, h) - row tile t, half h - is 1 KiB and
// holds, 16 B per lane, dwords 4 h .. 4 h + 3 of the A operand of the 64 lanes.
// Staging reads the codes coalesced (16-B loads, 8 lanes along the 128 B a row
// has in the step, 8 rows per wave-load) and scatters them into that order; the
// fragment read is two ds_read_b128 and one ds_read_u8 per row tile. c is XORed
// with 4 h + g (code_slot): a fragment read (16 lanes that hold every c once,
// half from an even and half from an odd g) finds 16 different slots and the
// 8 consecutive lanes of a staging store (one row, h = 0..1 and g = 0..3) find
// 8 different ones. The scale bytes of a row are one dword, [row][g]: a wave
// reads 64 consecutive bytes. Two images (2 * 16.5 KiB): the loads of step
// s + 1 (x^ into registers, the next weights) are issued before the MFMAs of
// step s and stored to the other image after them - one barrier per step.
// Rows at and beyond M are codes 0 / scale 127 in LDS and never read.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels/kernels.h"
#include "kernels/mxfp4_mma.h"
#include "kernels/tiled_x.h"

namespace dissem {
namespace kern {

namespace {

typedef int i32x8_t __attribute__((ext_vector_type(8)));

constexpr int kBM = kMxfp4MxBM, kBN = kMxfp4MxBN;
constexpr int kWaves = kTiledWaves;       // 256 threads
constexpr int kMT = kBM / 16;             // row tiles of x per workgroup
constexpr int kNT = kBN / 16 / kWaves;    // 16-row weight tiles per wave
constexpr int kStage = kBM / 8 / kWaves;  // 16-B code loads of a thread per step
constexpr uint32_t kOne = 127;            // the scale byte of 2^0
static_assert(kBM == 128 && kBN % (32 * kWaves) == 0, "tile shape");

// The 16-B slot of an image's codes that holds dwords 4 h .. 4 h + 3 of the A operand of lane (c, g)
// for row tile t.
__device__ __forceinline__ int code_slot(int t, int h, int g, int c) {
  return (t * 2 + h) * 64 + g * 16 + (c ^ (4 * h + g));
}

// The four e4m3 codes of a dword by the size of their exponent field f: c0 keeps the codes with
// f <= 5 (below 2^-1, the subnormals among them), c1 those with 6 <= f <= 10, c2 those with f >= 11
// (16 and more, the NaN codes among them); the others become +0. Every code is in exactly one.
// Within a class the products code * e2m1 span less than 2^13 from the lowest bit of the smallest
// to the largest (2^-10 .. 11.25 * 2^-2, 2^-5 .. 90, 2^0 .. 2688), which the adder of a group of 8
// holds exactly (the header).
__device__ __forceinline__ void split_classes(uint32_t w, uint32_t& c0, uint32_t& c1, uint32_t& c2) {
  const uint32_t f = (w >> 3) & 0x0F0F0F0Fu;
  const uint32_t m6 = (((f + 0x0A0A0A0Au) >> 4) & 0x01010101u) * 0xFFu;   // 0xFF where f >= 6
  const uint32_t m11 = (((f + 0x05050505u) >> 4) & 0x01010101u) * 0xFFu;  // 0xFF where f >= 11
  c0 = w & ~m6;
  c1 = w & m6 & ~m11;
  c2 = w & m11;
}

struct XImage {
  u32x4_t codes[kMT * 2 * 64];
  uint8_t scales[kBM * 4];
};

template <bool GATED, bool BF16>
__global__ void __launch_bounds__(64 * kWaves, 2)
    mxfp4_mx_kernel(Mxfp4Layout L, int64_t off0, int64_t off1, const uint8_t* __restrict__ xq,
                    const uint8_t* __restrict__ xs, int64_t M, int N, int K, void* __restrict__ y, int64_t ldy,
                    unsigned mblocks) {
  constexpr int NT = kNT, P = GATED ? kNT / 2 : kNT;
  __shared__ XImage img[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const unsigned lid = xcd_remap(blockIdx.x, gridDim.x);
  const unsigned nb = lid / mblocks, mb = lid - nb * mblocks;
  const int64_t m0 = int64_t(mb) * kBM;
  const int n0 = (int(nb) * kWaves + wave) * (16 * P);
  const int kblk = K >> 5, total = (kblk + 3) >> 2;

  // this lane's weight row per tile, in scale blocks; tiles beyond N read and store nothing
  int64_t row_blk[NT];
  bool valid[P];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    valid[j] = n0 + 16 * j < N;
    row_blk[j] = (off0 + int64_t(n0 + 16 * j + c) * K) >> 5;
    if (GATED) row_blk[P + j] = (off1 + int64_t(n0 + 16 * j + c) * K) >> 5;
  }

  f32x4_t acc[kMT][NT];
#pragma unroll
  for (int t = 0; t < kMT; ++t)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[t][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const u32x4_t zero4 = {0u, 0u, 0u, 0u};

  // Staging. Codes: load i of wave w covers rows 32 w + 8 i .. + 7, 8 lanes per row; this lane's 16 B
  // are bytes 16 sl .. 16 sl + 15 of the step: half sl >> 2 of lane group sl & 3. Scales: thread tid
  // takes the blocks 2 (tid & 1) and 2 (tid & 1) + 1 of row tid >> 1.
  const int sl = lane & 7, sr = wave * (8 * kStage) + (lane >> 3);
  const int zr = tid >> 1, zb = 2 * (tid & 1);
  u32x4_t st[kStage];
  uint32_t sc2;
  auto stage_load = [&](int s) {
    const bool kok = (s << 7) + 16 * sl < K;
    const uint8_t* src = xq + (m0 + sr) * K + ((s << 7) + 16 * sl);
#pragma unroll
    for (int i = 0; i < kStage; ++i)
      st[i] = kok && m0 + sr + 8 * i < M ? *reinterpret_cast<const u32x4_t*>(src + int64_t(8 * i) * K) : zero4;
    const int b = 4 * s + zb;
    const bool rok = m0 + zr < M;
    const uint8_t* ss = xs + (m0 + zr) * kblk + b;
    const uint32_t lo = rok && b < kblk ? ss[0] : kOne, hi = rok && b + 1 < kblk ? ss[1] : kOne;
    sc2 = lo | (hi << 8);
  };
  auto stage_store = [&](XImage& im) {
#pragma unroll
    for (int i = 0; i < kStage; ++i) {
      const int r = sr + 8 * i;
      im.codes[code_slot(r >> 4, sl >> 2, sl & 3, r & 15)] = st[i];
    }
    *reinterpret_cast<uint16_t*>(&im.scales[zr * 4 + zb]) = uint16_t(sc2);
  };

  // weights: the block of this lane in the current step, registers only
  BlockPos pos[NT];
  u32x4_t qn[NT];
  uint32_t sn[NT];
  auto weights_load = [&](int s, bool first) {
    const bool bok = 4 * s + g < kblk;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      qn[j] = zero4;
      sn[j] = kOne;
      if (valid[j % P] && bok) {
        if (first) pos[j].init(L, row_blk[j] + g);
        else pos[j].advance(L, 4);
        qn[j] = *reinterpret_cast<const u32x4_t*>(pos[j].q());
        sn[j] = pos[j].scale();
      }
    }
  };
  weights_load(0, true);
  stage_load(0);
  stage_store(img[0]);
  __syncthreads();

  for (int s = 0; s < total; ++s) {
    const XImage& im = img[s & 1];
    if (s + 1 < total) stage_load(s + 1);
    i32x8_t b[NT];
    int sb[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      b[j] = i32x8_t{int(qn[j][0]), int(qn[j][1]), int(qn[j][2]), int(qn[j][3]), 0, 0, 0, 0};
      sb[j] = int(sn[j]);
    }
    // the next step's weights are in flight during this one. A lane whose block lies beyond K in
    // step s + 1 (the tail) keeps its position: it is in the last step and never advances again.
    if (s + 1 < total) weights_load(s + 1, false);
#pragma unroll
    for (int t = 0; t < kMT; ++t) {
      const u32x4_t lo = im.codes[code_slot(t, 0, g, c)], hi = im.codes[code_slot(t, 1, g, c)];
      const int sa = im.scales[(16 * t + c) * 4 + g];
      const uint32_t w[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      i32x8_t a[3];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        uint32_t c0, c1, c2;
        split_classes(w[i], c0, c1, c2);
        a[0][i] = int(c0);
        a[1][i] = int(c1);
        a[2][i] = int(c2);
      }
#pragma unroll
      for (int cl = 0; cl < 3; ++cl)
#pragma unroll
        for (int j = 0; j < NT; ++j)
          acc[t][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[cl], b[j], acc[t][j], 0, 4, 0, sa, 0, sb[j]);
    }
    if (s + 1 < total) {
      stage_store(img[(s + 1) & 1]);
      __syncthreads();
    }
  }

#pragma unroll
  for (int j = 0; j < P; ++j) {
    if (!valid[j]) continue;
#pragma unroll
    for (int t = 0; t < kMT; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t m = m0 + 16 * t + 4 * g + i;
        if (m < M)
          store_y<BF16>(y, m * ldy + n0 + 16 * j + c,
                        GATED ? swiglu(acc[t][j][i], acc[t][GATED ? P + j : j][i]) : acc[t][j][i]);
      }
  }
}

bool layer_ok(const void* packed, int64_t src_bytes, int64_t src_chunk, const uint8_t* xq, const uint8_t* xs, int64_t M,
              int64_t N, int64_t K, const void* y, int64_t ldy, bool y_bf16) {
  if (src_chunk <= 0 || src_chunk % 1024 || src_bytes <= 0 || src_bytes % 64) return false;
  if (M < 1 || N < 16 || N % 16 || K < 32 || K % 32 || K > 0x7FFFFF80 || N > 0x7FFFFFF0 || ldy < N) return false;
  if ((reinterpret_cast<uintptr_t>(packed) & 15) || (reinterpret_cast<uintptr_t>(xq) & 15) || !xs ||
      (reinterpret_cast<uintptr_t>(y) & (y_bf16 ? 1 : 3)))
    return false;
  return src_chunk / 64 <= 0x7FFFFFFF;
}

bool param_ok(int64_t off, int64_t src_bytes, int64_t N, int64_t K) {
  return off >= 0 && off % 32 == 0 && N <= (src_bytes / 2 - off) / K;
}

template <bool GATED>
hipError_t launch(const void* packed, int64_t src_bytes, int64_t src_chunk, int64_t off0, int64_t off1,
                  const uint8_t* xq, const uint8_t* xs, int64_t M, int64_t N, int64_t K, void* y, int64_t ldy,
                  bool y_bf16, hipStream_t s) {
  constexpr int cols = GATED ? kBN / 2 : kBN;  // columns of y per workgroup
  const int64_t mblocks = (M + kBM - 1) / kBM, nblocks = (N + cols - 1) / cols;
  if (mblocks > 0x7FFFFFFF / nblocks) return hipErrorInvalidValue;  // one launch: the grid is 1-D
  const Mxfp4Layout L = mxfp4_layout(packed, src_bytes, src_chunk);
  const dim3 grid{unsigned(mblocks * nblocks)}, block{64 * kWaves};
  if (y_bf16)
    mxfp4_mx_kernel<GATED, true><<<grid, block, 0, s>>>(L, off0, off1, xq, xs, M, int(N), int(K), y, ldy, unsigned(mblocks));
  else
    mxfp4_mx_kernel<GATED, false><<<grid, block, 0, s>>>(L, off0, off1, xq, xs, M, int(N), int(K), y, ldy, unsigned(mblocks));
  return hipGetLastError();
}

}  // namespace

hipError_t mxfp4_linear_mx(const void* packed, int64_t src_bytes, int64_t src_chunk, int64_t elem_off,
                           const uint8_t* x_codes, const uint8_t* x_scales, int64_t M, int64_t N, int64_t K, void* y,
                           int64_t ldy, bool y_bf16, hipStream_t s) {
  if (!layer_ok(packed, src_bytes, src_chunk, x_codes, x_scales, M, N, K, y, ldy, y_bf16)) return hipErrorInvalidValue;
  if (!param_ok(elem_off, src_bytes, N, K)) return hipErrorInvalidValue;
  return launch<false>(packed, src_bytes, src_chunk, elem_off, elem_off, x_codes, x_scales, M, N, K, y, ldy, y_bf16, s);
}

hipError_t mxfp4_swiglu_mx(const void* packed, int64_t src_bytes, int64_t src_chunk, int64_t gate_off, int64_t up_off,
                           const uint8_t* x_codes, const uint8_t* x_scales, int64_t M, int64_t N, int64_t K, void* y,
                           int64_t ldy, bool y_bf16, hipStream_t s) {
  if (!layer_ok(packed, src_bytes, src_chunk, x_codes, x_scales, M, N, K, y, ldy, y_bf16)) return hipErrorInvalidValue;
  if (!param_ok(gate_off, src_bytes, N, K) || !param_ok(up_off, src_bytes, N, K)) return hipErrorInvalidValue;
  return launch<true>(packed, src_bytes, src_chunk, gate_off, up_off, x_codes, x_scales, M, N, K, y, ldy, y_bf16, s);
}

}  // namespace kern
}  // namespace dissem
