// mxprobe: what gfx950's block-scaled matrix instruction computes (ISA semantics
// probe), for the form kernels/mxfp4_mx.hip issues:
// v_mfma_scale_f32_16x16x128_f8f6f4 with A = e4m3 (format 0) and B = e2m1
// (format 4). Every experiment is one wave and one instruction; the data are
// small integers (exact in every format involved) with an asymmetric B, so a
// wrong operand map cannot hide. Prints one JSON line per question:
//   a_row / b_col   one-hot A byte (B nibble): the row (column) of D it reaches
//   k_pairing       which B nibble a given A byte is multiplied with
//   scale_*_reach   the lane group whose scale register reaches a byte (nibble)
//   map_verify      random A, B under the maps found against a host model
//   cd_map          the lanes and registers of D for one row and one column
//   opsel_a/b       the byte of the scale register that op_sel picks
//   scale_scope     one lane's scale doubled, against the model
//   special         0xFF / 0 / 1 / 254 scale bytes, e4m3 NaN codes, subnormals
//   accum_exact     sums of exact products below 2^24, in two orders of k
//   accum_align     how far below the largest addend (a product, or C) a product survives
// The expectation it started from: lane l holds row (A) or column (B) l & 15
// and k = 32 (l >> 4) + i, i = byte i of A's 32 bytes, nibble i (low nibble
// first) of B's low 16 bytes, a lane's scale byte reaching its own 32 values; D
// is the bf16 form's (lane l, register i: row 4 (l >> 4) + i, column l & 15).
// k is counted by B's places, so k_pairing and scale_a_reach show where A
// departs from it (on MI355X: bytes 0..15 of lane group g are k = 16 g + i and
// bytes 16..31 are k = 64 + 16 g + (i - 16), while the scale of k block b still
// comes from lane group b). The model then runs on the maps found.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct Exp {
  uint32_t a[64][8], b[64][8], sa[64], sb[64];
  float c;
  int oa, ob;
};

template <int OA, int OB>
__device__ f32x4 mx(i32x8 a, i32x8 b, f32x4 c, int sa, int sb) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 4, OA, sa, OB, sb);
}

__global__ void __launch_bounds__(64) run(const Exp* __restrict__ e, float* __restrict__ d) {
  const Exp& x = e[blockIdx.x];
  const int l = threadIdx.x;
  i32x8 a, b;
  for (int i = 0; i < 8; ++i) {
    a[i] = int(x.a[l][i]);
    b[i] = int(x.b[l][i]);
  }
  const f32x4 c = {x.c, x.c, x.c, x.c};
  const int sa = int(x.sa[l]), sb = int(x.sb[l]);
  f32x4 r;
  switch (x.oa * 4 + x.ob) {
    case 0: r = mx<0, 0>(a, b, c, sa, sb); break;
    case 1: r = mx<0, 1>(a, b, c, sa, sb); break;
    case 2: r = mx<0, 2>(a, b, c, sa, sb); break;
    case 3: r = mx<0, 3>(a, b, c, sa, sb); break;
    case 4: r = mx<1, 0>(a, b, c, sa, sb); break;
    case 8: r = mx<2, 0>(a, b, c, sa, sb); break;
    default: r = mx<3, 0>(a, b, c, sa, sb); break;
  }
  for (int i = 0; i < 4; ++i) d[(int64_t(blockIdx.x) * 64 + l) * 4 + i] = r[i];
}

// ---- host side: the formats and the model under the expected maps
static double e4m3(uint8_t q) {
  const int e = (q >> 3) & 15, m = q & 7;
  if (e == 15 && m == 7) return NAN;
  const double v = e ? std::ldexp(8 + m, e - 10) : std::ldexp(m, -9);
  return q & 0x80 ? -v : v;
}
static double e2m1(uint32_t q) {
  static const double t[8] = {0, 0.5, 1, 1.5, 2, 3, 4, 6};
  return q & 8 ? -t[q & 7] : t[q & 7];
}
static uint8_t int_code(int v) {  // e4m3 code of an integer in [-8, 8]
  static const uint8_t t[9] = {0x00, 0x38, 0x40, 0x44, 0x48, 0x4A, 0x4C, 0x4E, 0x50};
  return v < 0 ? uint8_t(0x80 | t[-v]) : t[v];
}
static uint32_t byte_of(const uint32_t* w, int i) { return (w[i >> 2] >> (8 * (i & 3))) & 0xFFu; }
static uint32_t nib_of(const uint32_t* w, int i) { return (w[i >> 3] >> (4 * (i & 7))) & 0xFu; }
static void set_byte(uint32_t* w, int i, uint32_t v) {
  w[i >> 2] = (w[i >> 2] & ~(0xFFu << (8 * (i & 3)))) | (v << (8 * (i & 3)));
}
static void set_nib(uint32_t* w, int i, uint32_t v) {
  w[i >> 3] = (w[i >> 3] & ~(0xFu << (4 * (i & 7)))) | (v << (4 * (i & 7)));
}

// The maps the model uses, found by the one-hot experiments below before anything is verified (the
// expectation until then): byte i of A in lane group g is multiplied with the B nibble whose place
// is k = 32 (its lane group) + (its index), ka[g][i]; sga / sgb: the lane group whose scale register
// reaches byte (nibble) i of lane group g.
static int ka[4][32], sga[4][32], sgb[4][32];
static void expected_maps() {
  for (int g = 0; g < 4; ++g)
    for (int i = 0; i < 32; ++i) ka[g][i] = 32 * g + i, sga[g][i] = sgb[g][i] = g;
}

// D[r][c] under those maps, scale byte = byte op_sel of the lane's scale register
static void model(const Exp& x, float out[16][16]) {
  for (int r = 0; r < 16; ++r)
    for (int c = 0; c < 16; ++c) {
      double s = x.c;
      for (int g = 0; g < 4; ++g)
        for (int i = 0; i < 32; ++i) {
          const int k = ka[g][i], gb = k >> 5, ib = k & 31;
          const int ea = int((x.sa[r + 16 * sga[g][i]] >> (8 * x.oa)) & 0xFF) - 127;
          const int eb = int((x.sb[c + 16 * sgb[gb][ib]] >> (8 * x.ob)) & 0xFF) - 127;
          s += std::ldexp(e4m3(uint8_t(byte_of(x.a[r + 16 * g], i))), ea) *
               std::ldexp(e2m1(nib_of(x.b[c + 16 * gb], ib)), eb);
        }
      out[r][c] = float(s);
    }
}
static float at(const float* d, int r, int c) { return d[(c + 16 * (r >> 2)) * 4 + (r & 3)]; }
static uint32_t bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}
static int mismatches(const Exp& x, const float* d) {
  float m[16][16];
  model(x, m);
  int bad = 0;
  for (int r = 0; r < 16; ++r)
    for (int c = 0; c < 16; ++c) bad += bits(m[r][c]) != bits(at(d, r, c));
  return bad;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return uint32_t(rng_state >> 33);
}

static Exp blank() {
  Exp x;
  memset(&x, 0, sizeof x);
  for (int l = 0; l < 64; ++l) x.sa[l] = x.sb[l] = 0x7F7F7F7Fu;
  return x;
}
static void fill_a(Exp& x, uint32_t code) {
  for (int l = 0; l < 64; ++l)
    for (int i = 0; i < 8; ++i) x.a[l][i] = code * 0x01010101u;
}
static void fill_b(Exp& x, uint32_t code) {
  for (int l = 0; l < 64; ++l)
    for (int i = 0; i < 4; ++i) x.b[l][i] = code * 0x11111111u;
}
static Exp random_ints(int sa_spread, int sb_spread) {
  Exp x = blank();
  for (int l = 0; l < 64; ++l) {
    for (int i = 0; i < 32; ++i) set_byte(x.a[l], i, int_code(int(rnd() % 17) - 8));
    for (int i = 0; i < 32; ++i) set_nib(x.b[l], i, rnd() & 15);
    for (int i = 4; i < 8; ++i) x.b[l][i] = rnd();  // expected unused
    x.sa[l] = (127 + (sa_spread ? rnd() % (sa_spread + 1) : 0)) * 0x01010101u;
    x.sb[l] = (127 + (sb_spread ? rnd() % (sb_spread + 1) : 0)) * 0x01010101u;
  }
  return x;
}

static std::vector<float> execute(const std::vector<Exp>& v) {
  Exp* de;
  float* dd;
  std::vector<float> out(v.size() * 256);
  if (hipMalloc(&de, v.size() * sizeof(Exp)) != hipSuccess || hipMalloc(&dd, out.size() * 4) != hipSuccess) exit(2);
  hipMemcpy(de, v.data(), v.size() * sizeof(Exp), hipMemcpyHostToDevice);
  run<<<unsigned(v.size()), 64>>>(de, dd);
  if (hipMemcpy(out.data(), dd, out.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) exit(2);
  hipFree(de);
  hipFree(dd);
  return out;
}

// rows / columns of D that hold a NaN, as 16-bit masks, the NaN count and one value that is none
static void summary(const char* name, const float* d) {
  unsigned rows = 0, cols = 0;
  int nans = 0;
  float other = 0.f;
  for (int r = 0; r < 16; ++r)
    for (int c = 0; c < 16; ++c) {
      const float v = at(d, r, c);
      if (v != v) rows |= 1u << r, cols |= 1u << c, ++nans;
      else other = v;
    }
  printf("{\"op\": \"special\", \"case\": \"%s\", \"nan_outputs\": %d, \"nan_rows\": \"0x%04x\", \"nan_cols\": "
         "\"0x%04x\", \"d00\": \"0x%08x\", \"d_3_9\": \"0x%08x\", \"a_non_nan\": \"0x%08x\"}\n",
         name, nans, rows, cols, bits(at(d, 0, 0)), bits(at(d, 3, 9)), bits(other));
}

int main() {
  expected_maps();
  // 2. one-hot A byte / B nibble: where it lands in D
  for (int side = 0; side < 2; ++side) {
    std::vector<Exp> v;
    for (int l = 0; l < 64; ++l)
      for (int i = 0; i < 32; ++i) {
        Exp x = blank();
        if (side == 0) {
          fill_b(x, 2);
          set_byte(x.a[l], i, 0x38);
        } else {
          fill_a(x, 0x38);
          set_nib(x.b[l], i, 2);
        }
        v.push_back(x);
      }
    const auto d = execute(v);
    int bad = 0, fl = -1, fi = -1, fgot = -1;
    for (int e = 0; e < 2048; ++e) {
      const int want = (e >> 5) & 15;
      int got = -1, n = 0;
      for (int r = 0; r < 16; ++r)
        for (int c = 0; c < 16; ++c)
          if (at(&d[e * 256], r, c) == 1.0f) ++n, got = side == 0 ? r : c;
          else if (at(&d[e * 256], r, c) != 0.0f) n += 100;
      if (n != 16 || got != want) {
        if (!bad) fl = e >> 5, fi = e & 31, fgot = got;
        ++bad;
      }
    }
    printf("{\"op\": \"%s\", \"positions\": 2048, \"expected\": \"lane & 15\", \"deviations\": %d, \"first\": "
           "{\"lane\": %d, \"index\": %d, \"got\": %d}}\n", side == 0 ? "a_row" : "b_col", bad, fl, fi, fgot);
  }
  // 3. the k of B that an A byte meets: B nibble (lane, i) holds bit p of 32 (lane >> 4) + i
  {
    std::vector<Exp> v;
    for (int l = 0; l < 64; ++l)
      for (int i = 0; i < 32; ++i)
        for (int p = 0; p < 7; ++p) {
          Exp x = blank();
          set_byte(x.a[l], i, 0x38);
          for (int lb = 0; lb < 64; ++lb)
            for (int ib = 0; ib < 32; ++ib)
              if (((32 * (lb >> 4) + ib) >> p) & 1) set_nib(x.b[lb], ib, 2);
          v.push_back(x);
        }
    const auto d = execute(v);
    // the table from row 0; the other rows are held against it
    int bad = 0, expect_bad = 0;
    for (int e = 0; e < 2048; ++e) {
      const int r = (e >> 5) & 15, g = e >> 9, i = e & 31;
      int got = 0;
      bool uniform = true;
      for (int p = 0; p < 7; ++p) {
        const float* dd = &d[(e * 7 + p) * 256];
        const float v0 = at(dd, r, 0);
        for (int c = 1; c < 16; ++c) uniform &= at(dd, r, c) == v0;
        if (v0 == 1.0f) got |= 1 << p;
        else uniform &= v0 == 0.0f;
      }
      if (r == 0) ka[g][i] = got;
      bad += !uniform || got != ka[g][i];
      expect_bad += got != 32 * g + i;
    }
    printf("{\"op\": \"k_pairing\", \"positions\": 2048, \"deviations_from_32g_plus_i\": %d, "
           "\"rows_that_differ_from_row_0\": %d, \"b_place_met_by_a_byte\": [", expect_bad, bad);
    for (int g = 0; g < 4; ++g) {
      printf("%s[", g ? ", " : "");
      for (int i = 0; i < 32; ++i) printf("%s%d", i ? ", " : "", ka[g][i]);
      printf("]");
    }
    printf("]}\n");
  }
  // 3b. whose scale register reaches a byte of A (a nibble of B): one-hot value, one lane group's scale doubled
  for (int side = 0; side < 2; ++side) {
    std::vector<Exp> v;
    for (int l = 0; l < 64; ++l)
      for (int i = 0; i < 32; ++i)
        for (int gs = 0; gs < 4; ++gs) {
          Exp x = blank();
          if (side == 0) {
            fill_b(x, 2);
            set_byte(x.a[l], i, 0x38);
            x.sa[(l & 15) + 16 * gs] = 0x80808080u;
          } else {
            fill_a(x, 0x38);
            set_nib(x.b[l], i, 2);
            x.sb[(l & 15) + 16 * gs] = 0x80808080u;
          }
          v.push_back(x);
        }
    const auto d = execute(v);
    int(*tab)[32] = side == 0 ? sga : sgb;
    int bad = 0, expect_bad = 0;
    for (int e = 0; e < 2048; ++e) {
      const int rc = (e >> 5) & 15, g = e >> 9, i = e & 31;
      int got = -1, n = 0;
      for (int gs = 0; gs < 4; ++gs) {
        const float* dd = &d[(e * 4 + gs) * 256];
        const float v0 = side == 0 ? at(dd, rc, 0) : at(dd, 0, rc);
        if (v0 == 2.0f) got = gs, ++n;
        else if (v0 != 1.0f) n += 100;
      }
      if (n != 1) got = -1;
      if (rc == 0) tab[g][i] = got;
      bad += got < 0 || got != tab[g][i];
      expect_bad += got != g;
    }
    printf("{\"op\": \"%s\", \"positions\": 2048, \"deviations_from_own_lane_group\": %d, "
           "\"rows_that_differ_from_row_0\": %d, \"lane_group_of_the_scale\": [",
           side == 0 ? "scale_a_reach" : "scale_b_reach", expect_bad, bad);
    for (int g = 0; g < 4; ++g) {
      printf("%s[", g ? ", " : "");
      for (int i = 0; i < 32; ++i) printf("%s%d", i ? ", " : "", tab[g][i]);
      printf("]");
    }
    printf("]}\n");
    for (int g = 0; g < 4; ++g)
      for (int i = 0; i < 32; ++i)
        if (tab[g][i] < 0) tab[g][i] = g;
  }
  // 3c. random A and B under the maps found, against the model
  {
    std::vector<Exp> v;
    for (int i = 0; i < 8; ++i) v.push_back(random_ints(0, 0));
    const auto d = execute(v);
    int bad = 0;
    for (size_t i = 0; i < v.size(); ++i) bad += mismatches(v[i], &d[i * 256]);
    printf("{\"op\": \"map_verify\", \"outputs\": %zu, \"mismatches\": %d}\n", v.size() * 256, bad);
  }
  // 4. C/D: A row 3 and B column 9 set, everything else zero
  {
    Exp x = blank();
    for (int g = 0; g < 4; ++g)
      for (int i = 0; i < 8; ++i) x.a[3 + 16 * g][i] = 0x38383838u;
    for (int g = 0; g < 4; ++g)
      for (int i = 0; i < 4; ++i) x.b[9 + 16 * g][i] = 0x22222222u;
    const auto d = execute({x});
    printf("{\"op\": \"cd_map\", \"a_row\": 3, \"b_col\": 9, \"nonzero\": [");
    bool first = true;
    for (int l = 0; l < 64; ++l)
      for (int i = 0; i < 4; ++i)
        if (d[l * 4 + i] != 0.f) {
          printf("%s{\"lane\": %d, \"reg\": %d, \"value\": %g}", first ? "" : ", ", l, i, d[l * 4 + i]);
          first = false;
        }
    printf("], \"expected\": {\"lane\": 9, \"reg\": 3, \"value\": 128}}\n");
  }
  // 5. op_sel: scale bytes 125, 127, 128, 130 in bytes 0..3 of one side's register
  for (int side = 0; side < 2; ++side) {
    std::vector<Exp> v;
    for (int o = 0; o < 4; ++o) {
      Exp x = blank();
      fill_a(x, 0x38);
      fill_b(x, 2);
      for (int l = 0; l < 64; ++l) (side == 0 ? x.sa : x.sb)[l] = 0x82807F7Du;
      (side == 0 ? x.oa : x.ob) = o;
      v.push_back(x);
    }
    const auto d = execute(v);
    printf("{\"op\": \"%s\", \"scale_register\": \"0x82807f7d\", \"log2_scale_by_op_sel\": [%g, %g, %g, %g], "
           "\"expected\": [-2, 0, 1, 3]}\n", side == 0 ? "opsel_a" : "opsel_b", std::log2(d[0] / 128.0),
           std::log2(d[256] / 128.0), std::log2(d[512] / 128.0), std::log2(d[768] / 128.0));
  }
  // 6. one lane's scale doubled: its row (column) gains 32 and nothing else moves
  {
    std::vector<Exp> v;
    for (int side = 0; side < 2; ++side)
      for (int l = 0; l < 64; ++l) {
        Exp x = random_ints(0, 0);
        (side == 0 ? x.sa : x.sb)[l] = 0x80808080u;
        v.push_back(x);
      }
    const auto d = execute(v);
    int bad = 0;
    for (size_t i = 0; i < v.size(); ++i) bad += mismatches(v[i], &d[i * 256]);
    printf("{\"op\": \"scale_scope\", \"experiments\": %zu, \"outputs\": %zu, \"mismatches\": %d}\n", v.size(),
           v.size() * 256, bad);
  }
  // 7. special inputs, printed as they come
  {
    struct Case {
      const char* name;
      Exp x;
    };
    std::vector<Case> cs;
    auto ones = [] {
      Exp x = blank();
      fill_a(x, 0x38);
      fill_b(x, 2);
      return x;
    };
    Exp x = ones();
    x.sa[5] = 0xFFFFFFFFu;
    cs.push_back({"scale_a_0xff_lane5", x});
    x = ones();
    x.sb[21] = 0xFFFFFFFFu;
    cs.push_back({"scale_b_0xff_lane21", x});
    x = ones();
    x.sb[21] = 0xFFFFFFFFu;
    for (int i = 0; i < 4; ++i) x.b[21][i] = 0;
    cs.push_back({"scale_b_0xff_lane21_codes_zero", x});
    x = ones();
    x.sb[21] = 0xFFFFFFFFu;
    for (int i = 0; i < 8; ++i) x.a[16 + 3][i] = 0;  // the A values of row 3 that meet it are zero
    cs.push_back({"scale_b_0xff_lane21_a_row3_zero", x});
    x = ones();
    for (int l = 0; l < 64; ++l) x.sa[l] = 0, x.sb[l] = 0xFEFEFEFEu;
    cs.push_back({"scale_a_0_b_254_expect_128", x});
    x = ones();
    for (int l = 0; l < 64; ++l) x.sa[l] = 0;
    cs.push_back({"scale_a_0_b_127_expect_2^-120", x});
    x = ones();
    for (int l = 0; l < 64; ++l) x.sa[l] = 0x01010101u;
    cs.push_back({"scale_a_1_b_127_expect_2^-119", x});
    x = ones();
    for (int l = 0; l < 64; ++l) x.sb[l] = 0;
    cs.push_back({"scale_b_0_a_127_expect_2^-120", x});
    x = ones();
    for (int l = 0; l < 64; ++l) x.sa[l] = 0xFEFEFEFEu, x.sb[l] = 0x78787878u;
    cs.push_back({"scale_a_254_b_120_expect_2^127", x});
    x = ones();
    for (int l = 0; l < 64; ++l) x.sa[l] = 0xFEFEFEFEu, x.sb[l] = 0xFEFEFEFEu;
    cs.push_back({"scale_a_254_b_254_expect_inf", x});
    x = ones();
    set_byte(x.a[2], 7, 0x7F);
    cs.push_back({"a_code_0x7f_lane2", x});
    x = ones();
    set_byte(x.a[2], 7, 0xFF);
    cs.push_back({"a_code_0xff_lane2", x});
    x = ones();
    set_byte(x.a[2], 7, 0x7F);
    set_nib(x.b[9], 7, 0);  // the B value of column 9 that meets it is zero
    cs.push_back({"a_code_0x7f_lane2_b_col9_zero", x});
    // subnormals: A = 2^-9 * 2^-100, B = 0.5 * 2^-20: every product 2^-130
    x = blank();
    fill_a(x, 0x01);
    fill_b(x, 1);
    for (int l = 0; l < 64; ++l) x.sa[l] = 27 * 0x01010101u, x.sb[l] = 107 * 0x01010101u;
    cs.push_back({"128_products_2^-130_expect_2^-123", x});
    x = blank();
    set_byte(x.a[0], 0, 0x01);
    fill_b(x, 1);
    for (int l = 0; l < 64; ++l) x.sa[l] = 27 * 0x01010101u, x.sb[l] = 107 * 0x01010101u;
    cs.push_back({"one_product_2^-130_row0", x});
    x = blank();
    set_byte(x.a[0], 0, 0x01);
    fill_b(x, 1);
    for (int l = 0; l < 64; ++l) x.sa[l] = 29 * 0x01010101u, x.sb[l] = 107 * 0x01010101u;
    cs.push_back({"one_product_2^-128_row0", x});
    x = blank();
    x.c = std::ldexp(1.0f, -140);
    cs.push_back({"c_2^-140_no_products", x});
    x = blank();
    x.c = std::ldexp(1.0f, -140);
    set_byte(x.a[0], 0, 0x01);
    fill_b(x, 1);
    for (int l = 0; l < 64; ++l) x.sa[l] = 17 * 0x01010101u, x.sb[l] = 107 * 0x01010101u;
    cs.push_back({"c_2^-140_plus_product_2^-140_row0", x});
    std::vector<Exp> v;
    for (auto& c : cs) v.push_back(c.x);
    const auto d = execute(v);
    for (size_t i = 0; i < cs.size(); ++i) summary(cs[i].name, &d[i * 256]);
  }
  // 8. accumulation: integer A with scales 2^0..2^6, B with 2^0..2^2: every product a multiple of 0.5 below
  // 2^14, every sum below 2^21; then the same data with k reversed inside every group of 16 (a permutation of
  // k under the expected map and under the one found)
  {
    std::vector<Exp> v;
    for (int i = 0; i < 16; ++i) {
      const Exp x = random_ints(6, 2);
      Exp y = x;
      for (int l = 0; l < 64; ++l)
        for (int k = 0; k < 32; ++k) {
          set_byte(y.a[l], k, byte_of(x.a[l], k ^ 15));
          set_nib(y.b[l], k, nib_of(x.b[l], k ^ 15));
        }
      v.push_back(x);
      v.push_back(y);
    }
    const auto d = execute(v);
    int bad = 0, order = 0;
    for (size_t i = 0; i < v.size(); ++i) bad += mismatches(v[i], &d[i * 256]);
    for (size_t i = 0; i < v.size(); i += 2) order += memcmp(&d[i * 256], &d[(i + 1) * 256], 1024) != 0;
    printf("{\"op\": \"accum_exact\", \"outputs\": %zu, \"mismatches_against_exact_sum\": %d, "
           "\"pairs_that_differ_when_k_is_permuted\": %d}\n", v.size() * 256, bad, order);
  }
  // 9. how far below the largest addend a product survives: (a) one product 2^t (block 0 of row 0: one
  // code 1.0 under scale byte 127 + t, the rest of the block zero) next to 96 products of 1 in the
  // other blocks, (b) C = 2^t and 128 products of 1. Printed: the sum minus 2^t, which is 96 or
  // 128 as long as nothing is cut; f32 itself holds 2^t + 128 exactly up to t = 23.
  {
    std::vector<Exp> v;
    for (int t = 0; t <= 30; ++t) {
      Exp x = blank();
      fill_b(x, 2);
      for (int g = 0; g < 4; ++g)  // k = 32 .. 127 of row 0 under the A map found: bytes 16..31 of every lane group,
        for (int i = (g < 2 ? 4 : 0); i < 8; ++i) x.a[16 * g][i] = 0x38383838u;  // bytes 0..15 of groups 2 and 3
      set_byte(x.a[0], 0, 0x38);
      x.sa[0] = uint32_t(127 + t) * 0x01010101u;
      v.push_back(x);
      Exp y = blank();
      fill_b(y, 2);
      for (int g = 0; g < 4; ++g)
        for (int i = 0; i < 8; ++i) y.a[16 * g][i] = 0x38383838u;
      y.c = std::ldexp(1.0f, t);
      v.push_back(y);
    }
    const auto d = execute(v);
    for (int side = 0; side < 2; ++side) {
      printf("{\"op\": \"accum_align\", \"case\": \"%s\", \"sum_minus_2^t_for_t_0_to_30\": [",
             side == 0 ? "one_product_2^t_and_96_products_of_1" : "c_2^t_and_128_products_of_1");
      for (int t = 0; t <= 30; ++t)
        printf("%s%.10g", t ? ", " : "", double(at(&d[(2 * t + side) * 256], 0, 0)) - std::ldexp(1.0, t));
      printf("]}\n");
    }
  }
  // 10. the same inside ONE scale block, where the span comes from the codes themselves: k = 0 of row 0
  // holds the e4m3 code 2^(j - 7), j = 1..15, against the e2m1 code 1 or 4, and k = 1..31 hold 2^-9
  // against 0.5: one product 2^u, u = -6..10, and 31 products of 2^-10 under equal scales. Printed:
  // (sum - 2^u) * 2^10, which is 31 as long as nothing is cut.
  {
    std::vector<Exp> v;
    std::vector<int> us;
    for (int big_b = 0; big_b < 2; ++big_b)
      for (int j = 1; j <= 15; ++j) {
        Exp x = blank();
        for (int i = 0; i < 4; ++i) x.a[0][i] = 0x01010101u;  // bytes 0..15: k = 0..15
        for (int i = 0; i < 4; ++i) x.a[16][i] = 0x01010101u;  // lane group 1, bytes 0..15: k = 16..31
        for (int l = 0; l < 16; ++l)
          for (int i = 0; i < 4; ++i) x.b[l][i] = 0x11111111u;
        set_byte(x.a[0], 0, uint32_t(j) << 3);
        for (int l = 0; l < 16; ++l) set_nib(x.b[l], 0, big_b ? 6 : 2);
        v.push_back(x);
        us.push_back(j - 7 + 2 * big_b);
      }
    const auto d = execute(v);
    printf("{\"op\": \"accum_align\", \"case\": \"one_product_2^u_and_31_products_of_2^-10_in_one_block\", "
           "\"u_and_sum_minus_2^u_times_2^10\": [");
    for (size_t e = 0; e < v.size(); ++e)
      printf("%s[%d, %.10g]", e ? ", " : "", us[e], (double(at(&d[e * 256], 0, 0)) - std::ldexp(1.0, us[e])) * 1024.0);
    printf("]}\n");
  }
  return hipDeviceSynchronize() == hipSuccess ? 0 : 1;
}
