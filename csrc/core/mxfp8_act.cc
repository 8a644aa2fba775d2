#include "core/mxfp8_act.h"

#include <cstring>
#include <stdexcept>
#include <vector>

#include "core/fp8.h"

namespace dissem {
namespace mxfp8 {

void quantize_host(const uint16_t* bf16, int64_t n, uint8_t* codes, uint8_t* scales) {
  if (n < 0 || n % kBlock) throw std::runtime_error("mxfp8 quantization needs a multiple of 32 elements");
  std::vector<float> s(size_t(n / kBlock));
  fp8::pack_host(bf16, n, codes, s.data(), kBlock);
  for (int64_t b = 0; b < n / kBlock; ++b) {
    uint32_t u;
    std::memcpy(&u, &s[size_t(b)], 4);
    scales[b] = uint8_t(u >> 23);  // the scale is 2^E, E in [-126, 120]: its exponent field is E + 127
  }
}

}  // namespace mxfp8
}  // namespace dissem
