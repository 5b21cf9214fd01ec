// The ofx_assoc handle: made and freed by assoc.hip (ofx_assoc_create / ofx_assoc_destroy), and the scratch that
// ofx_associate and ofx_photo_associate (photo.hip) both run their compaction in.
#pragma once
#include <stdint.h>

namespace ofx {

struct Assoc {
  int64_t cap = 0;
  uint8_t* flag = nullptr;   // [cap] 1 = accepted
  int32_t* rank = nullptr;   // [cap + 1] exclusive ranks of the accepted points, their number at [n]
  int32_t* tsum = nullptr;   // [scan_tiles(cap) + 1]
};

}  // namespace ofx
