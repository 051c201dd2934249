// Stand-in for tensorflow/core/platform/types.h.  The reference decoder's
// headers include it and use none of its names; the fixed-width aliases are
// here for completeness.
#pragma once
#include <cstdint>

namespace tensorflow {

typedef std::int32_t int32;
typedef std::int64_t int64;

}  // namespace tensorflow
