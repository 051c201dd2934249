// Stand-in for tensorflow/core/lib/core/errors.h: errors::InvalidArgument of
// one string, the only form the reference decoder calls.
#pragma once
#include "tensorflow/core/lib/core/status.h"

namespace tensorflow {
namespace errors {

inline Status InvalidArgument(const char* message) { return Status(message); }

}  // namespace errors
}  // namespace tensorflow
