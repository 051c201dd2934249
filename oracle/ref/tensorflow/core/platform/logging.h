// Stand-in for tensorflow/core/platform/logging.h: CHECK_NOTNULL (returns its
// argument) and CHECK_EQ, the two checks the reference decoder makes.  A
// failed check aborts, as TensorFlow's does.
#pragma once
#include <cstdio>
#include <cstdlib>

namespace tensorflow {
namespace ref_standin {

template <class P>
inline P CheckNotNull(const char* what, P p) {
  if (p == nullptr) {
    std::fprintf(stderr, "Check failed: '%s' must be non NULL\n", what);
    std::abort();
  }
  return p;
}

}  // namespace ref_standin
}  // namespace tensorflow

#define CHECK_NOTNULL(p) ::tensorflow::ref_standin::CheckNotNull(#p, (p))
#define CHECK_EQ(a, b)                                              \
  do {                                                              \
    if (!((a) == (b))) {                                            \
      std::fprintf(stderr, "Check failed: %s == %s\n", #a, #b);     \
      std::abort();                                                 \
    }                                                               \
  } while (0)
