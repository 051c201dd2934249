// Stand-in for tensorflow/core/lib/gtl/flatmap.h.  BeamEntry::children is the
// decoder's only FlatMap and GetChild's emplace its only use: the pair of
// iterator and inserted-flag that std::unordered_map returns as well.  Nothing
// iterates the map, so its order cannot matter.
#pragma once
#include <unordered_map>

namespace tensorflow {
namespace gtl {

template <class Key, class Value>
using FlatMap = std::unordered_map<Key, Value>;

}  // namespace gtl
}  // namespace tensorflow
