// Stand-in for tensorflow/core/lib/core/status.h: the part of Status that the
// reference decoder's TopPaths and its caller use (OK(), ok(),
// error_message()).  No error codes: the decoder returns InvalidArgument only.
#pragma once
#include <string>

namespace tensorflow {

class Status {
 public:
  Status() {}
  explicit Status(const std::string& message) : ok_(false), message_(message) {}
  static Status OK() { return Status(); }
  bool ok() const { return ok_; }
  const std::string& error_message() const { return message_; }

 private:
  bool ok_ = true;
  std::string message_;
};

}  // namespace tensorflow
