// Stand-in for tensorflow/core/platform/macros.h: TF_DISALLOW_COPY_AND_ASSIGN,
// the one macro the reference decoder's headers use.
#pragma once

#define TF_DISALLOW_COPY_AND_ASSIGN(TypeName) \
  TypeName(const TypeName&) = delete;         \
  void operator=(const TypeName&) = delete
