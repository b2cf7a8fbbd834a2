// Internal, host side: hipFuncAttributeMaxDynamicSharedMemorySize for kernels that ask for more dynamic LDS than the 64 KiB default.
#pragma once
#include "common.h"
#include <algorithm>
#include <utility>
#include <vector>

// The attribute holds ONE value per kernel function (the last set wins): keep the LARGEST size ever asked of a function and set it
// again only when a larger one appears -- B = 32 (160 KB), then B = 64 (32 KB), then B = 32 again must still find 160 KB
template <typename Kernel>
void ensure_dynamic_lds(Kernel kernel, size_t bytes) {
  static std::vector<std::pair<const void*, size_t>> attr_max;
  const void* kf = reinterpret_cast<const void*>(kernel);
  auto it = std::find_if(attr_max.begin(), attr_max.end(), [&](const std::pair<const void*, size_t>& e) { return e.first == kf; });
  if (it != attr_max.end() && it->second >= bytes) return;
  if (hipFuncSetAttribute(kf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) { (void)hipGetLastError(); }
  if (it == attr_max.end()) attr_max.push_back({kf, bytes}); else it->second = bytes;
}
