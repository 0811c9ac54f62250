// Which side a *_core.h (and ordered_sum.h) is compiled for: the compiler says, no translation unit does ("Metric cores").
//   C2W_HD         a phase or helper that runs on the device in a .hip and on the host in a host driver
//   C2W_BOTH       what a launcher calls on the host as well (shape and support functions)
//   C2W_CORE_HOST  defined on the host side only: the one-thread-at-a-time stand-ins for atomics, wave shuffles and device intrinsics
// A .hip compiled as HIP gets the device qualifiers in both of its passes; anything compiled as plain C++ (tests/host_*_main.cpp)
// gets them empty, with the host <cmath> and a float4.  Every core includes this first, so each compiles as the first include of a
// unit on either side.
#pragma once

#ifdef __HIP__
#include <hip/hip_runtime.h>
#define C2W_HD __device__ __attribute__((always_inline))
#define C2W_BOTH __host__ __device__ __attribute__((always_inline))
#else
#include <cmath>
#define C2W_HD
#define C2W_BOTH
#define C2W_CORE_HOST 1
// The 16-byte load of the cores that take one.  Under a name of its own and reached through the macro, so that a host program which
// defines a float4 itself before it includes a core still compiles: from here on both mean this type.
struct alignas(16) c2w_host_float4 { float x, y, z, w; };
#define float4 c2w_host_float4
#endif
