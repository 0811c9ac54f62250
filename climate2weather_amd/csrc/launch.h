// The launch layer: the host-side chores every launcher of libc2w_hip.so shares ("Launch layer").  Host code only.
//   c2w_lds_optin<kernel>(bytes)   the dynamic-LDS opt-in a kernel needs before a launch with more than 64 KB, once per device
//   c2w_by_dtype / c2w_by_dtype16  the C2W_DTYPE_* tag of the C ABI -> the storage type a launcher template is instantiated with
//   c2w_cu_count()                 the compute units of the current device, where dispatch arithmetic means "one workgroup per CU"
//   c2w_aligned(bytes, pointers..) the argument check of the metric launchers: every pointer a multiple of `bytes`
//   c2w_grid_fits(workgroups)      and: the one-dimensional grid is within what a launch takes
// A new kernel uses these; nothing else in csrc/ calls hipFuncSetAttribute, compares a dtype tag to pick a template, or spells the CU
// count as a number.
#pragma once
#include <atomic>
#include <cstdint>
#include "common.h"
#include "c2w_hip.h"

constexpr int C2W_MAX_DEVICES = 64;  // devices with a table slot; a device index beyond it is served uncached

// `bytes` a power of two.  A null pointer counts as aligned: whether an argument may be null is the entry point's own check.
template <typename... P>
bool c2w_aligned(uintptr_t bytes, const P*... p) {
    return ((uintptr_t(0) | ... | (uintptr_t)p) & (bytes - 1)) == 0;
}

constexpr bool c2w_grid_fits(long long workgroups) { return workgroups <= 0x7fffffffLL; }

// Raises hipFuncAttributeMaxDynamicSharedMemorySize of `Kernel` to at least `bytes` on the current device; returns the HIP error (0: ok).
// The runtime keeps the attribute per device, so the table of what was granted is per device too (per kernel: a static of this template).
// Threads: the slot is written only after the attribute is set, so a thread that reads >= bytes launches with the opt-in in place; two
// threads that race on a first launch both set the attribute before either launches, which is harmless: every site asks for ONE size
// per kernel (the largest any of its launches takes), so the racing calls set the same value.
template <auto Kernel>
int c2w_lds_optin(int bytes) {
    static std::atomic<int> granted[C2W_MAX_DEVICES];
    int dev = -1;
    HIP_CHECK_RET(hipGetDevice(&dev));
    const bool slot = dev >= 0 && dev < C2W_MAX_DEVICES;
    if (slot && granted[dev].load(std::memory_order_acquire) >= bytes) return 0;
    HIP_CHECK_RET(hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    if (slot) granted[dev].store(bytes, std::memory_order_release);
    return 0;
}

// f(T{}) for the storage type T of `dtype`; any other tag is C2W_ERR_BAD_ARG.  The 16 form is for launchers that exist in the two 16-bit
// types only (it instantiates no fp32 kernel).
template <typename F>
int c2w_by_dtype16(int dtype, F&& f) {
    if (dtype == C2W_DTYPE_BF16) return f(bf16_t{});
    if (dtype == C2W_DTYPE_F16) return f(f16_t{});
    return C2W_ERR_BAD_ARG;
}
template <typename F>
int c2w_by_dtype(int dtype, F&& f) {
    return dtype == C2W_DTYPE_F32 ? f(float{}) : c2w_by_dtype16(dtype, f);
}

// Compute units of the current device (256 on the MI355X), cached per device.  256 when the runtime cannot say (no device): the query
// entry points that plan with it, such as c2w_conv_splitk_plan, stay total.
inline int c2w_cu_count() {
    static std::atomic<int> cus[C2W_MAX_DEVICES];
    int dev = -1, n = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    const bool slot = dev >= 0 && dev < C2W_MAX_DEVICES;
    if (slot && (n = cus[dev].load(std::memory_order_relaxed)) > 0) return n;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) return 256;
    if (slot) cus[dev].store(n, std::memory_order_relaxed);
    return n;
}
