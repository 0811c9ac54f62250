// The second launch of a fixed-order sum (ordered_sum.h, step 5), for every metric whose planes have several chunks or tiles:
// partial [outer][parts][inner] -> out [outer][inner], the parts added in index order, each entry written through the POLICY the metric
// names (ordered_sum::nan_if_nan or nan_if_not_finite).  INNER is the inner width where it is a constant of the metric (the division
// is then a shift), 0 for `inner` at run time.
#pragma once
#include "launch.h"
#include "ordered_sum.h"

namespace {

template <double (*POLICY)(double), int INNER>
__global__ __launch_bounds__(ordered_sum::THREADS) void fold_parts_kernel(const double* __restrict__ partial, double* __restrict__ out, long long entries,
                                                                          int parts, int inner) {
    const long long e = (long long)blockIdx.x * ordered_sum::THREADS + threadIdx.x;
    if (e < entries) out[e] = POLICY(ordered_sum::fold_parts(partial, e, parts, INNER ? INNER : inner));
}

// on `st`, after the kernel that wrote `partial`; the caller launches it only when parts > 1.  Returns the HIP error (0: ok).
template <double (*POLICY)(double), int INNER = 0>
int c2w_fold_parts(const double* partial, double* out, long long outer, int parts, hipStream_t st, int inner = INNER) {
    const long long entries = outer * inner;
    fold_parts_kernel<POLICY, INNER><<<(unsigned)((entries + 255) / 256), ordered_sum::THREADS, 0, st>>>(partial, out, entries, parts, inner);
    return (int)hipGetLastError();
}

}  // namespace
