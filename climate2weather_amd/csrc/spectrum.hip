// Ensemble spectra: the radially averaged power spectral density of a batch of square fp32 fields (c2w_hip.h: c2w_rapsd), one launch,
// one read of each field, N/2 floats out and nothing in between in global memory.  A field lives in LDS from its load to its bin means:
// two real rows per complex row transform, column transforms over the N/2 kept columns, power, bin means (spectrum_core.h has the
// arithmetic and the index maps; this file is the workgroup around them).  A field of N <= 32 takes 2N threads, so a workgroup of 256
// takes 16, 8 or 4 fields; at N = 64 and 128 it takes one.  No atomics, no float sum whose order depends on the launch: a field's
// outputs are the same bits wherever it lies in the batch.
#include "launch.h"
#include "spectrum_core.h"

namespace {

using namespace spectrum;

template <int N>
__global__ __launch_bounds__(256) void rapsd_kernel(const float* __restrict__ x, float* __restrict__ spec, long long n_fields) {
    using P = Plan<N>;
    extern __shared__ __align__(16) float spec_lds[];  // FPW images | N twiddles | per field: doubles, ints (Plan<N>::lds_bytes)
    Cplx* const tw = (Cplx*)(spec_lds + P::FPW * P::IMG);
    double* const dbl = (double*)(tw + N);
    int* const ints = (int*)(dbl + P::FPW * P::AUX_D);
    const int slot = threadIdx.x / P::TPF, tl = threadIdx.x % P::TPF;
    const long long f = (long long)blockIdx.x * P::FPW + slot;
    const bool live = f < n_fields;  // the last workgroup of a batch may hold fewer fields: its idle threads only meet the barriers
    FieldView v;
    v.x = x + (live ? f : 0) * (long long)(N * N);
    v.spec = spec + (live ? f : 0) * (long long)P::R;
    v.img = spec_lds + slot * P::IMG;
    v.tw = tw;
    v.dpart = dbl + slot * P::AUX_D;
    v.dlev = v.dpart + P::TPF;
    v.cnt = ints + slot * P::TPF;
    if (threadIdx.x < N) tw[threadIdx.x] = twiddle128(threadIdx.x * (128 / N));
    if (live) phase_load<N>(v, tl);
    __syncthreads();
    if (live) phase_fold<N>(v, tl);
    __syncthreads();
    if (live) phase_rows_a<N>(v, tl);
    __syncthreads();
    if (live) phase_rows_b<N>(v, tl);
    __syncthreads();
    if (live) phase_untangle<N>(v, tl);
    __syncthreads();
    if (live) phase_cols_a<N>(v, tl);
    __syncthreads();
    if (live) phase_cols_b<N>(v, tl);
    __syncthreads();
    if (live) phase_bins<N>(v, tl);
    __syncthreads();
    if (live) phase_store<N>(v, tl);
}

// The N = 128 image is 66 KiB: above the static limit, so the kernel needs the dynamic-LDS opt-in.
template <int N>
int rapsd_launch(const float* x, float* spec, long long n_fields, hipStream_t st) {
    using P = Plan<N>;
    constexpr size_t lds = P::lds_bytes();
    if constexpr (lds > 48 * 1024) {
        if (int rc = c2w_lds_optin<rapsd_kernel<N>>((int)lds)) return rc;
    }
    const long long grid = (n_fields + P::FPW - 1) / P::FPW;
    if (!c2w_grid_fits(grid)) return C2W_ERR_BAD_SHAPE;
    rapsd_kernel<N><<<(unsigned)grid, 256, lds, st>>>(x, spec, n_fields);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int c2w_rapsd_supported(int H, int W) {
    return H == W && (H == 8 || H == 16 || H == 32 || H == 64 || H == 128) ? 1 : 0;
}

extern "C" int c2w_rapsd(const float* x, float* spec, long long n_fields, int H, int W, void* stream) {
    if (!c2w_rapsd_supported(H, W)) return C2W_ERR_UNSUPPORTED;
    if (!x || !spec || !c2w_aligned(16, x) || n_fields < 0) return C2W_ERR_BAD_ARG;
    if (n_fields == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    switch (H) {
        case 8: return rapsd_launch<8>(x, spec, n_fields, st);
        case 16: return rapsd_launch<16>(x, spec, n_fields, st);
        case 32: return rapsd_launch<32>(x, spec, n_fields, st);
        case 64: return rapsd_launch<64>(x, spec, n_fields, st);
        default: return rapsd_launch<128>(x, spec, n_fields, st);
    }
}
