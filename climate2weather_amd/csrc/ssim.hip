// Ensemble SSIM: the mean structural similarity of n_pairs fp32 field pairs under a uniform window (c2w_hip.h: c2w_ssim), one launch,
// one read of each x field, one double out per pair and nothing in between in global memory.  A workgroup of 256 owns one pair, or
// four when W <= 32; rows stream through a ring of LDS rows in strips of 8 output rows, the next strip's 16 bytes per thread in flight
// while this one is summed (ssim_core.h has the arithmetic and the index maps; this file is the workgroup around them).  No atomics, no
// sum whose order depends on the launch: a pair's score is the same bits wherever it lies in the batch.
#include "launch.h"
#include "ssim_core.h"

namespace {

using namespace ssim;

template <int WIN>
__global__ __launch_bounds__(256) void ssim_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ range,
                                                   double* __restrict__ out, long long n_pairs, long long n_truth, int H, int W) {
    using P = Plan<WIN>;
    __shared__ __align__(16) float lds_f[P::FLOATS];  // 45.1 / 40.6 / 36.1 KiB with the doubles: static, three workgroups a CU
    __shared__ double lds_d[DOUBLES];
    const Shape sh = make_shape(H, W, WIN);
    const int tid = threadIdx.x;
    View v;
    v.x = x, v.y = y, v.range = range, v.out = out;
    v.n_pairs = n_pairs, v.n_truth = n_truth, v.first = (long long)blockIdx.x * sh.FPW;
    v.ringA = lds_f, v.ringB = lds_f + P::RING_FLOATS, v.V = lds_f + 2 * P::RING_FLOATS;
    v.dpart = lds_d, v.dlev = lds_d + THREADS;
    Thread th;
    phase_pivot_partial(v, sh, tid);
    __syncthreads();
    phase_pivot_fold(v, sh, tid);
    __syncthreads();
    phase_prologue<WIN>(v, sh, th, tid);
    fetch<WIN>(v, sh, th, tid, 0);
    for (int s = 0; s < sh.NS; ++s) {
        phase_stash<WIN>(v, sh, th, tid, s);
        __syncthreads();
        if (s + 1 < sh.NS) fetch<WIN>(v, sh, th, tid, s + 1);
        phase_vertical<WIN>(v, sh, tid, s);
        __syncthreads();
        phase_horizontal<WIN>(v, sh, th, tid, s);
    }
    __syncthreads();  // the pivots' second-level partials have been read by everyone long ago; dpart is free since the prologue
    phase_partial(v, th, tid);
    __syncthreads();
    phase_fold(v, sh, tid);
    __syncthreads();
    phase_store(v, sh, tid);
}

template <int WIN>
int ssim_launch(const float* x, const float* y, const float* range, double* out, long long n_pairs, long long n_truth, int H, int W,
                hipStream_t st) {
    const int fpw = make_shape(H, W, WIN).FPW;
    const long long grid = (n_pairs + fpw - 1) / fpw;
    if (!c2w_grid_fits(grid)) return C2W_ERR_BAD_SHAPE;
    ssim_kernel<WIN><<<(unsigned)grid, THREADS, 0, st>>>(x, y, range, out, n_pairs, n_truth, H, W);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int c2w_ssim_supported(int H, int W, int win) {
    return ssim::supported(H, W, win) ? 1 : 0;
}

extern "C" int c2w_ssim(const float* x, const float* y, const float* data_range, double* out, long long n_pairs, long long n_truth, int H, int W,
                        int win, void* stream) {
    if (!c2w_ssim_supported(H, W, win)) return C2W_ERR_UNSUPPORTED;
    if (!x || !y || !data_range || !out || !c2w_aligned(16, x, y) || !c2w_aligned(8, out) || n_pairs < 0 || n_truth < 1)
        return C2W_ERR_BAD_ARG;
    if (n_pairs == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    switch (win) {
        case 7: return ssim_launch<7>(x, y, data_range, out, n_pairs, n_truth, H, W, st);
        case 11: return ssim_launch<11>(x, y, data_range, out, n_pairs, n_truth, H, W, st);
        default: return ssim_launch<15>(x, y, data_range, out, n_pairs, n_truth, H, W, st);
    }
}
