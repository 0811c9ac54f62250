// Block moments at the observation grid (c2w_hip.h: c2w_block_moments): per S x S block of every (row, t, f) plane the finite count,
// the pivot and the pivoted float64 sums S1, S2 and, with a truth, X.  A thread owns a quad of 4 adjacent columns of a block row and
// adds its cells in row order; the first thread of each block adds the block's columns in order: the bits are the same at every
// position of a launch.  blockmoments_maps.h has the index maps and the arithmetic; this file is the workgroups around them.
#include "launch.h"
#include "blockmoments_maps.h"

namespace {

using namespace blockmoments;

// workgroup b owns (row, 256 consecutive items of the row's planes) = (b / n_chunks, b % n_chunks)
template <int S, bool TRUTH>
__global__ __launch_bounds__(THREADS) void block_moments_kernel(const float* __restrict__ x, const float* __restrict__ y, int* __restrict__ n,
                                                                float* __restrict__ pivot, double* __restrict__ sums, int n_chunks, int planes,
                                                                int items, int H, int W) {
    __shared__ double column_sums[entries(TRUTH) * 4 * THREADS];
    __shared__ int finite_cells[2 * THREADS];
    const int tid = threadIdx.x;
    View v;
    v.x = x, v.y = y, v.n = n, v.pivot = pivot, v.sums = sums;
    v.d = (int)(blockIdx.x / n_chunks), v.chunk = (int)(blockIdx.x % n_chunks);
    v.planes = planes, v.items = items, v.H = H, v.W = W;
    v.lds_sums = column_sums, v.lds_count = finite_cells;
    b_walk<S, TRUTH>(v, tid);
    __syncthreads();
    b_fold<S, TRUTH>(v, tid);
}

}  // namespace

extern "C" int c2w_block_moments_supported(int H, int W, int s) { return blockmoments::supported(H, W, s) ? 1 : 0; }

extern "C" int c2w_block_moments(const float* x, const float* y, int* n, float* pivot, double* sums, int M, int T, int F, int H, int W, int s,
                                 void* stream) {
    if (!blockmoments::supported(H, W, s) || M < 1 || T < 0 || F < 1) return C2W_ERR_UNSUPPORTED;
    const long long planes = (long long)T * F, items = blockmoments::row_items(planes, H, W, s);
    const int D = M + (y ? 1 : 0);
    const long long nc = blockmoments::chunks(items), grid = (long long)D * nc;
    if (items > 0x7fffffffLL - THREADS || !c2w_grid_fits(grid)) return C2W_ERR_UNSUPPORTED;  // the general route takes it
    if (!x || !n || !pivot || !sums) return C2W_ERR_BAD_ARG;
    if (!c2w_aligned(16, x, y) || !c2w_aligned(8, sums) || !c2w_aligned(4, n, pivot)) return C2W_ERR_BAD_ARG;
    if (T == 0) return 0;
    blockmoments::by_size(s, [&](auto size) {
        constexpr int S = size.i;
        if (y)
            block_moments_kernel<S, true><<<(unsigned)grid, THREADS, 0, (hipStream_t)stream>>>(x, y, n, pivot, sums, (int)nc, (int)planes, (int)items, H, W);
        else
            block_moments_kernel<S, false><<<(unsigned)grid, THREADS, 0, (hipStream_t)stream>>>(x, y, n, pivot, sums, (int)nc, (int)planes, (int)items, H, W);
    });
    return (int)hipGetLastError();
}
