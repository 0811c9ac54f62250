// Extremes of an ensemble (c2w_hip.h: c2w_block_extremes_update, c2w_lmoments): the block maxima or minima of every series, streamed
// over calls of any length, and the sample L-moments of every series' block extremes.  The block extremes are integer maxima of keys:
// no bit depends on any order.  The L-moments are one thread's own arithmetic on its own registers: the bits are the same at every
// position of a launch.  extremes_maps.h has the index maps and the arithmetic; this file is the workgroups around them.
#include "launch.h"
#include "extremes_maps.h"

namespace {

using namespace extremes;

// workgroup b owns (row, variable, chunk) = (b / (F chunks), b / chunks % F, b % chunks)
__global__ __launch_bounds__(THREADS) void block_extremes_kernel(const float* __restrict__ x, const float* __restrict__ y, const int* __restrict__ dir,
                                                                 unsigned* __restrict__ open, float* __restrict__ table, long long* __restrict__ invalid,
                                                                 int n_chunks, int D, int T, int F, int hw, int B, int block, long long t0) {
    __shared__ int nan_hours[1];
    const int tid = threadIdx.x;
    BView v;
    v.x = x, v.y = y, v.dir = dir, v.open = open, v.table = table, v.invalid = invalid;
    v.chunk = (int)(blockIdx.x % n_chunks), v.f = (int)(blockIdx.x / n_chunks % F), v.d = (int)(blockIdx.x / n_chunks / F);
    v.D = D, v.T = T, v.F = F, v.hw = hw, v.B = B, v.block = block, v.t0 = t0;
    v.lds = nan_hours;
    b_zero(v, tid);
    __syncthreads();
    b_walk(v, tid);
    __syncthreads();
    b_flush(v, tid);
}

// workgroup b owns (row, chunk of 256 V cells) = (b / chunks, b % chunks)
template <int K, int V>
__global__ __launch_bounds__(THREADS) void lmoments_kernel(const float* __restrict__ table, double* __restrict__ lmom, int* __restrict__ n_valid,
                                                           int n_chunks, int n, int hw) {
    LView v;
    v.table = table, v.lmom = lmom, v.n_valid = n_valid;
    v.row = (long long)(blockIdx.x / n_chunks), v.chunk = (int)(blockIdx.x % n_chunks), v.n = n, v.hw = hw;
    l_cells<K, V>(v, threadIdx.x);
}

}  // namespace

extern "C" int c2w_block_extremes_supported(int hw, int block, int max_blocks) { return extremes::update_supported(hw, block, max_blocks) ? 1 : 0; }

extern "C" int c2w_block_extremes_update(const float* x, const float* y, const int* dir, unsigned* open, float* table, long long* invalid, int M, int T,
                                         int F, int hw, int block, int max_blocks, long long t0, void* stream) {
    if (!extremes::update_supported(hw, block, max_blocks) || M < 1) return C2W_ERR_UNSUPPORTED;
    if (!x || !dir || !open || !table || !invalid || T < 0 || F < 1 || t0 < 0) return C2W_ERR_BAD_ARG;
    if (!c2w_aligned(16, x, y, open, table) || !c2w_aligned(8, invalid) || !c2w_aligned(4, dir)) return C2W_ERR_BAD_ARG;
    if (T == 0) return 0;
    const int nc = extremes::chunks(hw), D = M + (y ? 1 : 0);
    const long long grid = (long long)D * F * nc;
    if (T > MAX_T || !c2w_grid_fits(grid) || extremes::end_closed(t0, T, block) > max_blocks) return C2W_ERR_BAD_SHAPE;
    block_extremes_kernel<<<(unsigned)grid, THREADS, 0, (hipStream_t)stream>>>(x, y, dir, open, table, invalid, nc, D, T, F, hw, max_blocks, block, t0);
    return (int)hipGetLastError();
}

extern "C" int c2w_lmoments_supported(int hw, int n) { return extremes::lmoments_supported(hw, n) ? 1 : 0; }

extern "C" int c2w_lmoments(const float* table, double* lmom, int* n_valid, long long R, int n, int hw, void* stream) {
    if (!extremes::lmoments_supported(hw, n)) return C2W_ERR_UNSUPPORTED;
    if (!table || !lmom || !n_valid || R < 0) return C2W_ERR_BAD_ARG;
    if (!c2w_aligned(16, table) || !c2w_aligned(8, lmom) || !c2w_aligned(4, n_valid)) return C2W_ERR_BAD_ARG;
    if (R == 0) return 0;
    int rc = 0;
    extremes::by_rows(n, [&](auto rows) {
        constexpr int K = rows.i, V = extremes::V_OF<K>;
        const int nc = extremes::lchunks(hw, V);
        if (R > 0x7fffffffLL || !c2w_grid_fits(R * nc)) {
            rc = C2W_ERR_BAD_SHAPE;
            return;
        }
        lmoments_kernel<K, V><<<(unsigned)(R * nc), THREADS, 0, (hipStream_t)stream>>>(table, lmom, n_valid, nc, n, hw);
        rc = (int)hipGetLastError();
    });
    return rc;
}
