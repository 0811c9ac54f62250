// Ensemble marginals (c2w_hip.h: c2w_kde_eval, c2w_pit_counts): the Gaussian kernel density estimate of every (member, variable) and
// (truth, variable) data set at N grid points, dense and exact (no pair is dropped, no truncation radius), and the rank histogram of
// the truth within the ensemble.  kde_partial_kernel is the hot path: a workgroup owns one data set and one chunk of its values and
// keeps its share of the grid as fp32 accumulators in registers; kde_fold_kernel adds a data set's chunks in index order in double;
// pit_count_kernel reads every field once and bins in LDS.  kde_core.h has the index maps and the arithmetic; this file is the
// workgroups around them.  No float atomics, no sum whose order depends on the launch.
#include "launch.h"
#include "kde_core.h"

namespace {

using namespace kde;

// workgroup b owns data set b / chunks and chunk b % chunks; samples and truth ride in the same launch
template <int P>
__global__ __launch_bounds__(THREADS) void kde_partial_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ off,
                                                              const float* __restrict__ pivot, const double* __restrict__ h,
                                                              double* __restrict__ partial, long long n_x, long long n_chunks, int T, int F, int hw,
                                                              int N) {
    __shared__ float4 kde_tile[THREADS];  // 4 KiB
    const int tid = threadIdx.x;
    KView v;
    v.x = x, v.y = y, v.off = off, v.pivot = pivot, v.h = h, v.partial = partial, v.n_x = n_x;
    v.ds = (long long)blockIdx.x / n_chunks, v.chunk = (long long)blockIdx.x % n_chunks, v.T = T, v.F = F, v.hw = hw, v.N = N;
    v.lds = kde_tile;
    KThread<P> th;
    k_init(v, th, tid);
    const long long tiles = k_tiles(th);
    k_fetch(v, th, tid, 0);
    for (long long tile = 0; tile < tiles; ++tile) {
        k_stash(v, th, tid);
        __syncthreads();
        if (tile + 1 < tiles) k_fetch(v, th, tid, tile + 1);  // in flight while this tile is walked
        k_compute(v, th, k_count(th, tile));
        __syncthreads();
    }
    k_store(v, th, tid, __syncthreads_or(th.bad));
}

__global__ __launch_bounds__(THREADS) void kde_fold_kernel(const double* __restrict__ partial, const double* __restrict__ h, double* __restrict__ dens,
                                                           long long n, int N, int blocks_per_set) {
    const long long ds = blockIdx.x / blocks_per_set;
    const int j = (blockIdx.x % blocks_per_set) * THREADS + threadIdx.x;
    if (j < N) f_fold(partial, h, dens, ds, j, n, N);
}

__global__ __launch_bounds__(THREADS) void pit_count_kernel(const float* __restrict__ x, const float* __restrict__ y, long long* __restrict__ counts, int M,
                                                            int T, int F, int hw) {
    __shared__ int pit_hist[PIT_HIST];  // 4160 bytes
    const int tid = threadIdx.x;
    PView v;
    v.x = x, v.y = y, v.counts = counts, v.block = blockIdx.x, v.grid = gridDim.x, v.M = M, v.T = T, v.F = F, v.hw = hw, v.hist = pit_hist;
    pit_zero(v, tid);
    __syncthreads();
    pit_count(v, tid);
    __syncthreads();
    pit_flush(v, tid);
}

template <int P>
int launch_partial(const float* x, const float* y, const float* off, const float* pivot, const double* h, double* partial, long long n_x,
                   long long n_chunks, long long grid, int T, int F, int hw, int N, hipStream_t st) {
    kde_partial_kernel<P><<<(unsigned)grid, THREADS, 0, st>>>(x, y, off, pivot, h, partial, n_x, n_chunks, T, F, hw, N);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int c2w_kde_supported(int hw, int N) { return kde::supported(hw, N) ? 1 : 0; }

extern "C" long long c2w_kde_scratch_bytes(long long D, long long n, int N) {
    if (D < 0 || n < 1 || N < 1) return 0;
    return D * kde::chunks(n) * N * (long long)sizeof(double);
}

extern "C" int c2w_kde_partial(const float* x, const float* y, const float* offsets, const float* pivot, const double* h, double* scratch,
                               unsigned long long scratch_bytes, long long n_rep, int T, int F, int hw, int N, void* stream) {
    if (!kde::supported(hw, N)) return C2W_ERR_UNSUPPORTED;
    if (n_rep < 0 || T < 1 || F < 1 || (n_rep > 0 && !x) || !offsets || !pivot || !h || !scratch || !c2w_aligned(16, x, y) ||
        !c2w_aligned(8, h, scratch) || !c2w_aligned(4, offsets, pivot))
        return C2W_ERR_BAD_ARG;
    const long long n_x = n_rep * F, D = n_x + (y ? F : 0), n = (long long)T * hw, nc = kde::chunks(n), grid = D * nc;
    if (D == 0) return 0;
    if (!c2w_grid_fits(grid)) return C2W_ERR_BAD_SHAPE;
    if (scratch_bytes < (unsigned long long)c2w_kde_scratch_bytes(D, n, N)) return C2W_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    switch (kde::points_per_thread(N)) {
        case 1: return launch_partial<1>(x, y, offsets, pivot, h, scratch, n_x, nc, grid, T, F, hw, N, st);
        case 2: return launch_partial<2>(x, y, offsets, pivot, h, scratch, n_x, nc, grid, T, F, hw, N, st);
        case 3: return launch_partial<3>(x, y, offsets, pivot, h, scratch, n_x, nc, grid, T, F, hw, N, st);
        default: return launch_partial<4>(x, y, offsets, pivot, h, scratch, n_x, nc, grid, T, F, hw, N, st);
    }
}

extern "C" int c2w_kde_fold(const double* scratch, const double* h, double* dens, long long D, long long n, int N, void* stream) {
    if (N < 1 || N > kde::MAX_N) return C2W_ERR_UNSUPPORTED;
    if (D < 0 || n < 1 || !scratch || !h || !dens || !c2w_aligned(8, h, scratch, dens)) return C2W_ERR_BAD_ARG;
    const int per_set = (N + THREADS - 1) / THREADS;
    if (D == 0) return 0;
    if (!c2w_grid_fits(D * per_set)) return C2W_ERR_BAD_SHAPE;
    kde_fold_kernel<<<(unsigned)(D * per_set), THREADS, 0, (hipStream_t)stream>>>(scratch, h, dens, n, N, per_set);
    return (int)hipGetLastError();
}

extern "C" int c2w_kde_eval(const float* x, const float* y, const float* offsets, const float* pivot, const double* h, double* scratch,
                            unsigned long long scratch_bytes, double* dens, long long n_rep, int T, int F, int hw, int N, void* stream) {
    if (!kde::supported(hw, N)) return C2W_ERR_UNSUPPORTED;
    if (!dens || !c2w_aligned(8, dens)) return C2W_ERR_BAD_ARG;
    if (int rc = c2w_kde_partial(x, y, offsets, pivot, h, scratch, scratch_bytes, n_rep, T, F, hw, N, stream)) return rc;
    return c2w_kde_fold(scratch, h, dens, n_rep * F + (y ? F : 0), (long long)T * hw, N, stream);
}

extern "C" int c2w_pit_supported(int hw, int M) { return kde::pit_supported(hw, M) ? 1 : 0; }

extern "C" int c2w_pit_counts(const float* x, const float* y, long long* counts, int M, int T, int F, int hw, void* stream) {
    if (!kde::pit_supported(hw, M)) return C2W_ERR_UNSUPPORTED;
    if (!x || !y || !counts || T < 1 || F < 1 || !c2w_aligned(16, x, y) || !c2w_aligned(8, counts)) return C2W_ERR_BAD_ARG;
    // eight workgroups a CU at most, a whole number of times per variable; the counts are integers, so the grid changes no result
    long long per_var = (long long)c2w_cu_count() * 8 / F;
    per_var = per_var < 1 ? 1 : per_var > T ? T : per_var;
    const long long grid = per_var * F;
    if (!c2w_grid_fits(grid) || ((long long)T + per_var - 1) / per_var * hw > 0x7fffffffLL) return C2W_ERR_BAD_SHAPE;  // an LDS bin is an int
    hipStream_t st = (hipStream_t)stream;
    HIP_CHECK_RET(hipMemsetAsync(counts, 0, (size_t)F * (M + 1) * sizeof(long long), st));
    pit_count_kernel<<<(unsigned)grid, THREADS, 0, st>>>(x, y, counts, M, T, F, hw);
    return (int)hipGetLastError();
}
