// Ensemble CRPS and spread-skill (c2w_hip.h: c2w_crps_terms): per cell the four terms A, B, E, V of the M members against the truth,
// per (t, f) plane their sums in double.  crps_terms_kernel is the hot path: a workgroup owns one plane or one chunk of it, a thread
// sorts the members of its cells in registers by a compile-time network and reads every value once; the shared fold_parts_kernel
// (ordered_sum_launch.h) adds the chunks of a plane in index order when there are several.  crps_core.h has the index maps and the arithmetic; this file is the workgroups
// around them.  No float atomics, no sum whose order depends on the launch.
#include "ordered_sum_launch.h"
#include "crps_core.h"

namespace {

using namespace crps;

// workgroup b owns plane b / n_chunks and chunk b % n_chunks
template <int K, int V>
__global__ __launch_bounds__(THREADS) void crps_terms_kernel(const float* __restrict__ x, const float* __restrict__ y, double* __restrict__ out,
                                                             float* __restrict__ cells, int n_chunks, int M, int T, int F, int hw) {
    __shared__ double crps_lds[LDS_DOUBLES];  // 8704 bytes
    const int tid = threadIdx.x;
    View v;
    v.x = x, v.y = y, v.out = out, v.cells = cells, v.plane = (long long)blockIdx.x / n_chunks, v.chunk = (int)(blockIdx.x % n_chunks);
    v.M = M, v.T = T, v.F = F, v.hw = hw, v.lds = crps_lds;
    Thread<K, V> th;
    t_init(v, th);
    const int n = rounds(hw, v.chunk, V);
    for (int it = 0; it < n; ++it) {
        t_fetch(v, th, tid, it);
        t_cells(v, th);
    }
    t_stash(v, th, tid);
    __syncthreads();
    t_fold_groups(v, tid);
    __syncthreads();
    t_fold_store(v, tid);
}

template <int K, int V>
int launch_terms(const float* x, const float* y, double* out, float* cells, long long grid, int n_chunks, int M, int T, int F, int hw, hipStream_t st) {
    crps_terms_kernel<K, V><<<(unsigned)grid, THREADS, 0, st>>>(x, y, out, cells, n_chunks, M, T, F, hw);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int c2w_crps_supported(int hw, int M) { return crps::supported(hw, M) ? 1 : 0; }

extern "C" long long c2w_crps_scratch_bytes(int T, int F, int hw) {
    if (T < 1 || F < 1 || hw < 1) return 0;
    return crps::scratch_bytes(T, F, hw);
}

extern "C" int c2w_crps_terms(const float* x, const float* y, double* sums, float* cells, double* scratch, unsigned long long scratch_bytes, int M, int T,
                              int F, int hw, void* stream) {
    if (!crps::supported(hw, M)) return C2W_ERR_UNSUPPORTED;
    if (!x || !y || !sums || T < 1 || F < 1 || !c2w_aligned(16, x, y, cells) || !c2w_aligned(8, sums, scratch)) return C2W_ERR_BAD_ARG;
    const int nc = crps::chunks(hw);
    const long long planes = (long long)T * F, grid = planes * nc, need = crps::scratch_bytes(T, F, hw);
    if (need > 0 && (!scratch || scratch_bytes < (unsigned long long)need)) return C2W_ERR_BAD_ARG;
    if (!c2w_grid_fits(grid)) return C2W_ERR_BAD_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    double* out = nc > 1 ? scratch : sums;
    int rc;
    switch (crps::rows_of(M)) {
        case 8: rc = launch_terms<8, 4>(x, y, out, cells, grid, nc, M, T, F, hw, st); break;
        case 16: rc = launch_terms<16, 4>(x, y, out, cells, grid, nc, M, T, F, hw, st); break;
        case 32: rc = launch_terms<32, 2>(x, y, out, cells, grid, nc, M, T, F, hw, st); break;
        default: rc = launch_terms<64, 1>(x, y, out, cells, grid, nc, M, T, F, hw, st); break;
    }
    if (rc || nc == 1) return rc;
    return c2w_fold_parts<ordered_sum::nan_if_nan, 4>(scratch, sums, planes, nc, st);
}
