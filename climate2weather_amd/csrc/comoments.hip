// Co-moments of an ensemble (c2w_hip.h: c2w_comoments_update): per (row, cell) the pivoted sums S, C, ST, QT, X of the F variables
// over time, streamed over calls of any length.  One thread owns a cell's series and adds its terms in hour order into float64
// accumulators that travel from call to call: the bits are the same at every position of a launch and for every cut of the hours into
// calls.  comoments_maps.h has the index maps and the arithmetic; this file is the workgroups around them.
#include "launch.h"
#include "comoments_maps.h"

namespace {

using namespace comoments;

// workgroup b owns (row, chunk of 256 V(F) cells) = (b / chunks, b % chunks)
template <int F, bool TRUTH>
__global__ __launch_bounds__(THREADS) void comoments_update_kernel(const float* __restrict__ x, const float* __restrict__ y, int* __restrict__ n,
                                                                   float* __restrict__ pivot, float* __restrict__ truth_pivot,
                                                                   double* __restrict__ sums, long long* __restrict__ invalid, int n_chunks, int D,
                                                                   int T, int hw) {
    __shared__ int invalid_hours[1];
    const int tid = threadIdx.x;
    View v;
    v.x = x, v.y = y, v.n = n, v.pivot = pivot, v.truth_pivot = truth_pivot, v.sums = sums, v.invalid = invalid;
    v.d = (int)(blockIdx.x / n_chunks), v.chunk = (int)(blockIdx.x % n_chunks);
    v.D = D, v.T = T, v.hw = hw;
    v.lds = invalid_hours;
    u_zero(v, tid);
    __syncthreads();
    u_walk<F, TRUTH>(v, tid);
    __syncthreads();
    u_flush(v, tid);
}

}  // namespace

extern "C" int c2w_comoments_supported(int hw, int F) { return comoments::supported(hw, F) ? 1 : 0; }

extern "C" int c2w_comoments_update(const float* x, const float* y, int* n, float* pivot, float* truth_pivot, double* sums, long long* invalid, int M,
                                    int T, int F, int hw, void* stream) {
    if (!comoments::supported(hw, F) || M < 1) return C2W_ERR_UNSUPPORTED;
    if (!x || !n || !pivot || (y && !truth_pivot) || !sums || !invalid || T < 0) return C2W_ERR_BAD_ARG;
    if (!c2w_aligned(16, x, y, n, pivot, truth_pivot, sums) || !c2w_aligned(8, invalid)) return C2W_ERR_BAD_ARG;
    if (T == 0) return 0;
    const int nc = comoments::chunks(hw, F), D = M + (y ? 1 : 0);
    const long long grid = (long long)D * nc;
    if (T > MAX_T || !c2w_grid_fits(grid)) return C2W_ERR_BAD_SHAPE;
    comoments::by_variables(F, [&](auto vars) {
        constexpr int NF = vars.i;
        if (y)
            comoments_update_kernel<NF, true><<<(unsigned)grid, THREADS, 0, (hipStream_t)stream>>>(x, y, n, pivot, truth_pivot, sums, invalid, nc, D, T, hw);
        else
            comoments_update_kernel<NF, false><<<(unsigned)grid, THREADS, 0, (hipStream_t)stream>>>(x, y, n, pivot, truth_pivot, sums, invalid, nc, D, T, hw);
    });
    return (int)hipGetLastError();
}
