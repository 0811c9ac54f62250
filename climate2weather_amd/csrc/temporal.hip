// Temporal increments of an ensemble (c2w_hip.h: c2w_tincr_terms): per row d, anchor t, variable f and lag tau the sums over the cells
// of |dx|, dx^2 and (dx - dy)^2, dx the row's increment from t to t + tau and dy the truth's.  tincr_terms_kernel is the hot path: a
// workgroup owns one (d, t, f) anchor plane or one chunk of it and walks the lags four at a time; the shared fold_parts_kernel
// (ordered_sum_launch.h) adds the chunks of a plane in index order when there are several.  temporal_core.h has the index maps and the
// arithmetic; this file is the workgroup around them.  No float atomics, no sum whose order depends on the launch.
#include "ordered_sum_launch.h"
#include "temporal_core.h"

namespace {

using namespace tincr;

// workgroup b owns plane b / n_chunks and chunk b % n_chunks
template <bool HAS_Y>
__global__ __launch_bounds__(THREADS) void tincr_terms_kernel(const float* __restrict__ x, const float* __restrict__ y, double* __restrict__ out,
                                                              int n_chunks, int T, int F, int hw, int L) {
    __shared__ double tincr_lds[LDS_DOUBLES];  // 26112 bytes
    const int tid = threadIdx.x;
    View v;
    v.x = x, v.y = HAS_Y ? y : nullptr, v.out = out, v.plane = (long long)blockIdx.x / n_chunks, v.chunk = (int)(blockIdx.x % n_chunks);
    v.T = T, v.F = F, v.hw = hw, v.L = L, v.lds = tincr_lds;
    const int n = rounds(hw, v.chunk), np = passes(L);
    for (int pass = 0; pass < np; ++pass) {
        if (!pass_has_pairs(v, pass)) {  // the same for every thread of the workgroup
            t_store(v, tid, pass, false);
            continue;
        }
        Thread th;
        t_init(th);
        for (int it = 0; it < n; ++it) t_round<HAS_Y>(v, th, tid, pass, it);
        t_stash(v, th, tid);
        __syncthreads();
        t_fold_groups(v, tid);
        __syncthreads();
        t_store(v, tid, pass, true);  // reads the group totals only: the next pass's stash does not touch them
    }
}

}  // namespace

extern "C" int c2w_tincr_supported(int hw, int L) { return tincr::supported(hw, L) ? 1 : 0; }

extern "C" long long c2w_tincr_scratch_bytes(long long rows, int T, int F, int hw, int L) {
    if (rows < 1 || T < 1 || F < 1 || !tincr::supported(hw, L)) return 0;
    return tincr::scratch_bytes(rows, T, F, hw, L);
}

extern "C" int c2w_tincr_terms(const float* x, const float* y, double* S, double* scratch, unsigned long long scratch_bytes, int n_rep, int T, int F,
                               int hw, int L, void* stream) {
    if (!tincr::supported(hw, L)) return C2W_ERR_UNSUPPORTED;
    if (!x || !S || n_rep < 1 || T < 1 || F < 1 || !c2w_aligned(16, x, y) || !c2w_aligned(8, S, scratch)) return C2W_ERR_BAD_ARG;
    const int nc = tincr::chunks(hw);
    const long long rows = (long long)n_rep + (y ? 1 : 0), planes = rows * T * F, grid = planes * nc, need = tincr::scratch_bytes(rows, T, F, hw, L);
    if (need > 0 && (!scratch || scratch_bytes < (unsigned long long)need)) return C2W_ERR_BAD_ARG;
    if (!c2w_grid_fits(grid)) return C2W_ERR_BAD_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    double* out = nc > 1 ? scratch : S;
    if (y)
        tincr_terms_kernel<true><<<(unsigned)grid, THREADS, 0, st>>>(x, y, out, nc, T, F, hw, L);
    else
        tincr_terms_kernel<false><<<(unsigned)grid, THREADS, 0, st>>>(x, y, out, nc, T, F, hw, L);
    const int rc = (int)hipGetLastError();
    if (rc || nc == 1) return rc;
    return c2w_fold_parts<ordered_sum::nan_if_not_finite>(scratch, S, planes, nc, st, 3 * L);
}
