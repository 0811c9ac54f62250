// Event verification of an ensemble (c2w_hip.h: c2w_event_counts, c2w_fss_sums): the joint table of truth indicator and member count
// per plane and threshold, and the neighbourhood sums of the fractions skill score at several radii.  Both products are integer
// tables: the workgroups add to the zeroed output with 64-bit integer adds, which commute, so the bits do not depend on any order.
// events_core.h has the index maps and the arithmetic; this file is the workgroups around them.
#include "launch.h"
#include "events_core.h"

namespace {

using namespace events;

// workgroup b owns plane b / n_chunks and chunk b % n_chunks
__global__ __launch_bounds__(THREADS) void event_counts_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ thr,
                                                               const int* __restrict__ dir, long long* __restrict__ counts,
                                                               long long* __restrict__ invalid, int n_chunks, int M, int T, int F, int hw, int K) {
    __shared__ int ev_bins[COUNT_LDS_INTS];  // 4168 bytes
    const int tid = threadIdx.x;
    CView v;
    v.x = x, v.y = y, v.thr = thr, v.dir = dir, v.counts = counts, v.invalid = invalid;
    v.plane = (long long)blockIdx.x / n_chunks, v.chunk = (int)(blockIdx.x % n_chunks);
    v.M = M, v.T = T, v.F = F, v.hw = hw, v.K = K, v.lds = ev_bins;
    c_zero(v, tid);
    __syncthreads();
    c_count(v, tid);
    __syncthreads();
    c_derive(v, tid);
    __syncthreads();
    c_flush(v, tid);
}

// workgroup b owns (plane, threshold, tile) = (b / (K tiles), b / tiles % K, b % tiles): the thresholds run over the grid
__global__ __launch_bounds__(THREADS) void fss_sums_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ thr,
                                                           const int* __restrict__ dir, long long* __restrict__ out, int n_tiles, int M, int T, int F,
                                                           int H, int W, int K, int S, int R, Radii radii) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fss_lds[];  // FSS_LDS_BYTES
    const int tid = threadIdx.x;
    FView v;
    v.x = x, v.y = y, v.thr = thr, v.dir = dir, v.out = out;
    v.tile = (int)(blockIdx.x % n_tiles), v.k = (int)(blockIdx.x / n_tiles % K), v.plane = (long long)blockIdx.x / n_tiles / K;
    v.M = M, v.T = T, v.F = F, v.H = H, v.W = W, v.K = K, v.S = S, v.R = R, v.radii = radii, v.lds = fss_lds;
    const Geo g = geo_of(H, W, R, v.tile);
    f_zero(v, tid);
    __syncthreads();
    for (int d = 0; d <= M; ++d) {
        unsigned short* sat = d == 0 ? sat0_of(v) : satm_of(v);
        f_load(v, g, tid, d);  // the member's table was last read before the barrier that precedes the flush of the row before
        __syncthreads();
        f_scan_rows(sat, g, tid);
        __syncthreads();
        f_scan_cols(sat, g, tid);
        __syncthreads();
        f_sums(v, g, tid, sat, d);
        __syncthreads();
        f_flush(v, tid, d);
    }
    EnsThread ens;
    f_ensemble_take(v, g, tid, ens);
    __syncthreads();  // the table is written over the bytes just taken
    f_ensemble_put(v, g, tid, ens);
    __syncthreads();
    f_scan_rows(sate_of(v), g, tid);
    __syncthreads();
    f_scan_cols(sate_of(v), g, tid);
    __syncthreads();
    f_sums(v, g, tid, sate_of(v), M + 1);
    __syncthreads();
    f_flush(v, tid, M + 1);
}

}  // namespace

extern "C" int c2w_event_counts_supported(int hw, int M, int K) { return events::counts_supported(hw, M, K) ? 1 : 0; }

extern "C" int c2w_event_counts(const float* x, const float* y, const float* thr, const int* dir, long long* counts, long long* invalid, int M, int T,
                                int F, int hw, int K, void* stream) {
    if (!events::counts_supported(hw, M, K)) return C2W_ERR_UNSUPPORTED;
    if (!x || !y || !thr || !dir || !counts || !invalid || T < 1 || F < 1 || !c2w_aligned(16, x, y) ||
        !c2w_aligned(8, counts, invalid) || !c2w_aligned(4, thr, dir))
        return C2W_ERR_BAD_ARG;
    const int nc = events::chunks(hw);
    const long long planes = (long long)T * F, grid = planes * nc;
    if (!c2w_grid_fits(grid)) return C2W_ERR_BAD_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    HIP_CHECK_RET(hipMemsetAsync(counts, 0, (size_t)planes * K * events::bins(M) * sizeof(long long), st));
    HIP_CHECK_RET(hipMemsetAsync(invalid, 0, (size_t)planes * sizeof(long long), st));
    event_counts_kernel<<<(unsigned)grid, THREADS, 0, st>>>(x, y, thr, dir, counts, invalid, nc, M, T, F, hw, K);
    return (int)hipGetLastError();
}

extern "C" int c2w_fss_supported(int H, int W, int M, int K, const int* radii, int S) {
    return radii && events::fss_supported(H, W, M, K, radii, S) ? 1 : 0;
}

extern "C" int c2w_fss_sums(const float* x, const float* y, const float* thr, const int* dir, long long* sums, const int* radii, int M, int T, int F,
                            int H, int W, int K, int S, void* stream) {
    if (!radii || !events::fss_supported(H, W, M, K, radii, S)) return C2W_ERR_UNSUPPORTED;
    if (!x || !y || !thr || !dir || !sums || T < 1 || F < 1 || !c2w_aligned(16, x, y) || !c2w_aligned(8, sums) || !c2w_aligned(4, thr, dir))
        return C2W_ERR_BAD_ARG;
    const int nt = events::tiles_y(H) * events::tiles_x(W);
    const long long planes = (long long)T * F, grid = planes * K * nt;
    if (!c2w_grid_fits(grid)) return C2W_ERR_BAD_SHAPE;
    Radii rr;
    for (int s = 0; s < MAX_S; ++s) rr.r[s] = s < S ? radii[s] : 0;
    if (int rc = c2w_lds_optin<fss_sums_kernel>(FSS_LDS_BYTES)) return rc;
    hipStream_t st = (hipStream_t)stream;
    HIP_CHECK_RET(hipMemsetAsync(sums, 0, (size_t)planes * K * S * (M + 2) * 2 * sizeof(long long), st));
    fss_sums_kernel<<<(unsigned)grid, THREADS, FSS_LDS_BYTES, st>>>(x, y, thr, dir, sums, nt, M, T, F, H, W, K, S, events::max_radius(radii, S), rr);
    return (int)hipGetLastError();
}
