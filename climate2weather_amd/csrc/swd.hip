// Sliced Wasserstein distance of an ensemble (c2w_hip.h: c2w_swd_project, c2w_swd_distance): two launches, because a column can only be
// sorted once all T of its rows are projected.  swd_project_kernel is an fp32-input MFMA GEMM of every field against the P unit
// directions with the normalisation applied to the loaded value; swd_distance_kernel sorts one column pair per workgroup in LDS and
// writes one double.  swd_core.h has the index maps and the arithmetic; this file is the workgroups around them.  No atomics, no
// scratch, no sum whose order depends on the launch.
#include "launch.h"
#include "swd_core.h"

namespace {

using namespace swd;

// workgroups 0 .. tiles_x - 1 own the fields of x, the rest those of y (the truth, when both go in one launch: its few tiles would
// fill an eighth of the chip on their own and take as long as the samples')
__global__ __launch_bounds__(THREADS) void swd_project_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ theta,
                                                              const float* __restrict__ shift, const float* __restrict__ scale,
                                                              float* __restrict__ proj_x, float* __restrict__ proj_y, long long n_x, long long n_y,
                                                              long long tiles_x, int T, int F, int d, int P) {
    __shared__ __align__(16) float swd_lds[LDS_FLOATS];  // 54 KiB, static: two workgroups a CU
    const int tid = threadIdx.x;
    const bool second = (long long)blockIdx.x >= tiles_x;
    PView v;
    v.x = second ? y : x, v.theta = theta, v.shift = shift, v.scale = scale, v.proj = second ? proj_y : proj_x;
    v.n_fields = second ? n_y : n_x, v.first = ((long long)blockIdx.x - (second ? tiles_x : 0)) * BM, v.T = T, v.F = F, v.d = d, v.P = P;
    v.lds = swd_lds;
    PThread th;
    p_init(v, th, tid);
    const int steps = d / BK;
    p_fetch(v, th, 0);
    p_stash(v, th, tid, 0);
    __syncthreads();
    for (int kt = 0; kt < steps; ++kt) {
        if (kt + 1 < steps) p_fetch(v, th, kt + 1);
        p_compute(v, th, tid, kt & 1);
        if ((kt + 1) % FOLD == 0 || kt + 1 == steps) p_fold(th);
        if (kt + 1 < steps) p_stash(v, th, tid, (kt + 1) & 1);  // the buffer everyone left at the barrier that ended step kt - 1
        __syncthreads();
    }
    p_epi_stash(v, th, tid);
    __syncthreads();
    p_epi_write(v, tid);
}

__global__ __launch_bounds__(1024) void swd_distance_kernel(const float* __restrict__ px, const float* __restrict__ py, double* __restrict__ out,
                                                            int F, int P, int T, int N) {
    extern __shared__ __align__(16) float swd_keys[];  // 2 N floats
    __shared__ double dpart[SORT_DOUBLES];
    const int tid = threadIdx.x;
    DView v;
    v.px = px, v.py = py, v.out = out, v.block = blockIdx.x, v.F = F, v.P = P, v.T = T, v.N = N, v.nthr = blockDim.x;
    v.keys = swd_keys, v.dpart = dpart;
    const int nan = __syncthreads_or(d_load(v, tid));
    if (nan) {  // the whole workgroup: nothing is sorted, the answer is written as such
        d_store(v, tid, 1);
        return;
    }
    for (int k = 2; k <= N; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            d_stage(v, tid, k, j);
            __syncthreads();
        }
    d_partial(v, tid);
    __syncthreads();
    d_fold(v, tid);
    __syncthreads();
    d_store(v, tid, 0);
}

}  // namespace

extern "C" int c2w_swd_supported(int d, int P, int T) {
    return swd::project_supported(d, P) && swd::distance_supported(T) ? 1 : 0;
}

extern "C" int c2w_swd_project_pair(const float* x, const float* y, const float* theta, const float* shift, const float* scale, float* proj_x,
                                    float* proj_y, long long n_rep, int T, int F, int d, int P, void* stream) {
    if (!swd::project_supported(d, P)) return C2W_ERR_UNSUPPORTED;
    if (!x || !theta || !shift || !scale || !proj_x || (y && !proj_y) || !c2w_aligned(16, x, y, theta) || !c2w_aligned(4, proj_x, proj_y) ||
        n_rep < 0 || T < 1 || F < 1)
        return C2W_ERR_BAD_ARG;
    const long long n_x = n_rep * T * F, n_y = y ? (long long)T * F : 0;
    const long long tiles_x = (n_x + BM - 1) / BM, grid = tiles_x + (n_y + BM - 1) / BM;
    if (grid == 0) return 0;
    if (!c2w_grid_fits(grid)) return C2W_ERR_BAD_SHAPE;
    swd_project_kernel<<<(unsigned)grid, THREADS, 0, (hipStream_t)stream>>>(x, y, theta, shift, scale, proj_x, proj_y, n_x, n_y, tiles_x, T, F, d, P);
    return (int)hipGetLastError();
}

extern "C" int c2w_swd_project(const float* x, const float* theta, const float* shift, const float* scale, float* proj, long long n_rep, int T,
                               int F, int d, int P, void* stream) {
    return c2w_swd_project_pair(x, nullptr, theta, shift, scale, proj, nullptr, n_rep, T, F, d, P, stream);
}

extern "C" int c2w_swd_distance(const float* proj_x, const float* proj_y, double* out, long long n_rep, int F, int P, int T, void* stream) {
    if (!swd::distance_supported(T)) return C2W_ERR_UNSUPPORTED;
    if (!proj_x || !proj_y || !out || !c2w_aligned(8, out) || n_rep < 0 || F < 1 || P < 1) return C2W_ERR_BAD_ARG;
    const long long grid = n_rep * F * P;
    if (grid == 0) return 0;
    if (!c2w_grid_fits(grid)) return C2W_ERR_BAD_SHAPE;
    const int N = swd::padded(T), lds = 2 * N * (int)sizeof(float);
    if (int rc = c2w_lds_optin<swd_distance_kernel>(2 * MAX_T * (int)sizeof(float))) return rc;  // above the static limit at the largest T
    swd_distance_kernel<<<(unsigned)grid, swd::sort_threads(N), lds, (hipStream_t)stream>>>(proj_x, proj_y, out, F, P, T, N);
    return (int)hipGetLastError();
}
