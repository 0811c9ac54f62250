// Event objects of an ensemble (c2w_hip.h: c2w_object_tables): how many events are there, how big are they and where?  One workgroup
// labels the connected components of one (row, time, variable, threshold) plane entirely in LDS -- a bit mask of the indicator, 16-bit
// labels, a label-equivalence union-find whose minimum labels make the result independent of any order -- and writes the plane's row,
// its object list and its share of the area histogram.  Everything is integers.  objects_maps.h has the index maps and the arithmetic;
// this file is the workgroup around them.
#include "launch.h"
#include "objects_maps.h"

namespace {

using namespace objects;

// workgroup b owns plane b = ((d T + t) F + f) K + k: the thresholds run over the grid
__global__ __launch_bounds__(THREADS) void object_tables_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ thr,
                                                                const int* __restrict__ dir, long long* __restrict__ plane,
                                                                long long* __restrict__ area_hist, int* __restrict__ objs,
                                                                long long* __restrict__ invalid, int D, int T, int F, int H, int W, int K,
                                                                int connectivity, int max_objects) {
    extern __shared__ __attribute__((aligned(16))) unsigned char obj_lds[];  // LDS_BYTES
    const int tid = threadIdx.x;
    View v;
    v.x = x, v.y = y, v.thr = thr, v.dir = dir, v.plane = plane, v.area_hist = area_hist, v.objects = objs, v.invalid = invalid;
    v.b = (long long)blockIdx.x;
    v.D = D, v.T = T, v.F = F, v.H = H, v.W = W, v.K = K, v.connectivity = connectivity, v.max_objects = max_objects, v.lds = obj_lds;
    o_zero(v, tid);
    __syncthreads();
    o_stage(v, tid);
    __syncthreads();
    o_label(v, tid);
    __syncthreads();
    o_link(v, tid);
    __syncthreads();
    o_flatten(v, tid);
    __syncthreads();
    o_rank1(v, tid);
    __syncthreads();
    o_rank2(v, tid);
    __syncthreads();
    o_rank3(v, tid);
    __syncthreads();
    o_runs(v, tid);
    __syncthreads();
    o_roots(v, tid);
    __syncthreads();
    o_store(v, tid);
}

}  // namespace

extern "C" int c2w_objects_supported(int H, int W, int K, int connectivity, int max_objects) {
    return objects::supported(H, W, K, connectivity, max_objects) ? 1 : 0;
}

extern "C" int c2w_object_tables(const float* x, const float* y, const float* thr, const int* dir, long long* plane, long long* area_hist, int* objs,
                                 long long* invalid, int M, int T, int F, int H, int W, int K, int connectivity, int max_objects, void* stream) {
    if (!objects::supported(H, W, K, connectivity, max_objects) || M < 1) return C2W_ERR_UNSUPPORTED;
    if (!x || !thr || !dir || !plane || !area_hist || !invalid || (max_objects > 0 && !objs) || T < 0 || F < 1) return C2W_ERR_BAD_ARG;
    if (!c2w_aligned(16, x, y) || !c2w_aligned(8, plane, area_hist, invalid) || !c2w_aligned(4, thr, dir, objs)) return C2W_ERR_BAD_ARG;
    const int D = M + (y ? 1 : 0);
    const long long grid = (long long)D * T * F * K;
    if (!c2w_grid_fits(grid)) return C2W_ERR_BAD_SHAPE;
    if (T == 0) return 0;
    if (int rc = c2w_lds_optin<object_tables_kernel>(LDS_BYTES)) return rc;
    object_tables_kernel<<<(unsigned)grid, THREADS, LDS_BYTES, (hipStream_t)stream>>>(x, y, thr, dir, plane, area_hist, objs, invalid, D, T, F, H, W, K,
                                                                                     connectivity, max_objects);
    return (int)hipGetLastError();
}
