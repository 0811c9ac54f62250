// Wind power of an ensemble (c2w_hip.h: c2w_wind_power): per cell the hub-height wind speed from the u and v planes and the turbine's
// power by a table lookup from LDS, per (d, t) plane their sums in double.  wind_power_kernel is the hot path: a workgroup owns one
// plane or one chunk of it, copies the packed curve into LDS once and reads every value of the two planes once, 16 bytes at a time;
// the shared fold_parts_kernel (ordered_sum_launch.h) adds the chunks of a plane in index order when there are several.  wind_core.h
// has the table, the lookup, the arithmetic and the index maps; this file is the workgroups around them.  No float atomics, no sum whose
// order depends on the launch.
#include "ordered_sum_launch.h"
#include "wind_core.h"

namespace {

using namespace wind;

// workgroup b owns plane b / n_chunks and chunk b % n_chunks
__global__ __launch_bounds__(THREADS) void wind_power_kernel(const float* __restrict__ fields, const uint4* __restrict__ table, double* __restrict__ out,
                                                             float* __restrict__ derived, int n_chunks, int F, int u_index, int v_index, int K,
                                                             float hub, int hw) {
    __shared__ uint4 wind_table[MAX_TABLE_BYTES / 16];  // 4624 bytes
    __shared__ double wind_lds[LDS_DOUBLES];            // 4352 bytes
    const int tid = threadIdx.x;
    View w;
    w.fields = fields, w.out = out, w.derived = derived, w.plane = blockIdx.x / (unsigned)n_chunks, w.chunk = (int)(blockIdx.x % (unsigned)n_chunks);
    w.F = F, w.u_index = u_index, w.v_index = v_index, w.hw = hw, w.hub = hub, w.table = view_table(wind_table, K), w.lds = wind_lds;
    Thread th;
    t_fetch(w, th, tid);  // the planes' loads are on their way while the table comes in
    for (int i = tid; i < table_bytes(K) / 16; i += THREADS) wind_table[i] = table[i];
    __syncthreads();
    t_cells(w, th, tid);
    t_stash(w, th, tid);
    __syncthreads();
    t_fold_groups(w, tid);
    __syncthreads();
    t_fold_store(w, tid);
}

}  // namespace

extern "C" int c2w_wind_supported(int hw, int K) { return wind::supported(hw, K) ? 1 : 0; }

extern "C" long long c2w_wind_table_bytes(int K) { return K >= 2 && K <= wind::MAX_K ? wind::table_bytes(K) : 0; }

extern "C" int c2w_wind_table(const double* xs, const double* ps, int K, void* table_host) {
    return wind::build_table(xs, ps, K, table_host) == 0 ? 0 : C2W_ERR_BAD_ARG;
}

extern "C" long long c2w_wind_scratch_bytes(long long planes, int hw) {
    if (planes < 1 || hw < 1) return 0;
    return wind::scratch_bytes(planes, hw);
}

extern "C" int c2w_wind_power(const float* fields, int F, int u_index, int v_index, const void* table, int K, float hub_factor, double* sums,
                              float* derived, double* scratch, unsigned long long scratch_bytes, long long planes, int hw, void* stream) {
    if (!wind::supported(hw, K)) return C2W_ERR_UNSUPPORTED;
    if (!fields || !table || !sums || planes < 1 || F < 1 || u_index < 0 || u_index >= F || v_index < 0 || v_index >= F ||
        !c2w_aligned(16, fields, table, derived) || !c2w_aligned(8, sums, scratch))
        return C2W_ERR_BAD_ARG;
    const int nc = wind::chunks(hw);
    const long long grid = planes * nc, need = wind::scratch_bytes(planes, hw);
    if (need > 0 && (!scratch || scratch_bytes < (unsigned long long)need)) return C2W_ERR_BAD_ARG;
    if (!c2w_grid_fits(grid)) return C2W_ERR_BAD_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    wind_power_kernel<<<(unsigned)grid, wind::THREADS, 0, st>>>(fields, (const uint4*)table, nc > 1 ? scratch : sums, derived, nc, F, u_index, v_index, K,
                                                                hub_factor, hw);
    int rc = (int)hipGetLastError();
    if (rc || nc == 1) return rc;
    return c2w_fold_parts<ordered_sum::nan_if_nan, 2>(scratch, sums, planes, nc, st);
}
