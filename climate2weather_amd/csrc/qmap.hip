// Quantile mapping per cell (c2w_hip.h: c2w_qmap_nodes, c2w_qmap_apply).  Node fit: qmap_gather_kernel turns a block of cells of the
// time-major planes into series-major scratch through an LDS tile, qmap_sort_kernel sorts one series per workgroup in LDS on the
// monotone key of quantile_core.h and interpolates the K levels in float64.  Apply: qmap_apply_kernel stages the {xq, yq} tables of a
// block of adjacent cells in LDS once and maps its group's rows, 16 bytes a load, each value bisected in LDS and mapped in float64.
// qmap_core.h has the maps and the arithmetic; this file is the workgroups around them.  No atomics, nothing read back by the host.
#include "launch.h"
#include "qmap_core.h"

namespace {

using namespace qmap;

// workgroup (x: position tile, y: cell tile, z: row)
__global__ __launch_bounds__(THREADS) void qmap_gather_kernel(const float* __restrict__ x, const int* __restrict__ tidx, float* __restrict__ scratch,
                                                              int T, int F, int hw, int Tu, int c0, int c1) {
    __shared__ float qmap_tile[TILE * TILE_LD];  // 16640 bytes
    const int tid = threadIdx.x;
    GView v;
    v.x = x, v.tidx = tidx, v.scratch = scratch, v.row = blockIdx.z, v.ctile = blockIdx.y, v.ptile = blockIdx.x;
    v.T = T, v.F = F, v.hw = hw, v.Tu = Tu, v.c0 = c0, v.c1 = c1, v.tile = qmap_tile;
    g_load(v, tid);
    __syncthreads();
    g_store(v, tid);
}

// workgroup b owns series b: (row, cell of the block, group)
__global__ __launch_bounds__(1024) void qmap_sort_kernel(const float* __restrict__ scratch, const int* __restrict__ goff,
                                                         const double* __restrict__ levels, double* __restrict__ q, long long* __restrict__ nvalid,
                                                         int F, int hw, int Tu, int c0, int c1, int G, int K, int skipna, int max_len) {
    extern __shared__ __align__(16) unsigned qmap_keys[];  // padded(max_len)
    const int tid = threadIdx.x;
    SView v;
    v.scratch = scratch, v.goff = goff, v.levels = levels, v.q = q, v.nvalid = nvalid, v.series = blockIdx.x;
    v.F = F, v.hw = hw, v.Tu = Tu, v.c0 = c0, v.c1 = c1, v.G = G, v.K = K, v.skipna = skipna, v.max_len = max_len;
    v.nthr = blockDim.x, v.keys = qmap_keys;
    s_load(v, tid);
    __syncthreads();
    const int N = padded(length_of(v));  // the same for the whole workgroup
    for (int k = 2; k <= N; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            s_stage(v, tid, k, j);
            __syncthreads();
        }
    s_nodes(v, tid);
}

// workgroup (x: slab, y: cell block, z: g F + f); x and out may be the same array
__global__ __launch_bounds__(APPLY_THREADS) void qmap_apply_kernel(const float* x, float* out, const double* __restrict__ xq, const double* __restrict__ yq,
                                                             const int* __restrict__ tidx, const int* __restrict__ goff, long long n_rep, int T, int F,
                                                             int hw, int Tu, int K) {
    extern __shared__ __align__(16) double qmap_tables[];  // apply_lds_bytes(K)
    const int tid = threadIdx.x;
    AView v;
    v.x = x, v.out = out, v.xq = xq, v.yq = yq, v.tidx = tidx, v.goff = goff, v.n_rep = n_rep;
    v.g = blockIdx.z / F, v.f = blockIdx.z % F, v.cblock = blockIdx.y, v.slab = blockIdx.x, v.slabs = gridDim.x;
    v.T = T, v.F = F, v.hw = hw, v.Tu = Tu, v.K = K, v.lds = qmap_tables;
    a_stage(v, tid);
    __syncthreads();
    a_walk(v, tid);
}

}  // namespace

extern "C" int c2w_qmap_supported(int hw, int K, int max_len) { return qmap::supported(hw, K, max_len) ? 1 : 0; }

extern "C" long long c2w_qmap_scratch_bytes(long long rows, int cells, int Tu) {
    if (rows < 1 || cells < 1 || Tu < 1) return 0;
    return qmap::scratch_bytes(rows, cells, Tu);
}

extern "C" int c2w_qmap_nodes(const float* x, const int* tidx, const int* goff, const double* levels, double* q, long long* n_valid, float* scratch,
                              unsigned long long scratch_bytes, long long n_rep, int T, int F, int hw, int Tu, int G, int K, int max_len, int skipna,
                              int c0, int c1, void* stream) {
    if (!qmap::supported(hw, K, max_len)) return C2W_ERR_UNSUPPORTED;
    if (!x || !tidx || !goff || !levels || !q || !n_valid || n_rep < 1 || T < 1 || F < 1 || G < 1 || Tu < 0 || Tu > T || max_len > Tu || c0 < 0 ||
        c1 > hw || c0 >= c1 || !c2w_aligned(4, x) || !c2w_aligned(8, q, n_valid, levels))
        return C2W_ERR_BAD_ARG;
    const long long rows = n_rep * F, need = Tu > 0 ? qmap::scratch_bytes(rows, c1 - c0, Tu) : 0;
    if (need > 0 && (!scratch || !c2w_aligned(4, scratch) || scratch_bytes < (unsigned long long)need)) return C2W_ERR_BAD_ARG;
    const long long series = rows * (c1 - c0) * G;
    if (rows > 65535 || tiles(c1 - c0) > 65535 || !c2w_grid_fits(series)) return C2W_ERR_BAD_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    if (Tu > 0) {
        const dim3 grid((unsigned)tiles(Tu), (unsigned)tiles(c1 - c0), (unsigned)rows);
        qmap_gather_kernel<<<grid, THREADS, 0, st>>>(x, tidx, scratch, T, F, hw, Tu, c0, c1);
        if (int rc = (int)hipGetLastError()) return rc;
    }
    const int N = padded(max_len);
    if (int rc = c2w_lds_optin<qmap_sort_kernel>(MAX_N * (int)sizeof(unsigned))) return rc;
    qmap_sort_kernel<<<(unsigned)series, sort_threads(N), N * sizeof(unsigned), st>>>(scratch, goff, levels, q, n_valid, F, hw, Tu, c0, c1, G, K,
                                                                                       skipna ? 1 : 0, max_len);
    return (int)hipGetLastError();
}

extern "C" int c2w_qmap_apply(const float* x, float* out, const double* xq, const double* yq, const int* tidx, const int* goff, long long n_rep, int T,
                              int F, int hw, int Tu, int G, int K, int max_len, void* stream) {
    if (!qmap::supported(hw, K, max_len)) return C2W_ERR_UNSUPPORTED;
    if (!x || !out || !xq || !yq || !tidx || !goff || n_rep < 1 || T < 1 || F < 1 || G < 1 || Tu < 0 || Tu > T || max_len > Tu ||
        !c2w_aligned(16, x, out) || !c2w_aligned(8, xq, yq))
        return C2W_ERR_BAD_ARG;
    if (Tu == 0) return 0;
    const long long blocks = (long long)G * F * cell_blocks(hw, K);
    if ((long long)G * F > 65535 || cell_blocks(hw, K) > 65535) return C2W_ERR_BAD_SHAPE;
    const int slabs = slab_count(blocks, n_rep * max_len, K, c2w_cu_count());
    if (int rc = c2w_lds_optin<qmap_apply_kernel>(APPLY_LDS)) return rc;
    const dim3 grid((unsigned)slabs, (unsigned)cell_blocks(hw, K), (unsigned)(G * F));
    qmap_apply_kernel<<<grid, APPLY_THREADS, apply_lds_bytes(K), (hipStream_t)stream>>>(x, out, xq, yq, tidx, goff, n_rep, T, F, hw, Tu, K);
    return (int)hipGetLastError();
}
