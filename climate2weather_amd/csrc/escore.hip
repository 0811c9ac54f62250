// Energy and variogram scores of an ensemble (c2w_hip.h: c2w_escore_pairs, c2w_vario_terms): per (t, f) plane the squared distances
// of every pair of the M + 1 rows (the truth and the members), and per offset of a half-plane stencil the three sums of the variogram
// score, all in double.  escore_pairs_kernel: a workgroup owns 256 cells of one plane, reads every value of the M + 1 rows once from
// HBM into LDS and serves the pair loop from there, a thread a 4 x 4 tile of pairs.  vario_terms_kernel: a workgroup owns an 8 x 32
// tile of one plane with its halo in LDS, a thread a cell, the offsets four at a time with the member loop innermost.  The shared
// fold_parts_kernel (ordered_sum_launch.h) adds the chunks or the tiles of a plane in index order.  escore_core.h has the index maps
// and the arithmetic; this file is the workgroups around them.  No float atomics, no sum whose order depends on the launch.
#include "ordered_sum_launch.h"
#include "escore_core.h"

namespace {

using namespace escore;

extern __shared__ __attribute__((aligned(16))) unsigned char escore_lds[];

// workgroup b owns plane b / n_chunks and chunk b % n_chunks
__global__ __launch_bounds__(THREADS) void escore_pairs_kernel(const float* __restrict__ x, const float* __restrict__ y, double* __restrict__ out,
                                                               long long planes, int n_chunks, int M, int hw) {
    const int tid = threadIdx.x;
    PView v;
    v.x = x, v.y = y, v.out = out, v.plane = blockIdx.x / (unsigned)n_chunks, v.planes = planes, v.chunk = (int)(blockIdx.x % (unsigned)n_chunks);
    v.M = M, v.hw = hw, v.lds = escore_lds;
    PThread th;
    p_stage(v, tid);
    __syncthreads();
    p_pairs_of_tile(v, th, tid);
    __syncthreads();
    p_stash(v, th, tid);
    __syncthreads();
    p_fold_store(v, tid);
}

// workgroup b owns plane b / n_tiles and tile b % n_tiles
template <int ORDER2>
__global__ __launch_bounds__(THREADS) void vario_terms_kernel(const float* __restrict__ x, const float* __restrict__ y, double* __restrict__ out,
                                                              long long planes, int n_tiles, int M, int H, int W, int R) {
    const int tid = threadIdx.x;
    VView v;
    v.x = x, v.y = y, v.out = out, v.plane = blockIdx.x / (unsigned)n_tiles, v.planes = planes, v.tile = (int)(blockIdx.x % (unsigned)n_tiles);
    v.M = M, v.H = H, v.W = W, v.R = R, v.lds = escore_lds;
    v_stage(v, tid);
    const int O = v_offsets(R);
    for (int o0 = 0; o0 < O; o0 += V_BATCH) {
        __syncthreads();  // the patch is in place; the last batch's totals are read
        v_terms<ORDER2>(v, tid, o0);
        __syncthreads();
        v_fold_groups(v, tid);
        __syncthreads();
        v_fold_store(v, tid, o0);
    }
}

constexpr int P_LDS_MAX = (P_MAX_M + 1) * P_PITCH * 4;  // 67 600 bytes at M = 64: beyond 64 KiB, hence the opt-in
constexpr int V_LDS_MAX = ((V_MAX_M + 1) * (V_TH + V_MAX_R) * (V_TW + 2 * V_MAX_R) * 4 + 7) / 8 * 8 + V_FOLD_DOUBLES * 8;  // 78 336 bytes

template <int ORDER2>
int launch_vario(const float* x, const float* y, double* out, long long planes, long long grid, int nt, int M, int H, int W, int R, hipStream_t st) {
    const int lds = v_lds_bytes(R, M);
    if (lds > 65536)
        if (int rc = c2w_lds_optin<vario_terms_kernel<ORDER2>>(V_LDS_MAX)) return rc;
    vario_terms_kernel<ORDER2><<<(unsigned)grid, THREADS, lds, st>>>(x, y, out, planes, nt, M, H, W, R);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int c2w_escore_supported(int hw, int M) { return escore::p_supported(hw, M) ? 1 : 0; }

extern "C" long long c2w_escore_scratch_bytes(long long planes, int hw, int M) {
    if (planes < 1 || !escore::p_supported(hw, M)) return 0;
    return escore::p_scratch_bytes(planes, hw, M);
}

extern "C" int c2w_escore_pairs(const float* x, const float* y, double* d2, double* scratch, unsigned long long scratch_bytes, int M, long long planes,
                                int hw, void* stream) {
    if (!escore::p_supported(hw, M)) return C2W_ERR_UNSUPPORTED;
    if (!x || !y || !d2 || planes < 1 || !c2w_aligned(16, x, y) || !c2w_aligned(8, d2, scratch)) return C2W_ERR_BAD_ARG;
    const int nc = escore::p_chunks(hw), P = escore::p_pairs(M);
    const long long grid = planes * nc, need = escore::p_scratch_bytes(planes, hw, M);
    if (need > 0 && (!scratch || scratch_bytes < (unsigned long long)need)) return C2W_ERR_BAD_ARG;
    if (!c2w_grid_fits(grid)) return C2W_ERR_BAD_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const int lds = escore::p_lds_bytes(M);
    if (lds > 65536)
        if (int rc = c2w_lds_optin<escore_pairs_kernel>(P_LDS_MAX)) return rc;
    escore_pairs_kernel<<<(unsigned)grid, escore::THREADS, lds, st>>>(x, y, nc > 1 ? scratch : d2, planes, nc, M, hw);
    int rc = (int)hipGetLastError();
    if (rc || nc == 1) return rc;
    return c2w_fold_parts<ordered_sum::nan_if_not_finite>(scratch, d2, planes, nc, st, P);
}

extern "C" int c2w_vario_supported(int H, int W, int R, int M, int order2) { return escore::v_supported(H, W, R, M, order2) ? 1 : 0; }

extern "C" long long c2w_vario_scratch_bytes(long long planes, int H, int W, int R) {
    if (planes < 1 || H < 1 || W < 1 || R < 1 || R > escore::V_MAX_R) return 0;
    return escore::v_scratch_bytes(planes, H, W, R);
}

extern "C" int c2w_vario_terms(const float* x, const float* y, double* V, double* scratch, unsigned long long scratch_bytes, int M, long long planes, int H,
                               int W, int R, int order2, void* stream) {
    if (!escore::v_supported(H, W, R, M, order2)) return C2W_ERR_UNSUPPORTED;
    if (!x || !y || !V || planes < 1 || !c2w_aligned(4, x, y) || !c2w_aligned(8, V, scratch)) return C2W_ERR_BAD_ARG;
    const int nt = escore::v_tiles(H, W);
    const long long grid = planes * nt, need = escore::v_scratch_bytes(planes, H, W, R);
    if (need > 0 && (!scratch || scratch_bytes < (unsigned long long)need)) return C2W_ERR_BAD_ARG;
    if (!c2w_grid_fits(grid) || (long long)H * W > 0x7fffffffLL) return C2W_ERR_BAD_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    double* out = nt > 1 ? scratch : V;
    int rc;
    switch (order2) {
        case 1: rc = launch_vario<1>(x, y, out, planes, grid, nt, M, H, W, R, st); break;
        case 2: rc = launch_vario<2>(x, y, out, planes, grid, nt, M, H, W, R, st); break;
        default: rc = launch_vario<4>(x, y, out, planes, grid, nt, M, H, W, R, st); break;
    }
    if (rc || nt == 1) return rc;
    return c2w_fold_parts<ordered_sum::nan_if_not_finite>(scratch, V, planes, nt, st, escore::v_offsets(R) * 3);
}
