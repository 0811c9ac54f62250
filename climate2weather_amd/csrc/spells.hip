// Event spells of an ensemble (c2w_hip.h: c2w_spell_update): how long an event lasts.  One block of times updates the per-series state
// (open run, longest, count, hours) and adds the spells that ended in it to the duration histogram and their first hours to the onset
// table.  Everything is integers: the workgroups add to the caller's accumulators with 64-bit integer adds, which commute, so the bits
// do not depend on any order.  spells_core.h has the index maps and the arithmetic; this file is the workgroup around them.
#include "launch.h"
#include "spells_core.h"

namespace {

using namespace spells;

// workgroup b owns (row, variable, chunk) = (b / (F chunks), b / chunks % F, b % chunks)
__global__ __launch_bounds__(THREADS) void spell_update_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ thr,
                                                               const int* __restrict__ dir, int* __restrict__ state, long long* __restrict__ hist,
                                                               long long* __restrict__ onsets, long long* __restrict__ invalid, int n_chunks, int D,
                                                               int T, int F, int hw, int K, int lmax, int period, int phase0, int k0, int kn) {
    __shared__ int spell_bins[LDS_INTS];  // 4484 bytes
    const int tid = threadIdx.x;
    View v;
    v.x = x, v.y = y, v.thr = thr, v.dir = dir, v.state = state, v.hist = hist, v.onsets = onsets, v.invalid = invalid;
    v.chunk = (int)(blockIdx.x % n_chunks), v.f = (int)(blockIdx.x / n_chunks % F), v.d = (int)(blockIdx.x / n_chunks / F);
    v.k0 = k0, v.kn = kn, v.D = D, v.T = T, v.F = F, v.hw = hw, v.K = K, v.lmax = lmax, v.period = period, v.phase0 = phase0;
    v.lds = spell_bins;
    s_zero(v, tid);
    __syncthreads();
    s_walk(v, tid);
    __syncthreads();
    s_flush(v, tid);
}

}  // namespace

extern "C" int c2w_spell_supported(int hw, int K, int max_duration, int period) { return spells::supported(hw, K, max_duration, period) ? 1 : 0; }

extern "C" int c2w_spell_update(const float* x, const float* y, const float* thr, const int* dir, int* state, long long* hist, long long* onsets,
                                long long* invalid, int M, int T, int F, int hw, int K, int max_duration, int period, long long t0, void* stream) {
    if (!spells::supported(hw, K, max_duration, period) || M < 1) return C2W_ERR_UNSUPPORTED;
    if (!x || !thr || !dir || !state || !hist || !invalid || (period > 0 && !onsets) || T < 0 || F < 1 || t0 < 0) return C2W_ERR_BAD_ARG;
    if (!c2w_aligned(16, x, y, state) || !c2w_aligned(8, hist, onsets, invalid) || !c2w_aligned(4, thr, dir)) return C2W_ERR_BAD_ARG;
    if (T == 0) return 0;
    const int nc = spells::chunks(hw), D = M + (y ? 1 : 0);
    const long long grid = (long long)D * F * nc;
    if (T > MAX_T || !c2w_grid_fits(grid)) return C2W_ERR_BAD_SHAPE;
    const int phase0 = period > 0 ? (int)(t0 % period) : 0;
    hipStream_t st = (hipStream_t)stream;
    for (int g = 0; g < spells::groups(K); ++g) {  // the groups touch disjoint entries of the state and of the tables
        spell_update_kernel<<<(unsigned)grid, THREADS, 0, st>>>(x, y, thr, dir, state, hist, onsets, invalid, nc, D, T, F, hw, K, max_duration, period,
                                                                phase0, g * GROUP, spells::group_size(K, g));
        if (int rc = (int)hipGetLastError()) return rc;
    }
    return 0;
}
