// Exact quantiles (c2w_hip.h: c2w_quantiles): the order statistics of every (member, variable) and (truth, variable) data set by radix
// select on the monotone key of the fp32 bit pattern.  quantile_count_kernel is the hot path: a workgroup owns one data set and a slab
// of its planes, reads them once with 16-byte loads and counts one key digit in LDS; quantile_locate_kernel turns the counts into the
// bins of the target ranks and the slots of the next pass, and after the last pass into the values.  Three reads of the data, nothing
// read back by the host in between.  quantile_core.h has the maps and the arithmetic; this file is the workgroups around them.
// Integer counts only: no float atomics, no result that depends on the launch.
#include "launch.h"
#include "quantile_core.h"

namespace {

using namespace qnt;

// workgroup b owns data set b / slabs and slab b % slabs; samples and truth ride in the same launch
template <bool FIRST>
__global__ __launch_bounds__(THREADS) void quantile_count_kernel(const float* __restrict__ x, const float* __restrict__ y, unsigned char* scratch,
                                                                 Layout lay, long long n_x, int slabs, int T, int F, int hw, int pass, int R) {
    extern __shared__ __align__(16) unsigned char qnt_lds[];
    const int tid = threadIdx.x;
    CView v;
    v.x = x, v.y = y, v.n_x = n_x, v.ds = blockIdx.x / slabs, v.slab = blockIdx.x % slabs, v.slabs = slabs, v.T = T, v.F = F, v.hw = hw;
    v.pass = pass, v.R = R;
    v.nan = (long long*)(scratch + lay.nan) + v.ds;
    v.pre = (const unsigned*)(scratch + lay.pre) + v.ds * R;
    v.tab = scratch + lay.tab + v.ds * BINS0;
    v.hist = (int*)qnt_lds;
    if (FIRST) {
        v.table = (long long*)(scratch + lay.table0) + v.ds * BINS0;
        v.ns = 0;
        v.lpre = nullptr, v.ltab = nullptr, v.lnan = v.hist + BINS0;
    } else {
        v.table = (long long*)(scratch + (pass == 1 ? lay.table1 : lay.table2)) + v.ds * R * BINS;
        const int ns = ((const int*)(scratch + lay.ns))[v.ds];
        v.ns = ns < 0 ? 0 : ns > R ? R : ns;
        v.lpre = (unsigned*)(v.hist + R * BINS), v.ltab = (unsigned char*)(v.lpre + R), v.lnan = (int*)(v.ltab + BINS0);
        if (v.ns == 0) return;  // a NaN row: the whole workgroup leaves
    }
    c_zero(v, tid);
    __syncthreads();
    c_count<FIRST>(v, tid);
    __syncthreads();
    c_flush(v, tid);
}

__global__ __launch_bounds__(LOCATE_THREADS) void quantile_locate_kernel(unsigned char* scratch, Layout lay, Levels lv, double* __restrict__ out,
                                                                         float* __restrict__ stats, long long* __restrict__ n_valid, long long n, int Q,
                                                                         int pass, int skipna) {
    __shared__ long long qnt_part[MAX_RANKS * LOCATE_THREADS];  // 32 KiB
    __shared__ unsigned qnt_newpre[MAX_RANKS];
    __shared__ int qnt_isfirst[MAX_RANKS];
    __shared__ double qnt_q[MAX_Q];
    const int tid = threadIdx.x, R = 2 * Q;
    LView v;
    v.ds = blockIdx.x, v.n = n, v.Q = Q, v.R = R, v.pass = pass, v.skipna = skipna, v.q = qnt_q;
    v.table = pass == 0 ? (const long long*)(scratch + lay.table0) + v.ds * BINS0
                        : (const long long*)(scratch + (pass == 1 ? lay.table1 : lay.table2)) + v.ds * R * BINS;
    v.nan = (const long long*)(scratch + lay.nan) + v.ds;
    v.res = (long long*)(scratch + lay.res) + v.ds * R;
    v.pre = (unsigned*)(scratch + lay.pre) + v.ds * R;
    v.rslot = (int*)(scratch + lay.rslot) + v.ds * R;
    v.ns = (int*)(scratch + lay.ns) + v.ds;
    v.tab = scratch + lay.tab + v.ds * BINS0;
    v.out = out, v.stats = stats, v.nvalid = n_valid;
    v.part = qnt_part, v.newpre = qnt_newpre, v.isfirst = qnt_isfirst;
#pragma unroll
    for (int j = 0; j < MAX_Q; ++j)  // static indices into the by-value argument: it stays out of private memory
        if (j == tid) qnt_q[j] = lv.q[j];
    l_open(v);
    __syncthreads();  // every thread has read what the previous pass left before any phase writes
    l_sums(v, tid);
    __syncthreads();
    l_find(v, tid);
    __syncthreads();
    if (pass == 2) {
        l_final(v, tid);
        return;
    }
    l_mark(v, tid);
    __syncthreads();
    l_slots(v, tid);
}

template <bool FIRST>
int launch_count(const float* x, const float* y, unsigned char* scratch, const Layout& lay, long long n_x, long long D, int slabs, int T, int F, int hw,
                 int pass, int Q, hipStream_t st) {
    // one size per kernel: the largest any launch takes (32 slots)
    if (int rc = c2w_lds_optin<quantile_count_kernel<FIRST>>(count_lds_bytes(FIRST ? 0 : 1, MAX_Q))) return rc;
    quantile_count_kernel<FIRST><<<(unsigned)(D * slabs), THREADS, count_lds_bytes(pass, Q), st>>>(x, y, scratch, lay, n_x, slabs, T, F, hw, pass, 2 * Q);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int c2w_quantile_supported(int hw, int Q) { return qnt::supported(hw, Q) ? 1 : 0; }

extern "C" long long c2w_quantile_scratch_bytes(long long D, int Q) {
    if (D < 0 || Q < 1 || Q > qnt::MAX_Q) return 0;
    return qnt::layout(D, Q).total;
}

extern "C" int c2w_quantiles(const float* x, const float* y, const double* q, int Q, int skipna, void* scratch, unsigned long long scratch_bytes,
                             double* out, float* stats, long long* n_valid, long long n_rep, int T, int F, int hw, void* stream) {
    if (!qnt::supported(hw, Q)) return C2W_ERR_UNSUPPORTED;
    if (n_rep < 0 || T < 1 || F < 1 || (n_rep > 0 && !x) || !q || !scratch || !out || !stats || !n_valid ||
        !c2w_aligned(16, x, y, scratch) || !c2w_aligned(8, out, n_valid) || !c2w_aligned(4, stats))
        return C2W_ERR_BAD_ARG;
    Levels lv{};
    for (int j = 0; j < Q; ++j) {
        if (!(q[j] >= 0.0 && q[j] <= 1.0)) return C2W_ERR_BAD_ARG;  // a NaN level fails both comparisons
        lv.q[j] = q[j];
    }
    const long long n_x = n_rep * F, D = n_x + (y ? F : 0), n = (long long)T * hw;
    if (D == 0) return 0;
    const int slabs = slab_count(D, T, c2w_cu_count());
    // an LDS counter is an int: a workgroup's slab stays below 2^31 values (and its quads below 2^29)
    if (!c2w_grid_fits(D * slabs) || (long long)slab_planes(T, slabs) * hw > 0x7fffffffLL) return C2W_ERR_BAD_SHAPE;
    const Layout lay = layout(D, Q);
    if (scratch_bytes < (unsigned long long)lay.total) return C2W_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    unsigned char* s = (unsigned char*)scratch;
    HIP_CHECK_RET(hipMemsetAsync(s, 0, (size_t)lay.zeroed, st));
    for (int pass = 0; pass < 3; ++pass) {
        if (int rc = pass == 0 ? launch_count<true>(x, y, s, lay, n_x, D, slabs, T, F, hw, pass, Q, st)
                               : launch_count<false>(x, y, s, lay, n_x, D, slabs, T, F, hw, pass, Q, st))
            return rc;
        quantile_locate_kernel<<<(unsigned)D, LOCATE_THREADS, 0, st>>>(s, lay, lv, out, stats, n_valid, n, Q, pass, skipna);
        if (int rc = (int)hipGetLastError()) return rc;
    }
    return 0;
}
