// Held-out validation: the loss tail (eps_pred - eps)^2 of src/thor/pipelines.py:35 resolved by noise-level bin x output channel, without
// the (B,C,H,W) tensor and without an atomic.  Two launches on one stream:
//   1. sq_err_image_channel_kernel   part[b][slab][c] = sum over the slab's pixels of (y - eps)^2        (plain fp32 stores)
//   2. loss_level_table_kernel       table[bin(t_b)][c] += (double) sum over slabs of part[b][slab][c]   (one workgroup, images in order)
// Every sum has one order, fixed by (B, C, HW): equal operands give equal bits.  HBM-bound streaming kernels: 16-byte loads of the rows.
#include <algorithm>
#include "launch.h"
#include "philox.h"

namespace {

constexpr int EV_PT = 64;               // pixels per LDS tile: the slab unit (pointwise.hip's LT_PT)
constexpr int EV_LD = EV_PT + 1;
constexpr int EV_Q = EV_PT / 4;         // 16 lanes share a channel plane's 64 pixels, four consecutive pixels each (one Philox counter)
constexpr int EV_TARGET_BLOCKS = 2048;  // 8 workgroups per CU of the 256: B = 128 images of 16384 pixels -> 16 slabs of 16 tiles each
constexpr size_t EV_LDS_MAX = 64 * 1024;

// Slabs of an image: whole 64-pixel tiles, `tps` of them per slab (the last slab may hold fewer, the last tile fewer pixels).  A pure
// function of (B, HW) -- the scratch size and the summation order follow from it.
struct SlabPlan { int ntile, tps, nslab; };
SlabPlan slab_plan(int B, int HW) {
    SlabPlan p;
    p.ntile = (HW + EV_PT - 1) / EV_PT;
    const int want = std::max(1, std::min(p.ntile, (EV_TARGET_BLOCKS + B - 1) / B));
    p.tps = (p.ntile + want - 1) / want;
    p.nslab = (p.ntile + p.tps - 1) / p.tps;
    return p;
}

__device__ __forceinline__ float sub16_sum(float v) {  // xor tree over the 16 lanes that share a channel
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Stage 1 through the LDS tile of sq_err_tiled_kernel (pointwise.hip): rows of 64 pixels x ldc channels are read as one contiguous run of
// 16-byte vectors and transposed; thread (q, cb) then owns pixels 4q .. 4q+3 of channels cb, cb + 16, ...  eps is read from memory as one
// 16-byte vector (SQ == 1) or regenerated (SQ == 2: the four pixels are one Philox counter of the dense NCHW index, bit-identical to
// c2w_philox_normal).  A thread's running sums live in LDS slots of its own, acc[c][q]; at the end the 16 lanes of a channel meet in a
// shuffle tree and lane 0 stores the slab's sum.  Channels >= C are never read out of the tile.  HW % 4 == 0, eps 16-byte aligned.
template <typename T, int SQ>
__global__ __launch_bounds__(256) void sq_err_image_channel_kernel(const T* __restrict__ y, const float* __restrict__ eps, float* __restrict__ part,
                                                                   int C, int HW, int ldc, int nslab, int tps, uint32_t k0, uint32_t k1) {
    constexpr int P = Elem<T>::PER16;
    extern __shared__ float ev_tile[];             // [ldc][EV_LD]
    float* const acc = ev_tile + (size_t)ldc * EV_LD;  // [C][EV_Q]
    const int b = blockIdx.x / nslab, slab = blockIdx.x - b * nslab;
    const int ntile = (HW + EV_PT - 1) / EV_PT, nvec = ldc / P;
    const int t0 = slab * tps, t1 = min(t0 + tps, ntile);
    const int q = threadIdx.x & (EV_Q - 1), cb = threadIdx.x / EV_Q;
    for (int c = cb; c < C; c += 256 / EV_Q) acc[c * EV_Q + q] = 0.f;  // own slots only: no barrier needed for them
    for (int tile = t0; tile < t1; ++tile) {
        const int p0 = tile * EV_PT;
        const int npx = min(EV_PT, HW - p0);
        for (int i = threadIdx.x; i < npx * nvec; i += 256) {
            const int px = i / nvec, v = i - px * nvec;
            float f[P];
            unpack16<T>(*(const u32x4_t*)(y + ((size_t)b * HW + p0) * ldc + (size_t)i * P), f);
#pragma unroll
            for (int e = 0; e < P; ++e) ev_tile[(v * P + e) * EV_LD + px] = f[e];
        }
        __syncthreads();
        if (4 * q < npx) {
#pragma unroll 2
            for (int c = cb; c < C; c += 256 / EV_Q) {
                const size_t o = ((size_t)b * C + c) * HW + p0 + 4 * q;
                const f32x4_t e = SQ == 2 ? philox_normal4(k0, k1, (unsigned long long)o >> 2) : *(const f32x4_t*)(eps + o);
                const float* t = ev_tile + c * EV_LD + 4 * q;
                // eps as VALUES before the subtraction (sq_err_tiled_kernel): otherwise hipcc contracts the Box-Muller product with the
                // difference and the regenerated form is one rounding away from the materialised stream
                float e0 = e[0], e1 = e[1], e2 = e[2], e3 = e[3];
                asm volatile("" : "+v"(e0), "+v"(e1), "+v"(e2), "+v"(e3));
                const float d0 = t[0] - e0, d1 = t[1] - e1, d2 = t[2] - e2, d3 = t[3] - e3;
                acc[c * EV_Q + q] += (__fmul_rn(d0, d0) + __fmul_rn(d1, d1)) + (__fmul_rn(d2, d2) + __fmul_rn(d3, d3));
            }
        }
        __syncthreads();
    }
    for (int c = cb; c < C; c += 256 / EV_Q) {  // cb is uniform over the 16 lanes of a channel: they take this loop together
        const float s = sub16_sum(acc[c * EV_Q + q]);
        if (q == 0) part[((size_t)b * nslab + slab) * C + c] = s;
    }
}

// Stage 1 for every other shape (eps as a tensor only): one thread per channel walks the slab's pixels in order.  The rows are read
// coalesced over the channels, eps at a stride of HW -- the path of odd image sizes and of rows too wide for the tile, not the hot one.
template <typename T>
__global__ __launch_bounds__(256) void sq_err_image_channel_any_kernel(const T* __restrict__ y, const float* __restrict__ eps,
                                                                       float* __restrict__ part, int C, int HW, int ldc, int nslab, int tps) {
    const int b = blockIdx.x / nslab, slab = blockIdx.x - b * nslab;
    const int p_lo = min(HW, slab * tps * EV_PT), p_hi = min(HW, (slab + 1) * tps * EV_PT);
    for (int c = threadIdx.x; c < C; c += 256) {
        const T* yr = y + ((size_t)b * HW + p_lo) * ldc + c;
        const float* er = eps + ((size_t)b * C + c) * HW + p_lo;
        float s = 0.f;
        for (int p = 0; p < p_hi - p_lo; ++p) {
            const float d = Elem<T>::ld(yr + (size_t)p * ldc) - er[p];
            s += __fmul_rn(d, d);
        }
        part[((size_t)b * nslab + slab) * C + c] = s;
    }
}

// Stage 2: one workgroup, thread c owns column c of the table (c, c + 256, ... beyond 256 channels), images in ascending order, slabs in
// ascending order.  Bin rule (part of the interface, c2w_hip.h): ONE fp32 multiply of t clamped to [0, 1].
__global__ __launch_bounds__(256) void loss_level_table_kernel(const float* __restrict__ part, const float* __restrict__ t, double* __restrict__ table,
                                                               long long* __restrict__ count, float* __restrict__ per_image, int B, int C, int nslab,
                                                               int K) {
    __shared__ float wsum[2][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int b = 0; b < B; ++b) {
        const float tb = fminf(fmaxf(t[b], 0.f), 1.f);
        const int bin = min(K - 1, (int)floorf(__fmul_rn(tb, (float)K)));
        float mine = 0.f;
        for (int c = threadIdx.x; c < C; c += 256) {
            const float* p = part + (size_t)b * nslab * C + c;
            float s = 0.f;
            for (int sl = 0; sl < nslab; ++sl) s += p[(size_t)sl * C];
            table[(size_t)bin * C + c] += (double)s;
            mine += s;
        }
        if (threadIdx.x == 0) count[bin] += 1;
        if (per_image != nullptr) {  // uniform over the workgroup: wave trees, then the four waves in order
            mine = wave_sum(mine);
            if (lane == 0) wsum[b & 1][wave] = mine;
            __syncthreads();  // the other half of wsum is rewritten only behind the NEXT barrier, after thread 0 has read this one
            if (threadIdx.x == 0) per_image[b] = ((wsum[b & 1][0] + wsum[b & 1][1]) + wsum[b & 1][2]) + wsum[b & 1][3];
        }
    }
}

int levels_launch(const void* y, const float* eps, unsigned long long seed, bool regen, const float* t, double* table, long long* count,
                  float* per_image, int B, int C, int HW, int ldc, int K, float* scratch, unsigned long long scratch_bytes, int dtype, void* stream) {
    const int P = dtype == C2W_DTYPE_F32 ? 4 : 8;
    if (dtype != C2W_DTYPE_F32 && dtype != C2W_DTYPE_BF16 && dtype != C2W_DTYPE_F16) return C2W_ERR_BAD_ARG;
    if (!y || (!regen && !eps) || !t || !table || !count || !c2w_aligned(16, y)) return C2W_ERR_BAD_ARG;
    if (B <= 0 || C <= 0 || HW <= 0 || K <= 0 || ldc < C || ldc % P != 0) return C2W_ERR_BAD_SHAPE;
    const SlabPlan pl = slab_plan(B, HW);
    const size_t lds = ((size_t)ldc * EV_LD + (size_t)C * EV_Q) * sizeof(float);
    const bool tiled = lds <= EV_LDS_MAX && (HW & 3) == 0 && (regen || c2w_aligned(16, eps));
    if (regen && !tiled) return C2W_ERR_UNSUPPORTED;  // the caller materialises the stream (c2w_philox_normal) and passes it as a tensor
    if (scratch == nullptr || scratch_bytes < (unsigned long long)c2w_sq_err_levels_scratch_bytes(B, C, HW)) return C2W_ERR_BAD_ARG;
    if (!c2w_grid_fits((long long)B * pl.nslab)) return C2W_ERR_BAD_SHAPE;
    const unsigned grid = (unsigned)B * pl.nslab;
    hipStream_t st = (hipStream_t)stream;
#define EV_STAGE1(T)                                                                                                                            \
    do {                                                                                                                                        \
        if (!tiled) sq_err_image_channel_any_kernel<T><<<grid, 256, 0, st>>>((const T*)y, eps, scratch, C, HW, ldc, pl.nslab, pl.tps);          \
        else if (regen) sq_err_image_channel_kernel<T, 2><<<grid, 256, lds, st>>>((const T*)y, nullptr, scratch, C, HW, ldc, pl.nslab, pl.tps, \
                                                                                   (uint32_t)seed, (uint32_t)(seed >> 32));                    \
        else sq_err_image_channel_kernel<T, 1><<<grid, 256, lds, st>>>((const T*)y, eps, scratch, C, HW, ldc, pl.nslab, pl.tps, 0u, 0u);        \
    } while (0)
    if (dtype == C2W_DTYPE_F32) EV_STAGE1(float);
    else if (dtype == C2W_DTYPE_BF16) EV_STAGE1(bf16_t);
    else EV_STAGE1(f16_t);
#undef EV_STAGE1
    HIP_CHECK_RET(hipGetLastError());
    loss_level_table_kernel<<<1, 256, 0, st>>>(scratch, t, table, count, per_image, B, C, pl.nslab, K);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" long long c2w_sq_err_levels_scratch_bytes(int B, int C, int HW) {
    if (B <= 0 || C <= 0 || HW <= 0) return C2W_ERR_BAD_SHAPE;
    return (long long)B * slab_plan(B, HW).nslab * C * (long long)sizeof(float);
}

extern "C" int c2w_sq_err_levels(const void* y, const float* eps, const float* t, double* table, long long* count, float* per_image, int B, int C,
                                 int HW, int ldc, int K, float* scratch, unsigned long long scratch_bytes, int dtype, void* stream) {
    return levels_launch(y, eps, 0ull, false, t, table, count, per_image, B, C, HW, ldc, K, scratch, scratch_bytes, dtype, stream);
}

extern "C" int c2w_sq_err_levels_noise(const void* y, unsigned long long seed, const float* t, double* table, long long* count, float* per_image,
                                       int B, int C, int HW, int ldc, int K, float* scratch, unsigned long long scratch_bytes, int dtype,
                                       void* stream) {
    return levels_launch(y, nullptr, seed, true, t, table, count, per_image, B, C, HW, ldc, K, scratch, scratch_bytes, dtype, stream);
}
