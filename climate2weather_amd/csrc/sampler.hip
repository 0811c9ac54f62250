// Device-resident pieces of the diffusion sampler (src/thor/pipelines.py:41-97) and of the sliding-window score
// function (src/thor/score.py:68-93,111-185).  The reference keeps the trajectory on the host and ships every
// window batch over PCIe each step; here the whole state x[L][F][H][W] (fp32) lives in HBM and these streaming
// kernels gather windows straight into the network's NHWC input, scatter the kept frames back, apply the
// predictor / corrector updates and the Gaussian-likelihood guidance term.
#include "common.h"
#include "c2w_hip.h"

int c2w_planes_to_rows_strided(const float* x, void* y, int B, int C, int HW, int ldc, long long img_stride, int dtype, hipStream_t st);

namespace {

inline int grid_for(long long n, int per_block = 256, int cap = 8192) {
    long long g = (n + per_block - 1) / per_block;
    if (g < 1) g = 1;
    return (int)(g < cap ? g : cap);
}

// unfold (src/thor/score.py:68-74) fused with NCHW->NHWC + cast: window j = frames i0+j .. i0+j+w-1, channel = tau*F + c.
// In memory a window's (w*F, H, W) tensor is just the contiguous run of frames starting at frame i0+j.
template <typename T>
__global__ __launch_bounds__(256) void window_gather_kernel(const float* __restrict__ x, T* __restrict__ y, int nw, int CW, int HW,
                                                            long long frame_stride, int i0, int ldc) {
    constexpr int P = Elem<T>::PER16;
    const int nvec = ldc / P;
    const long long total = (long long)nw * HW * nvec;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int pix = (int)(i % HW);
        const long long r = i / HW;
        const int vec = (int)(r % nvec);
        const int j = (int)(r / nvec);
        const float* src = x + (long long)(i0 + j) * frame_stride;
        float f[P];
#pragma unroll
        for (int e = 0; e < P; ++e) {
            const int c = vec * P + e;
            f[e] = (c < CW) ? src[(long long)c * HW + pix] : 0.f;
        }
        *(u32x4_t*)(y + ((size_t)j * HW + pix) * ldc + vec * P) = pack16<T>(f);
    }
}

// window_gather_kernel for an arbitrary list of windows: window j starts at frame first[j] of the flattened (members * L) frame array
// (exact guidance evaluates only the windows whose kept frames are observed, and co-sampled members share a batch).
template <typename T>
__global__ __launch_bounds__(256) void window_gather_list_kernel(const float* __restrict__ x, T* __restrict__ y, const int* __restrict__ first,
                                                                 int n, int CW, int HW, long long frame_stride, int ldc) {
    constexpr int P = Elem<T>::PER16;
    const int nvec = ldc / P;
    const long long total = (long long)n * HW * nvec;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int pix = (int)(i % HW);
        const long long r = i / HW;
        const int vec = (int)(r % nvec);
        const int j = (int)(r / nvec);
        const float* src = x + (long long)first[j] * frame_stride;
        float f[P];
#pragma unroll
        for (int e = 0; e < P; ++e) {
            const int c = vec * P + e;
            f[e] = (c < CW) ? src[(long long)c * HW + pix] : 0.f;
        }
        *(u32x4_t*)(y + ((size_t)j * HW + pix) * ldc + vec * P) = pack16<T>(f);
    }
}

// The adjoint of fold for a list of windows: the output gradient of window j is delta on the slots fold keeps of it (the centre frame;
// the leading k of a trajectory's first window, kind bit 0; the trailing k of its last, kind bit 1) where that frame is observed, and
// zero everywhere else -- the padding channels of the row included.  delta: [members][nobs][F][HW] fp32, observation o = frame / t_step.
template <typename T>
__global__ __launch_bounds__(256) void window_cotangent_list_kernel(const float* __restrict__ delta, T* __restrict__ dy,
                                                                    const int* __restrict__ first, const int* __restrict__ kind, int n, int L,
                                                                    int F, int HW, int k, int t_step, int nobs, int ldc) {
    constexpr int P = Elem<T>::PER16;
    const int nvec = ldc / P;
    const int CW = (2 * k + 1) * F;
    const long long total = (long long)n * HW * nvec;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int pix = (int)(i % HW);
        const long long r = i / HW;
        const int vec = (int)(r % nvec);
        const int j = (int)(r / nvec);
        const int member = first[j] / L, i0 = first[j] % L, kd = kind[j];
        float f[P];
#pragma unroll
        for (int e = 0; e < P; ++e) {
            const int c = vec * P + e;
            const int tau = c / F, frame = i0 + tau;
            const bool kept = c < CW && (tau == k || (tau < k && (kd & 1)) || (tau > k && (kd & 2)));
            const bool observed = frame % t_step == 0 && frame / t_step < nobs;
            f[e] = (kept && observed) ? delta[(((long long)member * nobs + frame / t_step) * F + (c - tau * F)) * HW + pix] : 0.f;
        }
        *(u32x4_t*)(dy + ((size_t)j * HW + pix) * ldc + vec * P) = pack16<T>(f);
    }
}

// The adjoint of the gather for a list of windows, in gather form: one thread owns V consecutive pixels of one plane (frame l, variable f)
// of the trajectory and adds scale * (the sum, in ascending j, over the windows that contain frame l, of their input gradient at slot
// l - first[j]) -- no atomics, a fixed order: the same bits launch after launch.  A block works on ONE frame, so the scan of the list
// is uniform over the block.  dx: [n][w F][HW] fp32; frames l0 .. l0 + nl - 1 of the flattened (members * L) frame array are visited.
template <int V>
__global__ __launch_bounds__(256) void window_grad_fold_list_kernel(const float* __restrict__ dx, float* __restrict__ out,
                                                                    const int* __restrict__ first, int n, int l0, int bpf, int F, int HW, int k,
                                                                    float scale) {
    const int l = l0 + (int)(blockIdx.x / bpf);
    const int w = 2 * k + 1;
    const int per_frame = F * HW / V;  // HW % V == 0: a vector never straddles two planes
    for (int i = (int)(blockIdx.x % bpf) * blockDim.x + threadIdx.x; i < per_frame; i += bpf * blockDim.x) {
        float s[V];
#pragma unroll
        for (int e = 0; e < V; ++e) s[e] = 0.f;
        bool any = false;
        for (int j = 0; j < n; ++j) {
            const int d = l - first[j];
            if (d < 0 || d >= w) continue;
            any = true;
            const float* src = dx + ((long long)j * w + d) * F * HW + (long long)i * V;
            if constexpr (V == 4) {
                const f32x4_t v = *(const f32x4_t*)src;
#pragma unroll
                for (int e = 0; e < V; ++e) s[e] += v[e];
            } else {
                s[0] += src[0];
            }
        }
        if (!any) continue;
        float* dst = out + (long long)l * F * HW + (long long)i * V;
        if constexpr (V == 4) {
            f32x4_t o = *(f32x4_t*)dst;
#pragma unroll
            for (int e = 0; e < V; ++e) o[e] += scale * s[e];
            *(f32x4_t*)dst = o;
        } else {
            dst[0] += scale * s[0];
        }
    }
}

// fold (src/thor/score.py:76-88 / _window_score :111-141): keep the centre frame of every window, the leading k frames of
// the first window and the trailing k frames of the last one.
// One thread per (window, pixel): the kept channels of a window are one contiguous run of its NHWC row -- [k F, (k+1) F) for an
// interior window, from 0 for the first, to w F for the last -- and land in the planes (gi F + c) of the trajectory.
template <typename T>
__global__ __launch_bounds__(256) void window_scatter_kernel(const T* __restrict__ y, float* __restrict__ eps, int nw, int F, int HW, int k,
                                                             int i0, int nwin_total, int ldc) {
    const int w = 2 * k + 1;
    const long long total = (long long)nw * HW;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int pix = (int)(i % HW);
        const int j = (int)(i / HW);
        const int gi = i0 + j;
        const int c_lo = gi == 0 ? 0 : k * F;
        const int c_hi = gi == nwin_total - 1 ? w * F : (k + 1) * F;
        const T* row = y + ((size_t)j * HW + pix) * ldc;
        float* dst = eps + (long long)gi * F * HW + pix;
        for (int c = c_lo; c < c_hi; ++c) dst[(long long)c * HW] = Elem<T>::ld(row + c);
    }
}

// predictor (src/thor/pipelines.py:41-46):  x <- mu' (x - sigma eps)/mu + sigma' eps  =  a x + b eps ; NaN/Inf raises `flag`
__global__ __launch_bounds__(256) void predict_kernel(float* __restrict__ x, const float* __restrict__ eps, int* __restrict__ flag, long long n,
                                                      float a, float b) {
    bool bad = false;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float v = a * x[i] + b * eps[i];
        x[i] = v;
        bad |= !(fabsf(v) <= 3.0e38f);
    }
    if (flag != nullptr && __any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ v, float* __restrict__ out, long long n) {
    float s = 0.f;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) s += v[i] * v[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) atomicAdd(out, s);
}

// corrector (src/thor/pipelines.py:81-88): delta = tau / mean(eps^2) ; x <- x - (delta eps + sqrt(2 delta) z) sigma'
__global__ __launch_bounds__(256) void correct_kernel(float* __restrict__ x, const float* __restrict__ eps, const float* __restrict__ z,
                                                      const float* __restrict__ sumsq, int* __restrict__ flag, long long n, float tau,
                                                      float sigma_next) {
    const float delta = tau / (sumsq[0] / (float)n);
    const float sd = sqrtf(2.f * delta);
    bool bad = false;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float v = x[i] - (delta * eps[i] + sd * z[i]) * sigma_next;
        x[i] = v;
        bad |= !(fabsf(v) <= 3.0e38f);
    }
    if (flag != nullptr && __any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

// Gaussian-likelihood guidance with the reference's measurement operator A = AvgPool2d(s) o x[::t_step]
// (exp/downscaling.py:129-132) and exact_grad=False (src/thor/score.py:28-57, all shipped configs):
//   x0 = (x - sigma eps)/mu ; err = y - A(x0) ; var = std_c^2 + gamma_c (sigma/mu)^2
// (std and gamma per variable c: exp/downscaling.py:219-233 builds both as (1, C, 1, 1) tensors for list-valued settings;
//  gammav == nullptr: the scalar `gamma` for every variable)
//   eps <- eps - sigma * (1/mu) * A^T(err/var)          (A^T spreads err/(var s^2) over the s x s cell)
// one wave per (observed frame, channel, pooled cell)
// DELTA: eps is only read and delta[o][c][H][W] (compact: observed frames only) = -corr is written instead -- what exact guidance puts on
// the network's output gradient; eps + delta is then bit for bit the eps the in-place form leaves (a + (-b) == a - b).
template <bool DELTA>
__global__ __launch_bounds__(256) void guidance_kernel(const float* __restrict__ x, float* __restrict__ eps, const float* __restrict__ yobs,
                                                       const float* __restrict__ stdv, const float* __restrict__ gammav, float* __restrict__ delta, int nobs,
                                                       int F, int H, int W, int s, int t_step, float mu, float sigma, float gamma) {
    const int lane = threadIdx.x & 63;
    const int PH = H / s, PW = W / s;
    const long long ncell = (long long)nobs * F * PH * PW;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (wave >= ncell) return;
    const int pw = (int)(wave % PW);
    long long r = wave / PW;
    const int ph = (int)(r % PH);
    r /= PH;
    const int c = (int)(r % F);
    const int o = (int)(r / F);
    const long long base = (((long long)o * t_step) * F + c) * H * W;
    float acc = 0.f;
    for (int q = lane; q < s * s; q += 64) {
        const long long idx = base + (long long)(ph * s + q / s) * W + pw * s + q % s;
        acc += (x[idx] - sigma * eps[idx]) / mu;
    }
    const float mean = wave_sum(acc) / (float)(s * s);
    const float sd = stdv[c];
    const float ratio = sigma / mu;
    const float var = sd * sd + (gammav != nullptr ? gammav[c] : gamma) * ratio * ratio;
    const float err = yobs[(((long long)o * F + c) * PH + ph) * PW + pw] - mean;
    const float corr = sigma * (err / var) / (mu * (float)(s * s));
    if constexpr (DELTA) {
        const long long dbase = ((long long)o * F + c) * H * W;
        for (int q = lane; q < s * s; q += 64) delta[dbase + (long long)(ph * s + q / s) * W + pw * s + q % s] = -corr;
    } else {
        for (int q = lane; q < s * s; q += 64) {
            const long long idx = base + (long long)(ph * s + q / s) * W + pw * s + q % s;
            eps[idx] -= corr;
        }
    }
}

// Measurement operator of the experiments, y = A(x) = AvgPool2d(s)(x[::t_step]) (exp/downscaling.py:129-132):
// one wave per (observed frame, channel, pooled cell); builds the observation from a high-resolution trajectory in HBM.
__global__ __launch_bounds__(256) void pool_stride_kernel(const float* __restrict__ x, float* __restrict__ y, int nobs, int F, int H, int W,
                                                          int s, int t_step) {
    const int lane = threadIdx.x & 63;
    const int PH = H / s, PW = W / s;
    const long long ncell = (long long)nobs * F * PH * PW;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (wave >= ncell) return;
    const int pw = (int)(wave % PW);
    long long r = wave / PW;
    const int ph = (int)(r % PH);
    r /= PH;
    const int c = (int)(r % F);
    const int o = (int)(r / F);
    const long long base = (((long long)o * t_step) * F + c) * H * W;
    float acc = 0.f;
    for (int q = lane; q < s * s; q += 64) acc += x[base + (long long)(ph * s + q / s) * W + pw * s + q % s];
    acc = wave_sum(acc);
    if (lane == 0) y[wave] = acc / (float)(s * s);
}

// Per-variable affine map y[l][c][:] = x[l][c][:] * scale[c] + shift[c]: the quantile (de)normalisation of
// data/pipeline.py:183-244 (all five modes are of this form) applied to an (L, F, H, W) trajectory in place or out of place.
__global__ __launch_bounds__(256) void affine_channels_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ scale,
                                                              const float* __restrict__ shift, long long planes, int F, int HW) {
    const int nv = HW >> 2;  // HW % 4 == 0 checked by the launcher
    const long long total = planes * nv;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long plane = i / nv;
        const int c = (int)(plane % F);
        const float a = scale[c], b = shift[c];
        f32x4_t v = ((const f32x4_t*)x)[i];
        v = v * a + b;
        ((f32x4_t*)y)[i] = v;
    }
}

}  // namespace

extern "C" int c2w_window_gather(const float* x, void* y, int nw, int F, int HW, int k, int i0, int ldc, int dtype, void* stream) {
    const int CW = (2 * k + 1) * F;
    const int P = dtype == C2W_DTYPE_F32 ? 4 : 8;
    if (!x || !y || nw <= 0 || ldc < CW || ldc % P) return C2W_ERR_BAD_SHAPE;
    // a window's (w F, H, W) tensor is the contiguous run of planes starting at frame i0 + j: the LDS-tiled plane -> row kernel
    // with an image stride of one frame (pointwise.hip); the per-thread gather below is the fallback for shapes it does not take
    if (c2w_planes_to_rows_strided(x + (long long)i0 * F * HW, y, nw, CW, HW, ldc, (long long)F * HW, dtype, (hipStream_t)stream) == 0)
        return (int)hipGetLastError();
    const long long total = (long long)nw * HW * (ldc / P);
    if (dtype == C2W_DTYPE_F32)
        window_gather_kernel<float><<<grid_for(total), 256, 0, (hipStream_t)stream>>>(x, (float*)y, nw, CW, HW, (long long)F * HW, i0, ldc);
    else if (dtype == C2W_DTYPE_BF16)
        window_gather_kernel<bf16_t><<<grid_for(total), 256, 0, (hipStream_t)stream>>>(x, (bf16_t*)y, nw, CW, HW, (long long)F * HW, i0, ldc);
    else if (dtype == C2W_DTYPE_F16)
        window_gather_kernel<f16_t><<<grid_for(total), 256, 0, (hipStream_t)stream>>>(x, (f16_t*)y, nw, CW, HW, (long long)F * HW, i0, ldc);
    else
        return C2W_ERR_BAD_ARG;
    return (int)hipGetLastError();
}

extern "C" int c2w_window_scatter(const void* y, float* eps, int nw, int F, int HW, int k, int i0, int nwin_total, int ldc, int dtype,
                                  void* stream) {
    if (!y || !eps || nw <= 0 || ldc < (2 * k + 1) * F) return C2W_ERR_BAD_SHAPE;
    const long long total = (long long)nw * HW;
    if (dtype == C2W_DTYPE_F32)
        window_scatter_kernel<float><<<grid_for(total), 256, 0, (hipStream_t)stream>>>((const float*)y, eps, nw, F, HW, k, i0, nwin_total, ldc);
    else if (dtype == C2W_DTYPE_BF16)
        window_scatter_kernel<bf16_t><<<grid_for(total), 256, 0, (hipStream_t)stream>>>((const bf16_t*)y, eps, nw, F, HW, k, i0, nwin_total, ldc);
    else if (dtype == C2W_DTYPE_F16)
        window_scatter_kernel<f16_t><<<grid_for(total), 256, 0, (hipStream_t)stream>>>((const f16_t*)y, eps, nw, F, HW, k, i0, nwin_total, ldc);
    else
        return C2W_ERR_BAD_ARG;
    return (int)hipGetLastError();
}

extern "C" int c2w_sampler_predict(float* x, const float* eps, int* nan_flag, long long n, float a, float b, void* stream) {
    if (!x || !eps) return C2W_ERR_BAD_ARG;
    predict_kernel<<<grid_for(n), 256, 0, (hipStream_t)stream>>>(x, eps, nan_flag, n, a, b);
    return (int)hipGetLastError();
}

extern "C" int c2w_sumsq(const float* v, float* out, long long n, void* stream) {
    if (!v || !out) return C2W_ERR_BAD_ARG;
    sumsq_kernel<<<grid_for(n, 256, 2048), 256, 0, (hipStream_t)stream>>>(v, out, n);
    return (int)hipGetLastError();
}

extern "C" int c2w_sampler_correct(float* x, const float* eps, const float* z, const float* sumsq, int* nan_flag, long long n, float tau,
                                   float sigma_next, void* stream) {
    if (!x || !eps || !z || !sumsq) return C2W_ERR_BAD_ARG;
    correct_kernel<<<grid_for(n), 256, 0, (hipStream_t)stream>>>(x, eps, z, sumsq, nan_flag, n, tau, sigma_next);
    return (int)hipGetLastError();
}

static int guidance_launch(const float* x, float* eps, const float* yobs, const float* stdv, const float* gammav, int nobs, int F, int H, int W,
                           int s_step, int t_step, float mu, float sigma, float gamma, void* stream) {
    if (!x || !eps || !yobs || !stdv || nobs <= 0 || s_step <= 0 || H % s_step || W % s_step || t_step <= 0) return C2W_ERR_BAD_SHAPE;
    const long long ncell = (long long)nobs * F * (H / s_step) * (W / s_step);
    const long long blocks = (ncell + 3) / 4;
    guidance_kernel<false><<<(int)blocks, 256, 0, (hipStream_t)stream>>>(x, eps, yobs, stdv, gammav, nullptr, nobs, F, H, W, s_step, t_step, mu,
                                                                         sigma, gamma);
    return (int)hipGetLastError();
}

extern "C" int c2w_guidance(const float* x, float* eps, const float* yobs, const float* stdv, int nobs, int F, int H, int W, int s_step,
                            int t_step, float mu, float sigma, float gamma, void* stream) {
    return guidance_launch(x, eps, yobs, stdv, nullptr, nobs, F, H, W, s_step, t_step, mu, sigma, gamma, stream);
}

extern "C" int c2w_guidance_per_variable(const float* x, float* eps, const float* yobs, const float* stdv, const float* gammav, int nobs, int F,
                                         int H, int W, int s_step, int t_step, float mu, float sigma, void* stream) {
    if (!gammav) return C2W_ERR_BAD_ARG;
    return guidance_launch(x, eps, yobs, stdv, gammav, nobs, F, H, W, s_step, t_step, mu, sigma, 0.f, stream);
}

extern "C" int c2w_guidance_delta(const float* x, const float* eps, const float* yobs, const float* stdv, const float* gammav_or_null, float gamma,
                                  float* delta, int nobs, int F, int H, int W, int s_step, int t_step, float mu, float sigma, void* stream) {
    if (!x || !eps || !yobs || !stdv || !delta || nobs <= 0 || F <= 0 || s_step <= 0 || H % s_step || W % s_step || t_step <= 0)
        return C2W_ERR_BAD_SHAPE;
    const long long ncell = (long long)nobs * F * (H / s_step) * (W / s_step);
    const long long blocks = (ncell + 3) / 4;
    guidance_kernel<true><<<(int)blocks, 256, 0, (hipStream_t)stream>>>(x, const_cast<float*>(eps), yobs, stdv, gammav_or_null, delta, nobs, F, H,
                                                                        W, s_step, t_step, mu, sigma, gamma);
    return (int)hipGetLastError();
}

extern "C" int c2w_window_gather_list(const float* x, void* y, const int* first, int n, int F, int HW, int k, int ldc, int dtype, void* stream) {
    const int CW = (2 * k + 1) * F;
    const int P = dtype == C2W_DTYPE_F32 ? 4 : 8;
    if (!x || !y || !first || n <= 0 || F <= 0 || HW <= 0 || k < 0 || ldc < CW || ldc % P) return C2W_ERR_BAD_SHAPE;
    const long long total = (long long)n * HW * (ldc / P);
    if (dtype == C2W_DTYPE_F32)
        window_gather_list_kernel<float><<<grid_for(total), 256, 0, (hipStream_t)stream>>>(x, (float*)y, first, n, CW, HW, (long long)F * HW, ldc);
    else if (dtype == C2W_DTYPE_BF16)
        window_gather_list_kernel<bf16_t><<<grid_for(total), 256, 0, (hipStream_t)stream>>>(x, (bf16_t*)y, first, n, CW, HW, (long long)F * HW, ldc);
    else if (dtype == C2W_DTYPE_F16)
        window_gather_list_kernel<f16_t><<<grid_for(total), 256, 0, (hipStream_t)stream>>>(x, (f16_t*)y, first, n, CW, HW, (long long)F * HW, ldc);
    else
        return C2W_ERR_BAD_ARG;
    return (int)hipGetLastError();
}

extern "C" int c2w_window_cotangent_list(const float* delta, void* dy, const int* first, const int* kind, int n, int L, int F, int HW, int k,
                                         int t_step, int nobs, int ldc, int dtype, void* stream) {
    const int P = dtype == C2W_DTYPE_F32 ? 4 : 8;
    if (!delta || !dy || !first || !kind || n <= 0 || L < 2 * k + 1 || F <= 0 || HW <= 0 || k < 0 || t_step <= 0 || nobs <= 0 ||
        (long long)(nobs - 1) * t_step >= L || ldc < (2 * k + 1) * F || ldc % P)
        return C2W_ERR_BAD_SHAPE;
    const long long total = (long long)n * HW * (ldc / P);
    if (dtype == C2W_DTYPE_F32)
        window_cotangent_list_kernel<float><<<grid_for(total), 256, 0, (hipStream_t)stream>>>(delta, (float*)dy, first, kind, n, L, F, HW, k, t_step,
                                                                                              nobs, ldc);
    else if (dtype == C2W_DTYPE_BF16)
        window_cotangent_list_kernel<bf16_t><<<grid_for(total), 256, 0, (hipStream_t)stream>>>(delta, (bf16_t*)dy, first, kind, n, L, F, HW, k,
                                                                                               t_step, nobs, ldc);
    else if (dtype == C2W_DTYPE_F16)
        window_cotangent_list_kernel<f16_t><<<grid_for(total), 256, 0, (hipStream_t)stream>>>(delta, (f16_t*)dy, first, kind, n, L, F, HW, k, t_step,
                                                                                              nobs, ldc);
    else
        return C2W_ERR_BAD_ARG;
    return (int)hipGetLastError();
}

extern "C" int c2w_window_grad_fold_list(const float* dx, float* out, const int* first, int n, int l0, int nl, int F, int HW, int k, float scale,
                                         void* stream) {
    if (!dx || !out || !first || n <= 0 || l0 < 0 || nl <= 0 || F <= 0 || HW <= 0 || k < 0) return C2W_ERR_BAD_SHAPE;
    const int V = HW % 4 == 0 ? 4 : 1;
    const long long per_frame = (long long)F * HW / V;
    if (per_frame > 0x7fffffffLL) return C2W_ERR_BAD_SHAPE;
    long long bpf = (per_frame + 1023) / 1024;  // a thread owns up to four vectors of its frame
    if (bpf > 64) bpf = 64;
    if (bpf * nl > 0x7fffffffLL) return C2W_ERR_BAD_SHAPE;
    const unsigned grid = (unsigned)(bpf * nl);
    if (V == 4)
        window_grad_fold_list_kernel<4><<<grid, 256, 0, (hipStream_t)stream>>>(dx, out, first, n, l0, (int)bpf, F, HW, k, scale);
    else
        window_grad_fold_list_kernel<1><<<grid, 256, 0, (hipStream_t)stream>>>(dx, out, first, n, l0, (int)bpf, F, HW, k, scale);
    return (int)hipGetLastError();
}

extern "C" int c2w_pool_stride(const float* x, float* y, int nobs, int F, int H, int W, int s_step, int t_step, void* stream) {
    if (!x || !y || nobs <= 0 || F <= 0 || s_step <= 0 || t_step <= 0 || H % s_step || W % s_step) return C2W_ERR_BAD_SHAPE;
    const long long ncell = (long long)nobs * F * (H / s_step) * (W / s_step);
    pool_stride_kernel<<<(unsigned)((ncell * 64 + 255) / 256), 256, 0, (hipStream_t)stream>>>(x, y, nobs, F, H, W, s_step, t_step);
    return (int)hipGetLastError();
}

extern "C" int c2w_affine_channels(const float* x, float* y, const float* scale, const float* shift, long long planes, int F, int HW,
                                   void* stream) {
    if (!x || !y || !scale || !shift || planes <= 0 || F <= 0 || HW <= 0 || HW % 4) return C2W_ERR_BAD_SHAPE;
    affine_channels_kernel<<<grid_for(planes * (HW / 4)), 256, 0, (hipStream_t)stream>>>(x, y, scale, shift, planes, F, HW);
    return (int)hipGetLastError();
}
