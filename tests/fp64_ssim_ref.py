"""The mean SSIM under a uniform window restated in float64, the yardstick it is judged by, and the test fields (shared by
tests/test_ssim_cpu.py and tests/test_gpu_ssim.py).

``ssim64`` is the definition (include/c2w_hip.h: c2w_ssim) with nothing clever in it: ``scipy.ndimage.uniform_filter`` in float64 -- the
filter the image library calls -- the straight ``E[xx] - E[x]^2``, the crop by ``(win - 1) / 2``.  ``ssim_yardstick`` is the same
definition in float32 with CPU ``torch.avg_pool2d``, both fields pivoted by the truth's mean before any product and the luminance factor
formed from ``u_x - u_y``: what a careful user of the vendor route gets.  A score S passes against the float64 S64 if

    |S - S64| <= 4 * max(|yardstick - S64| on that very pair, 16 * 2^-24)

the factor and the floor being those of tests/fp64_spectrum_ref.py.  ``ssim_straight32`` is the port that is NOT careful (fp32,
no pivot): the negative control, which the rule must refuse on a field with a large offset.
"""
import numpy as np
import torch
from scipy import ndimage

FLOOR = 16.0 * 2.0 ** -24
FACTOR = 4.0


def ssim64(x, y, R, win):
    """x, y (H, W) array-likes, data range R, odd window -> float: the mean of S over the windows inside the field"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    NP = win * win
    cn = NP / (NP - 1.0)
    ux, uy = ndimage.uniform_filter(x, size=win), ndimage.uniform_filter(y, size=win)
    uxx, uyy, uxy = ndimage.uniform_filter(x * x, size=win), ndimage.uniform_filter(y * y, size=win), ndimage.uniform_filter(x * y, size=win)
    vx, vy, vxy = cn * (uxx - ux * ux), cn * (uyy - uy * uy), cn * (uxy - ux * uy)
    C1, C2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
    pad = (win - 1) // 2
    return float(S[pad:S.shape[0] - pad, pad:S.shape[1] - pad].mean())


def _pool32(a, win):
    return torch.nn.functional.avg_pool2d(a[None, None], win, stride=1)[0, 0]


def ssim_yardstick(x, y, R, win):
    """float32 avg_pool2d on the CPU, pivoted by the truth's mean; the final mean over the windows in float64"""
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    p = np.float32(np.asarray(y, dtype=np.float64).mean())
    a, b = torch.from_numpy(x - p), torch.from_numpy(y - p)
    NP = win * win
    cn = np.float32(NP / (NP - 1.0))
    ua, ub, uaa, ubb, uab = _pool32(a, win), _pool32(b, win), _pool32(a * a, win), _pool32(b * b, win), _pool32(a * b, win)
    va, vb, vab = cn * (uaa - ua * ua), cn * (ubb - ub * ub), cn * (uab - ua * ub)
    C1, C2 = np.float32((0.01 * R) ** 2), np.float32((0.03 * R) ** 2)
    ux, uy, d = ua + p, ub + p, ua - ub
    S = (1.0 - d * d / (ux * ux + uy * uy + C1)) * ((2.0 * vab + C2) / (va + vb + C2))
    assert S.dtype == torch.float32
    return float(S.double().mean())


def ssim_straight32(x, y, R, win):
    """float32 avg_pool2d of the fields as they are: E[xx] - E[x]^2 at the size of offset^2"""
    a, b = torch.from_numpy(np.array(x, dtype=np.float32)), torch.from_numpy(np.array(y, dtype=np.float32))
    NP = win * win
    cn = np.float32(NP / (NP - 1.0))
    ua, ub, uaa, ubb, uab = _pool32(a, win), _pool32(b, win), _pool32(a * a, win), _pool32(b * b, win), _pool32(a * b, win)
    va, vb, vab = cn * (uaa - ua * ua), cn * (ubb - ub * ub), cn * (uab - ua * ub)
    C1, C2 = np.float32((0.01 * R) ** 2), np.float32((0.03 * R) ** 2)
    S = ((2.0 * ua * ub + C1) * (2.0 * vab + C2)) / ((ua * ua + ub * ub + C1) * (va + vb + C2))
    return float(S.double().mean())


def bound(x, y, R, win, S64=None):
    """FACTOR * max(the yardstick's error on this pair, FLOOR)"""
    S64 = ssim64(x, y, R, win) if S64 is None else S64
    return FACTOR * max(abs(ssim_yardstick(x, y, R, win) - S64), FLOOR)


def pair_range(x, y):
    """the reference's data range over one pair, as the fp32 number the kernel is handed"""
    return float(np.float32(max(np.max(x), np.max(y)) - min(np.min(x), np.min(y))))


# ------------------------------------------------------------------------------------------------------------------ the reference's loop

def ssim_reference(sample_arr, gt_arr, win=15):
    """exp/metrics.py:187-212 restated line by line with ssim64 in the library call's place: (M, T, H, W), (T, H, W) ->
    (ssim_values (M, T), their mean over time (M,), data_range)"""
    sample_arr, gt_arr = np.asarray(sample_arr), np.asarray(gt_arr)
    num_samples, num_timesteps = sample_arr.shape[:2]
    data_range = float(max(gt_arr.max(), sample_arr.max()) - min(gt_arr.min(), sample_arr.min()))
    ssim_values = np.zeros((num_samples, num_timesteps))
    for s in range(num_samples):
        for t in range(num_timesteps):
            ssim_values[s, t] = ssim64(sample_arr[s, t], gt_arr[t], data_range, win)
    return ssim_values, ssim_values.mean(1), data_range


# ------------------------------------------------------------------------------------------------------------------ fields

def smooth(H, W, seed, sigma=3.0):
    """white noise under a periodic Gaussian filter, zero mean and unit standard deviation"""
    z = ndimage.gaussian_filter(np.random.default_rng(seed).standard_normal((H, W)), sigma=sigma, mode="wrap")
    return (z - z.mean()) / z.std()


def white(H, W, seed):
    return np.random.default_rng(seed).standard_normal((H, W))


def impulse(H, W, i, j):
    x = np.zeros((H, W))
    x[i % H, j % W] = 1.0
    return x


KINDS = ("smooth", "white", "identical", "anti", "const_truth", "impulse", "temperature", "pressure")


def pairs(H, W, seed=0):
    """kind -> (x, y) fp32, x the sample and y the truth"""
    s = seed + 1000 * H + W
    t = smooth(H, W, s + 1)
    out = {
        "smooth": (t + 0.3 * smooth(H, W, s + 2), t),
        "white": (white(H, W, s + 3), white(H, W, s + 4)),
        "identical": (white(H, W, s + 5),) * 2,
        "anti": (3.0 - t + 0.1 * white(H, W, s + 6), 3.0 + t),
        "const_truth": (white(H, W, s + 7), np.full((H, W), 0.75)),
        "impulse": (impulse(H, W, H // 2 + 1, W // 2), impulse(H, W, H // 2, W // 2)),
        "temperature": (280.0 + 10.0 * t + 2.0 * white(H, W, s + 8), 280.0 + 10.0 * t),
        "pressure": (101325.0 + 1200.0 * t + 300.0 * white(H, W, s + 9), 101325.0 + 1200.0 * t),
    }
    return {k: (a.astype(np.float32), b.astype(np.float32)) for k, (a, b) in out.items()}


_CACHE = {}


def cases(H, W, win):
    """(kinds, x (8, H, W), y (8, H, W), R (8,) fp32, S64 (8,), bound (8,)) -- computed once per shape, shared and left unchanged"""
    key = (H, W, win)
    if key not in _CACHE:
        p = pairs(H, W)
        x, y = np.stack([p[k][0] for k in KINDS]), np.stack([p[k][1] for k in KINDS])
        R = np.array([pair_range(x[i], y[i]) for i in range(len(KINDS))], dtype=np.float32)
        S64 = np.array([ssim64(x[i], y[i], float(R[i]), win) for i in range(len(KINDS))])
        b = np.array([bound(x[i], y[i], float(R[i]), win, S64[i]) for i in range(len(KINDS))])
        for a in (x, y, R, S64, b):
            a.setflags(write=False)
        _CACHE[key] = (KINDS, x, y, R, S64, b)
    return _CACHE[key]
