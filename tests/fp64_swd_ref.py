"""The sliced Wasserstein distance restated in float64, the rule it is judged by, and the test fields (shared by tests/test_swd_cpu.py and
tests/test_gpu_swd.py).

The definition (include/c2w_hip.h: c2w_swd_project, c2w_swd_distance; recalled from an optimal-transport library that is not available
here), line by line:

    theta = numpy.random.RandomState(seed).randn(d, P); theta /= sqrt(sum(theta^2, axis 0))      ``theta64``
    a = X theta_p, b = Y theta_p                                                                 ``project64``
    D_p = mean_i (sort(a)_i - sort(b)_i)^2                                                        ``d64``
    SWD = sqrt(mean_p D_p)                                                                        ``swd64``
    and both arrays normalised by the truth's mean and population std first                      ``swd_reference``

The rule is the project's (tests/fp64_ssim_ref.py: FACTOR = 4, FLOOR = 16 * 2^-24) with a dot product's scale:

* a projection entry, against float64 on the same fp32 x, theta, shift, scale with x^ formed in fp32 as the kernel forms it:
      |err| <= 4 * max(|fp32 torch.matmul route - float64| on that entry, 16 * 2^-24 * sum_k |x^_k theta_k|)          ``proj_bound``
* the distance kernel on given fp32 columns: sorting is exact and the rest is double, relative error <= T * 2^-52       ``D_RTOL``
* end to end: W_2 in one dimension is 1-Lipschitz in each argument under the rms norm, so
      |sqrt(D_p) - sqrt(D_p64)| <= delta_p = rms_t(bound_a) + rms_t(bound_b),   |SWD - SWD64| <= sqrt(mean_p delta_p^2)  ``e2e``
  with no free constant.

``project_naive32`` is the port that is NOT careful -- project the raw field in a straight fp32 loop, normalise afterwards: (theta . x -
shift sum(theta)) * scale -- the negative control, which the rule must refuse on a field with a large offset at the reference's 128 x 128
(|x| is 84 times |x^| on a pressure field, so the chain's rounding is measured against a sum 84 times the rule's; measured: up to 1.9
times the bound, 0.42 at the median, so not every entry passes).  The same loop on x^ formed first (``chain32``) stays at 0.014 of the
bound: it is the offset that does it.  A blocked summation hides the trap at this size -- the naive algebra through torch.matmul reaches
0.33 of the bound -- which is no reason to rely on it.
"""
import numpy as np
import torch
from scipy import ndimage

U = 2.0 ** -24
FLOOR = 16.0 * U
FACTOR = 4.0


def D_RTOL(T):
    return T * 2.0 ** -52


# ------------------------------------------------------------------------------------------------------------------ the definition

def theta64(d, P=100, seed=0):
    """(d, P) float64 unit columns: the library's numpy backend, seed(seed); randn(d, P)"""
    theta = np.random.RandomState(seed).randn(d, P)
    return theta / np.sqrt(np.sum(theta ** 2, axis=0, keepdims=True))


_THETA = {}


def theta32(d, P=100, seed=0):
    """(P, d) fp32, K contiguous: the operand the kernel is handed (computed once per (d, P, seed), shared and left unchanged)"""
    if (d, P, seed) not in _THETA:
        th = np.ascontiguousarray(theta64(d, P, seed).T).astype(np.float32)
        th.setflags(write=False)
        _THETA[(d, P, seed)] = th
    return _THETA[(d, P, seed)]


def xhat32(x, shift, scale):
    """(x - shift) * scale in fp32, two roundings: x (..., F, d), shift and scale (F,)"""
    x = np.asarray(x, dtype=np.float32)
    s, c = np.asarray(shift, dtype=np.float32)[:, None], np.asarray(scale, dtype=np.float32)[:, None]
    out = (x - s) * c
    assert out.dtype == np.float32
    return out


def project64(xh, th):
    """xh (..., d) fp32 values, th (P, d) fp32 values -> (..., P) float64"""
    return np.asarray(xh, dtype=np.float64) @ np.asarray(th, dtype=np.float64).T


def abs_sum(xh, th):
    """sum_k |x^_k theta_k| per entry, float64"""
    return np.abs(np.asarray(xh, dtype=np.float64)) @ np.abs(np.asarray(th, dtype=np.float64)).T


def project_matmul32(xh, th):
    """the yardstick: fp32 torch.matmul on the CPU"""
    xh = np.ascontiguousarray(xh, dtype=np.float32)
    got = torch.matmul(torch.from_numpy(xh.reshape(-1, xh.shape[-1])), torch.tensor(np.asarray(th, dtype=np.float32)).t())
    assert got.dtype == torch.float32
    return got.numpy().reshape(xh.shape[:-1] + (th.shape[0],)).astype(np.float64)


def chain32(a, b):
    """a (..., d), b (P, d) -> (..., P): sum_k a_k b_k as a straight fp32 loop over k (products rounded, one running sum), what a
    one-thread-per-output port does"""
    prod = np.asarray(a, dtype=np.float32)[..., None, :] * np.asarray(b, dtype=np.float32)
    assert prod.dtype == np.float32
    return np.cumsum(prod, axis=-1, dtype=np.float32)[..., -1]


def project_naive32(x, th, shift, scale):
    """project first, normalise afterwards, a straight fp32 port: x (..., F, d) -> (..., F, P) = (theta . x - shift sum(theta)) * scale"""
    th = np.asarray(th, dtype=np.float32)
    s, c = np.asarray(shift, dtype=np.float32)[:, None], np.asarray(scale, dtype=np.float32)[:, None]
    out = (chain32(x, th) - s * chain32(np.ones(th.shape[1], np.float32), th)[None, :]) * c
    assert out.dtype == np.float32
    return out.astype(np.float64)


def proj_bound(xh, th, p64=None):
    """FACTOR * max(the yardstick's error on the entry, FLOOR * sum |x^ theta|), per entry"""
    p64 = project64(xh, th) if p64 is None else p64
    return FACTOR * np.maximum(np.abs(project_matmul32(xh, th) - p64), FLOOR * abs_sum(xh, th))


def d64(a, b):
    """a (..., T), b (..., T) columns -> mean_i (sort(a)_i - sort(b)_i)^2 in float64"""
    a, b = np.sort(np.asarray(a, dtype=np.float64), axis=-1), np.sort(np.asarray(b, dtype=np.float64), axis=-1)
    return ((a - b) ** 2).mean(axis=-1)


def swd64(X, Y, th, per_projection=False):
    """X (T, d), Y (T, d) already normalised, th (P, d) -> SWD (or the D_p)"""
    D = d64(project64(X, th).T, project64(Y, th).T)
    return D if per_projection else float(np.sqrt(D.mean()))


def e2e(samples, truth, th, shift, scale):
    """samples (n_rep, T, F, d), truth (T, F, d), th (P, d), shift / scale (F,) fp32 values ->
    (D64 (n_rep, F, P), delta (n_rep, F, P)): the float64 D_p on the fp32-formed x^ and the bound on |sqrt(D_p) - sqrt(D64_p)|"""
    xs, xt = xhat32(samples, shift, scale), xhat32(truth, shift, scale)
    ps, pt = project64(xs, th), project64(xt, th)                    # (n_rep, T, F, P), (T, F, P)
    bs, bt = proj_bound(xs, th, ps), proj_bound(xt, th, pt)
    D = d64(np.moveaxis(ps, 1, -1), np.moveaxis(pt, 0, -1)[None])   # (n_rep, F, P)
    rms = lambda b, ax: np.sqrt((b ** 2).mean(axis=ax))
    return D, rms(bs, 1) + rms(bt, 0)[None]


def swd_of(D):
    return np.sqrt(D.mean(axis=-1))


def swd_bound(delta):
    return np.sqrt((delta ** 2).mean(axis=-1))


def dp_bound(D, delta):
    """|D_p - D64_p| from |sqrt(D_p) - sqrt(D64_p)| <= delta"""
    return delta * (2.0 * np.sqrt(D) + delta)


# ------------------------------------------------------------------------------------------------------------------ the reference's loop

def swd_reference(sample_arr, gt_arr, n_projections=100, seed=0):
    """exp/metrics.py:254-264 and :13-44 restated line by line with swd64 in the library call's place:
    (M, T, H, W), (T, H, W) of one variable -> (wasserstein_array (M,), gtmean, gtstd), everything in float64"""
    sample_arr, gt_arr = np.asarray(sample_arr, dtype=np.float64), np.asarray(gt_arr, dtype=np.float64)
    gtmean, gtstd = gt_arr.mean(), gt_arr.std()
    sample_norm, gt_norm = (sample_arr - gtmean) / gtstd, (gt_arr - gtmean) / gtstd
    num_times, num_space = gt_norm.shape[0], gt_norm.shape[1] * gt_norm.shape[2]
    gt_vals = gt_norm.reshape(num_times, num_space)
    num_samples = sample_norm.shape[0]
    th = theta64(num_space, n_projections, seed).T
    wasserstein_array = np.zeros((num_samples,))
    for smpl_id in range(num_samples):
        wasserstein_array[smpl_id] = swd64(sample_norm[smpl_id].reshape(num_times, num_space), gt_vals, th)
    return wasserstein_array, gtmean, gtstd


# ------------------------------------------------------------------------------------------------------------------ fields

KINDS = ("white", "smooth", "constant", "temperature", "pressure")


def _smooth(shape, rng):
    z = ndimage.gaussian_filter1d(rng.standard_normal(shape), sigma=3.0, axis=-1, mode="wrap")
    return z / z.std()


def fields(kind, n_rep, T, F, d, seed=0):
    """(samples (n_rep, T, F, d) fp32, truth (T, F, d) fp32, shift (F,) fp32, scale (F,) fp32): variable f differs from its
    neighbours in offset and spread, so a wrong i % F shows; the moments are the truth's own (mean, 1 / population std) except for
    the constant kind, whose std is zero (shift f / 4, scale 1 / (1 + f))"""
    rng = np.random.default_rng(seed + 7919 * KINDS.index(kind) + d + 31 * T)
    f = np.arange(F, dtype=np.float64)[:, None]
    if kind == "white":
        base = lambda lead: f + (1.0 + f) * rng.standard_normal(lead + (F, d))
    elif kind == "smooth":
        base = lambda lead: 0.5 * f + (1.0 + 0.5 * f) * _smooth(lead + (F, d), rng)
    elif kind == "constant":
        base = lambda lead: np.broadcast_to(3.5 + f, lead + (F, d)).copy()
    elif kind == "temperature":
        base = lambda lead: 280.0 + 5.0 * f + 10.0 * _smooth(lead + (F, d), rng) + 2.0 * rng.standard_normal(lead + (F, d))
    elif kind == "pressure":
        base = lambda lead: 101325.0 - 300.0 * f + 1200.0 * _smooth(lead + (F, d), rng) + 300.0 * rng.standard_normal(lead + (F, d))
    else:
        raise KeyError(kind)
    truth, samples = base((T,)).astype(np.float32), base((n_rep, T)).astype(np.float32)
    if kind == "constant":
        shift, scale = 0.25 * f[:, 0], 1.0 / (1.0 + f[:, 0])
    else:
        t64 = truth.astype(np.float64)
        shift, scale = t64.mean(axis=(0, 2)), 1.0 / t64.std(axis=(0, 2))
    return samples, truth, shift.astype(np.float32), scale.astype(np.float32)
