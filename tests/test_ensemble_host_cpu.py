"""CPU checks of the host layer the ensemble metrics share (climate2weather_amd.ensemble_host): the dense fp32 copy, the scratch
conventions, the chunk step, the argument checks word for word, and the seam -- every metric module decides its own route."""
import ast
import importlib
import os

import numpy as np
import pytest
import torch

from climate2weather_amd import ensemble_host as EH

METRICS = ("crps", "ssim", "spectra", "wasserstein", "marginals", "quantiles", "windpower", "multivariate")
PACKAGE = os.path.dirname(EH.__file__)


# ------------------------------------------------------------------------------------------------------------------ dense32

def _is_kernel_input(t):
    return t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0


def test_dense32_is_the_identity_on_a_dense_aligned_fp32_tensor():
    x = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4)
    assert _is_kernel_input(x) and EH.dense32(x) is x


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float64])
def test_dense32_copies_another_dtype_once(dtype):
    x = (torch.arange(24, dtype=torch.float32).reshape(2, 3, 4) / 8).to(dtype)  # exact in every one of the three
    out = EH.dense32(x)
    assert _is_kernel_input(out) and out.data_ptr() != x.data_ptr() and out.shape == x.shape
    assert torch.equal(out, x.to(torch.float32))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_dense32_copies_a_strided_input_once(dtype):
    base = torch.arange(48, dtype=torch.float32).reshape(4, 12).to(dtype)
    for x in (base[:, ::2], base.t(), base[1:3, 2:7]):
        assert not x.is_contiguous()
        out = EH.dense32(x)
        assert _is_kernel_input(out) and out.shape == x.shape and torch.equal(out, x.to(torch.float32))
    assert torch.equal(base, torch.arange(48, dtype=torch.float32).reshape(4, 12).to(dtype))  # the input is left as it was


def test_dense32_copies_a_misaligned_view_once():
    base = torch.arange(33, dtype=torch.float32)
    assert base.data_ptr() % 16 == 0
    x = base[1:]  # dense fp32, 4 bytes past the alignment
    assert x.is_contiguous() and x.data_ptr() % 16 == 4
    out = EH.dense32(x)
    assert _is_kernel_input(out) and out.data_ptr() != x.data_ptr() and torch.equal(out, x)


# ------------------------------------------------------------------------------------------------------------------ scratch, chunk_step

@pytest.mark.parametrize("dtype", [torch.float64, torch.int64])
def test_scratch_in_both_conventions(dtype):
    dev = torch.device("cpu")
    assert EH.scratch(0, dev, dtype) is None and EH.scratch(0, dev, dtype, optional=True) is None
    for optional, nbytes, numel in ((True, 8, 1), (True, 4096, 512), (False, 0, 1), (False, 8, 1), (False, 4096, 512)):
        s = EH.scratch(nbytes, dev, dtype, optional=optional)
        assert s.dtype == dtype and tuple(s.shape) == (numel,) and s.device == dev and s.numel() * s.element_size() >= nbytes
    assert EH.scratch(8, dev).dtype == torch.float64  # the default


def test_chunk_step():
    C = EH.CHUNK_ELEMS
    assert C == 1 << 22
    assert [EH.chunk_step(n) for n in (0, 1, C, C + 1)] == [C, C, 1, 1]
    assert [EH.chunk_step(n) for n in (2, 3, C - 1, C // 2, C // 2 + 1)] == [C // 2, C // 3, 1, 2, 1]
    for n in (0, 1, 7, 4 * 6 * 128 * 128, C + 1):
        assert EH.chunk_step(n) == max(1, C // max(1, n))  # the expression the general routes spelled out


# ------------------------------------------------------------------------------------------------------------------ the messages

def _raises(fn, *args, **kwargs):
    with pytest.raises(ValueError) as e:
        fn(*args, **kwargs)
    return str(e.value)


def test_check_ensemble_says_what_the_modules_said():
    s, t = torch.zeros(3, 2, 4, 5, 6), torch.zeros(2, 4, 5, 6)
    for kw in ({}, dict(time="L"), dict(members="M >= 1"), dict(time="L", members="M >= 1"), dict(floating=True)):
        assert EH.check_ensemble(s, t, **kw) is None
    wrong = [(s, t[:1]), (s[0], t), (s, t[0]), (s[:, :, :, :, :5], t)]
    for a, b in wrong:
        sa, sb = tuple(a.shape), tuple(b.shape)
        assert _raises(EH.check_ensemble, a, b) == f"samples {sa} must be (M,) + truth {sb} = (T, F, H, W)"
        assert _raises(EH.check_ensemble, a, b, floating=True) == f"samples {sa} must be (M,) + truth {sb} = (T, F, H, W)"
        assert _raises(EH.check_ensemble, a, b, time="L") == f"samples {sa} must be (M,) + truth {sb} = (L, F, H, W)"
        assert _raises(EH.check_ensemble, a, b, members="M >= 1") == f"samples {sa} must be (M >= 1,) + truth {sb} = (T, F, H, W)"
        assert _raises(EH.check_ensemble, a, b, time="L", members="M >= 1") == f"samples {sa} must be (M >= 1,) + truth {sb} = (L, F, H, W)"
    none = s[:0]
    assert EH.check_ensemble(none, t) is None and EH.check_ensemble(none, t, time="L", floating=True) is None  # M = 0 is the caller's to answer
    assert _raises(EH.check_ensemble, none, t, members="M >= 1") == "samples (0, 2, 4, 5, 6) must be (M >= 1,) + truth (2, 4, 5, 6) = (T, F, H, W)"
    assert _raises(EH.check_ensemble, none, t, time="L", members="M >= 1") == "samples (0, 2, 4, 5, 6) must be (M >= 1,) + truth (2, 4, 5, 6) = (L, F, H, W)"
    assert _raises(EH.check_ensemble, s.long(), t, floating=True) == "samples (torch.int64) and truth (torch.float32) must be floating point"
    assert _raises(EH.check_ensemble, s.half(), t.int(), floating=True) == "samples (torch.float16) and truth (torch.int32) must be floating point"
    assert EH.check_ensemble(s.long(), t) is None  # only where asked for
    assert _raises(EH.check_ensemble, s.long(), t[:1], floating=True).startswith("samples (3, 2, 4, 5, 6) must be")  # the shape first


def test_the_public_entry_points_still_say_it():
    """one call per form, through the module that owns it"""
    from climate2weather_amd import crps, marginals, multivariate, quantiles, spectra, ssim, wasserstein, windpower
    s, t = torch.zeros(3, 2, 4, 8, 8), torch.zeros(1, 4, 8, 8)
    plain_T = "samples (3, 2, 4, 8, 8) must be (M,) + truth (1, 4, 8, 8) = (T, F, H, W)"
    plain_L = "samples (3, 2, 4, 8, 8) must be (M,) + truth (1, 4, 8, 8) = (L, F, H, W)"
    one_T = "samples (3, 2, 4, 8, 8) must be (M >= 1,) + truth (1, 4, 8, 8) = (T, F, H, W)"
    one_L = "samples (3, 2, 4, 8, 8) must be (M >= 1,) + truth (1, 4, 8, 8) = (L, F, H, W)"
    curve = windpower.PowerCurve([3.0, 12.0, 25.0], [0.0, 3e6, 3e6])
    for fn in (crps.ensemble_terms, crps.crps_report, multivariate.pair_sqdist, multivariate.multivariate_report):
        assert _raises(fn, s, t) == plain_T
    assert _raises(multivariate.variogram_terms, s, t, radius=1) == plain_T
    for fn in (ssim.ssim_report, spectra.spectral_report, wasserstein.swd_report):
        assert _raises(fn, s, t) == plain_L
    assert _raises(windpower.wind_report, s, t, curve) == plain_L
    assert _raises(marginals.pit_counts, s, t) == one_T
    for fn in (marginals.marginals_report, quantiles.quantile_report):
        assert _raises(fn, s, t) == one_L
    t = torch.zeros(2, 4, 8, 8)
    for fn in (crps.crps_report, ssim.ssim_report, spectra.spectral_report, wasserstein.swd_report, marginals.marginals_report,
               multivariate.multivariate_report):
        assert _raises(fn, s, t, names=["a", "b"]) == "2 names for 4 variables"
    assert _raises(quantiles.quantile_report, s, t, names=["a"]) == "1 names for 4 variables"
    assert _raises(crps.ensemble_terms, s.long(), t) == "samples (torch.int64) and truth (torch.float32) must be floating point"
    assert _raises(multivariate.pair_sqdist, s, t.long()) == "samples (torch.float32) and truth (torch.int64) must be floating point"
    for fn, q in ((quantiles.quantile, (0.5,)), (marginals.gaussian_kde, torch.zeros(4, 3, dtype=torch.float64))):
        assert _raises(fn, s, q, truth=t[:1]) == "truth (1, 4, 8, 8) must be (2, 4, 8, 8) = (T, F, H, W) of the values"
    assert _raises(quantiles.quantile, s[0, 0], 0.5) == "values (4, 8, 8) must be (..., T, F, H, W)"


def test_variable_names():
    assert EH.variable_names(None, 3) == ["var0", "var1", "var2"] and EH.variable_names(None, 0) == []
    given = ("tas", "pr")
    got = EH.variable_names(given, 2)
    assert got == ["tas", "pr"] and isinstance(got, list)
    assert EH.variable_names(iter(given), 2) == ["tas", "pr"]
    assert _raises(EH.variable_names, given, 3) == "2 names for 3 variables"
    assert _raises(EH.variable_names, [], 1) == "0 names for 1 variables"
    assert _raises(EH.variable_names, ["a", "b", "c"], 2) == "3 names for 2 variables"


def test_datasets():
    v = torch.arange(2 * 3 * 2 * 4 * 5 * 6, dtype=torch.float64).reshape(2, 3, 2, 4, 5, 6)
    t = torch.arange(2 * 4 * 5 * 6, dtype=torch.float32).reshape(2, 4, 5, 6)
    x, y, lead = EH.datasets(v, t)
    assert lead == (2, 3) and tuple(x.shape) == (6, 2, 4, 30) and tuple(y.shape) == (2, 4, 30)
    assert _is_kernel_input(x) and torch.equal(x, v.float().reshape(6, 2, 4, 30)) and y.data_ptr() == t.data_ptr()
    x, y, lead = EH.datasets(t, None)
    assert lead == () and tuple(x.shape) == (1, 2, 4, 30) and y is None and x.data_ptr() == t.data_ptr()
    x, _, lead = EH.datasets(v[:, :0], None)
    assert lead == (2, 0) and tuple(x.shape) == (0, 2, 4, 30)
    assert _raises(EH.datasets, t[0], None) == "values (4, 5, 6) must be (..., T, F, H, W)"
    assert _raises(EH.datasets, v, t[:, :3]) == "truth (2, 3, 5, 6) must be (2, 4, 5, 6) = (T, F, H, W) of the values"
    assert _raises(EH.datasets, v, t[0]) == "truth (4, 5, 6) must be (2, 4, 5, 6) = (T, F, H, W) of the values"


# ------------------------------------------------------------------------------------------------------------------ the reports

def test_variable_report_and_the_members_table():
    rows = [torch.tensor([1.0, 2.0, 4.0], dtype=torch.float64), torch.tensor([0.5, 0.5, 0.5], dtype=torch.float64)]
    rep = EH.VariableReport(("a", "b"), [dict(score=r) for r in rows])
    assert rep.names == ["a", "b"] and rep["b"]["score"] is rows[1] and [n for n, _ in rep] == ["a", "b"]
    with pytest.raises(ValueError):
        rep["c"]
    out = EH.member_mean_std(rows, ["p/a/score", "p/b/score"])
    assert list(out) == ["p/a/score", "p/a/score_std", "p/b/score", "p/b/score_std"]
    want = np.array([1.0, 2.0, 4.0])
    assert out["p/a/score"] == float(want.mean()) and out["p/a/score_std"] == float(want.std()) and out["p/b/score_std"] == 0.0
    from climate2weather_amd import crps, marginals, multivariate, quantiles, spectra, ssim, wasserstein, windpower
    for cls in (crps.CrpsReport, ssim.SsimReport, spectra.SpectralReport, wasserstein.WassersteinReport, marginals.MarginalsReport,
                quantiles.QuantileReport, multivariate.MultivariateReport):
        assert issubclass(cls, EH.VariableReport) and cls.__doc__ and "as_dict" in vars(cls)
    assert not issubclass(windpower.WindReport, EH.VariableReport)


# ------------------------------------------------------------------------------------------------------------------ the seam

class RouteAsked(Exception):
    pass


def _asked(x):
    raise RouteAsked


def _entry_points():
    from climate2weather_amd import crps, marginals, multivariate, quantiles, spectra, ssim, wasserstein, windpower
    curve = windpower.PowerCurve([3.0, 12.0, 25.0], [0.0, 3e6, 3e6])
    return {"crps": lambda s, t: crps.ensemble_terms(s, t),
            "ssim": lambda s, t: ssim.ssim(s, t, win_size=3),
            "spectra": lambda s, t: spectra.rapsd(s),
            "wasserstein": lambda s, t: wasserstein.sliced_wasserstein(s, t, n_projections=4),
            "marginals": lambda s, t: marginals.pit_counts(s, t),
            "quantiles": lambda s, t: quantiles.quantile(s, (0.25, 0.5)),
            "windpower": lambda s, t: windpower.wind_fields(s, curve, u=0, v=1),
            "multivariate": lambda s, t: multivariate.pair_sqdist(s, t)}


@pytest.mark.parametrize("patched", METRICS)
def test_every_module_asks_its_own_predicate_and_no_other(monkeypatch, patched):
    """what every tests/emu_*_ops.py::install relies on: the name ``_on_device`` of one module routes that module alone"""
    g = torch.Generator().manual_seed(11)
    s, t = torch.randn(3, 2, 2, 8, 8, generator=g), torch.randn(2, 2, 8, 8, generator=g)
    entry = _entry_points()
    assert set(entry) == set(METRICS)
    before = {name: fn(s, t) for name, fn in entry.items()}  # CPU tensors: every module takes its general route
    monkeypatch.setattr(importlib.import_module(f"climate2weather_amd.{patched}"), "_on_device", _asked)
    with pytest.raises(RouteAsked):
        entry[patched](s, t)
    for name in METRICS:
        if name != patched:
            got = entry[name](s, t)
            same = [torch.equal(a, b) for a, b in zip(got, before[name])] if isinstance(got, tuple) else [torch.equal(got, before[name])]
            assert all(same), name


def test_import_hygiene():
    """nothing in the layer decides a route, and no metric module takes a helper from another metric module"""
    tree = ast.parse(open(os.path.join(PACKAGE, "ensemble_host.py")).read())
    calls = {n.func.id for n in ast.walk(tree) if isinstance(n, ast.Call) and isinstance(n.func, ast.Name)}
    assert "on_device" not in calls and "_on_device" not in calls
    for name in METRICS:
        mod = importlib.import_module(f"climate2weather_amd.{name}")
        assert mod._on_device is EH.on_device and "_on_device" in vars(mod)
        for node in ast.walk(ast.parse(open(os.path.join(PACKAGE, f"{name}.py")).read())):
            if isinstance(node, ast.ImportFrom):
                assert node.module not in METRICS, (name, node.module)
    from climate2weather_amd import ssim, wasserstein
    assert not hasattr(ssim, "_dense32") and not hasattr(wasserstein, "MOMENT_CHUNK_ELEMS")
