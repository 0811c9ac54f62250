"""The fixed-order sum the ensemble metrics share (csrc/ordered_sum.h), without a GPU: the header compiled for the host under the
address and undefined-behaviour sanitizers, its phases run one thread after the other by tests/host_ordered_sum_main.cpp, against
tests/emu_ordered_sum.py bit for bit -- the LDS layout, the order of the additions, the sum over the parts and the two write policies."""
import os
import subprocess

import numpy as np
import pytest

import emu_ordered_sum as E
import host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POLICIES = {"nan_if_nan": (0, E.nan_if_nan), "nan_if_not_finite": (1, E.nan_if_not_finite)}
CANONICAL_NAN, PLUS_INF = 0x7ff8000000000000, 0x7ff0000000000000
ODD_NAN_BITS = 0xfff4000000c0ffee
ODD_NAN = np.array([ODD_NAN_BITS], np.uint64).view(np.float64)[0]  # the sign bit set, a payload, the quiet bit clear


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """a stand-alone program under the address and undefined-behaviour sanitizers; it is run directly, never loaded into Python"""
    return host_program.build(tmp_path_factory, "ordered_sum", sanitize=True, fp_contract_off=True, timeout=600)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _workgroup(host, tmp_path, acc, policy):
    """acc (N, 256) through the host build -> (N,); asserted equal to the emulation bit for bit"""
    code, fn = POLICIES[policy]
    N = acc.shape[0]
    np.ascontiguousarray(acc, np.float64).tofile(tmp_path / "acc")
    subprocess.run([str(host), "workgroup", str(N), str(code), str(tmp_path / "acc"), str(tmp_path / "out")], check=True, timeout=60)
    got = np.fromfile(tmp_path / "out", dtype=np.float64)
    assert got.shape == (N,)
    assert np.array_equal(_bits(got), _bits(E.fold_workgroup(acc, fn))), (N, policy)
    return got


def _parts(host, tmp_path, part, policy):
    """part (outer, parts, inner) through the host build -> (outer, inner); asserted equal to the emulation bit for bit"""
    code, fn = POLICIES[policy]
    outer, parts, inner = part.shape
    np.ascontiguousarray(part, np.float64).tofile(tmp_path / "part")
    subprocess.run([str(host), "parts", str(outer), str(parts), str(inner), str(code), str(tmp_path / "part"), str(tmp_path / "out")], check=True, timeout=60)
    got = np.fromfile(tmp_path / "out", dtype=np.float64).reshape(outer, inner)
    assert np.array_equal(_bits(got), _bits(E.fold_parts(part, 1, fn))), (part.shape, policy)
    return got


def _wide(rng, shape):
    """doubles of both signs spanning 30 orders of magnitude: the order of the additions shows in the last bits"""
    return rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-15, 15, shape)


def test_the_emulation_adds_in_index_order_from_plus_zero():
    """what the header is held to, stated once without it: a hand-written loop, and a case where the order of additions matters"""
    a = np.array([1e16, 1.0, -1e16, 1.0])
    assert E.seq_sum(a, 0) == 1.0 and E.seq_sum(a[::-1], 0) == 0.0  # ((1e16 + 1) - 1e16) + 1 against ((1 - 1e16) + 1) + 1e16
    acc = _wide(np.random.default_rng(5), (3, 256))
    want = np.zeros(3)
    for s in range(3):
        totals = []
        for g in range(16):
            t = 0.0
            for j in range(16):
                t += acc[s, g * 16 + j]
            totals.append(t)
        for t in totals:
            want[s] += t
    assert np.array_equal(_bits(E.fold_workgroup(acc, E.nan_if_nan)), _bits(want))
    assert E.THREADS == 256 and E.GROUP == 16 and E.GROUPS == 16
    core = open(os.path.join(ROOT, "climate2weather_amd", "csrc", "ordered_sum.h")).read()
    for text in ("THREADS = 256", "GROUP = 16", "GROUPS = THREADS / GROUP", "N * (THREADS + GROUPS)"):
        assert text in core, text


@pytest.mark.parametrize("N", [1, 2, 4, 12])
@pytest.mark.parametrize("policy", sorted(POLICIES))
def test_workgroup_fold_equals_the_emulation_bit_for_bit(host, tmp_path, N, policy):
    rng = np.random.default_rng(100 + N)
    got = _workgroup(host, tmp_path, _wide(rng, (N, 256)), policy)
    assert np.all(np.isfinite(got)) and np.all(got != 0.0)
    assert np.array_equal(_bits(_workgroup(host, tmp_path, np.zeros((N, 256)), policy)), np.zeros(N, np.uint64))
    # accumulators of -0.0 only: the sum starts from +0.0, and +0.0 + -0.0 is +0.0
    assert np.array_equal(_bits(_workgroup(host, tmp_path, np.full((N, 256), -0.0), policy)), np.zeros(N, np.uint64))


@pytest.mark.parametrize("N", [1, 2, 4, 12])
def test_write_policies_of_the_workgroup_fold(host, tmp_path, N):
    """an infinite or NaN accumulator reaches exactly its own sum, as the policy says; the other sums keep their bits"""
    rng = np.random.default_rng(200 + N)
    base = _wide(rng, (N, 256))
    clean = {p: _workgroup(host, tmp_path, base, p) for p in POLICIES}
    s, tid = N - 1, 77
    for values, want in (((np.inf,), {"nan_if_nan": PLUS_INF, "nan_if_not_finite": CANONICAL_NAN}),
                         ((np.inf, -np.inf), {"nan_if_nan": CANONICAL_NAN, "nan_if_not_finite": CANONICAL_NAN}),
                         ((ODD_NAN,), {"nan_if_nan": CANONICAL_NAN, "nan_if_not_finite": CANONICAL_NAN})):
        acc = base.copy()
        for k, v in enumerate(values):
            acc[s, tid + 100 * k] = v  # two infinities in different groups: they meet in the sum of the group totals
        assert values[0] is not ODD_NAN or int(_bits(acc)[s, tid]) == ODD_NAN_BITS  # the payload survived the copy
        for policy in POLICIES:
            got = _bits(_workgroup(host, tmp_path, acc, policy))
            assert int(got[s]) == int(want[policy]), (values, policy, hex(int(got[s])))
            assert np.array_equal(np.delete(got, s), np.delete(_bits(clean[policy]), s))


@pytest.mark.parametrize("parts", [1, 2, 5])
@pytest.mark.parametrize("inner", [1, 3, 12])
def test_fold_parts_equals_the_emulation_bit_for_bit(host, tmp_path, parts, inner):
    """partial [outer][parts][inner]: every entry adds its own parts, in index order from +0.0, under both policies"""
    rng = np.random.default_rng(1000 * parts + inner)
    outer = 3
    part = _wide(rng, (outer, parts, inner))
    for policy in POLICIES:
        got = _parts(host, tmp_path, part, policy)
        assert np.all(np.isfinite(got))
        assert np.array_equal(_bits(_parts(host, tmp_path, np.full((outer, parts, inner), -0.0), policy)), np.zeros((outer, inner), np.uint64))
    o, i = outer - 1, inner - 1
    for values, want in (((np.inf,), {"nan_if_nan": PLUS_INF, "nan_if_not_finite": CANONICAL_NAN}),
                         ((np.inf, -np.inf), {"nan_if_nan": CANONICAL_NAN, "nan_if_not_finite": CANONICAL_NAN}),
                         ((ODD_NAN,), {"nan_if_nan": CANONICAL_NAN, "nan_if_not_finite": CANONICAL_NAN})):
        if len(values) > parts:
            continue  # two infinities need two parts
        bad = part.copy()
        for k, v in enumerate(values):
            bad[o, parts - 1 - k, i] = v
        for policy, (_, fn) in POLICIES.items():
            got = _bits(_parts(host, tmp_path, bad, policy))
            assert int(got[o, i]) == int(want[policy]), (values, policy, hex(int(got[o, i])))
            clean = _bits(E.fold_parts(part, 1, fn))
            keep = np.ones((outer, inner), bool)
            keep[o, i] = False
            assert np.array_equal(got[keep], clean[keep])
