"""The omniscient attacks' host side (byzantine_aircomp_amd.attacks, the C ABI's refusals) and
the numpy reference of tests/attack_cases.py.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import attack_cases as ac
from conftest import ROOT
from bucket_cases import normal_matrix

NEW_SYMBOLS = ("gm_attack_affine_f32", "gm_attack_affine_bf16", "gm_attack_minmax_f32")
NAMES = ("alie", "ipm", "minmax", "minsum")


@pytest.mark.parametrize("K,B,want", [(50, 10, 0.2533), (17, 4, 0.2934), (1024, 1, -0.0012)])
def test_z_max(K, B, want):
    import byzantine_aircomp_amd as bz
    assert bz.z_max(K, B) == ac.ref_z_max(K, B)
    assert abs(bz.z_max(K, B) - want) < 5e-5


def test_z_max_refuses_a_byzantine_majority_of_the_median():
    import byzantine_aircomp_amd as bz
    for K, B in [(50, 26), (50, 40), (17, 9), (7, 4)]:
        with pytest.raises(ValueError):
            bz.z_max(K, B)
    assert bz.z_max(50, 25) == ac.ref_z_max(50, 25)          # s = 1: the last B allowed


def test_alie_checks_z_before_any_gpu_work():
    import byzantine_aircomp_amd as bz
    X = torch.zeros(10, 8)
    with pytest.raises(ValueError):
        bz.alie(X, 6)                                        # 6 >= floor(10/2 + 1)
    for B in (0, -1, 9, 10, 2.0, True):
        with pytest.raises(ValueError):
            bz.alie.with_options(z=1.0)(X, B)                # no honest pair, or no integer
    with pytest.raises(ValueError):
        bz.ipm(torch.zeros(10), 2)
    assert not X.any()


def test_dtype_refusals():
    import byzantine_aircomp_amd as bz
    for attack in (bz.alie, bz.ipm, bz.minmax, bz.minsum):
        with pytest.raises(TypeError):
            attack(torch.zeros(10, 8, dtype=torch.float64), 2)
        with pytest.raises(TypeError):
            attack(torch.zeros(10, 8, dtype=torch.float16), 2)
    for attack in (bz.minmax, bz.minsum, bz.minmax.with_options(dev="sign")):
        with pytest.raises(TypeError):
            attack(torch.zeros(10, 8, dtype=torch.bfloat16), 2)
    with pytest.raises(ValueError):
        bz.minmax.with_options(dev="l2")
    with pytest.raises(TypeError):
        bz.minmax.with_options(z=1.0)
    with pytest.raises(TypeError):
        bz.alie.with_options(epsilon=1.0)
    with pytest.raises(TypeError):
        bz.ipm.with_options(z=1.0)


def test_with_options_keep_the_names():
    import byzantine_aircomp_amd as bz
    assert bz.alie.with_options(z=1.5).__name__ == "alie"
    assert bz.ipm.with_options(epsilon=0.5).__name__ == "ipm"
    assert bz.minmax.with_options(dev="unit").__name__ == "minmax"
    assert bz.minsum.with_options(dev="sign").__name__ == "minsum"
    for name in NAMES:
        assert getattr(bz, name).__name__ == name


def test_exported_and_mapped_by_name():
    import byzantine_aircomp_amd as bz
    from byzantine_aircomp_amd import attacks, training
    for name in NAMES + ("z_max",):
        assert name in attacks.__all__ and getattr(bz, name) is getattr(attacks, name)
    for name in NAMES:
        assert name in training.ATTACK_NAMES
        assert training.attack_by_name(name) is getattr(attacks, name)
    assert training.attack_by_name("weightflip") is training.weightflip
    with pytest.raises(KeyError):
        training.attack_by_name("nope")


def test_symbols_declared_bound_and_exported():
    from byzantine_aircomp_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gmagg.h")).read(),
                  flags=re.S)
    bound = {n for n, _, _ in _lib.SIGNATURES}
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                          text=True, check=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\bint\s+{name}\s*\(", text), name
        assert name in bound and name in exported and hasattr(lib, name), name
    assert lib.gm_abi_version() == 5


def test_null_arguments_are_refused_with_a_message():
    from byzantine_aircomp_amd import _lib
    lib = _lib.load()
    for rc in (lib.gm_attack_affine_f32(None, None, 10, 8, 8, 0, 2, 1.0, -1.0, None),
               lib.gm_attack_affine_bf16(None, None, 10, 8, 8, 0, 2, 1.0, -1.0, None),
               lib.gm_attack_minmax_f32(None, None, 10, 8, 8, 0, 2, 0, 0, None, None)):
        assert rc == -1
        assert b"NULL" in lib.gm_last_error()


@pytest.mark.parametrize("K,B,d", [(7, 2, 37), (50, 10, 70)])
def test_closed_form_gamma_equals_the_bisection(K, B, d):
    geo = ac.honest_geometry(K, B, d)
    for rule in ("max", "sum"):
        assert ac.amplification(geo, rule) <= 2.0
        for dev in ac.DEVS:
            g, p = ac.ref_gamma(geo, rule, dev)
            assert g > 0
            assert abs(g - ac.bisect_gamma(geo, rule, dev)) <= 1e-12 * g, (rule, dev)
            # the constraint is tight at gamma
            lhs = ac.constraint_value(geo, rule, geo["mu"] - g * p)
            assert abs(lhs - ac.bound_of(geo, rule)) <= 1e-12 * lhs


def _emulate_kernel(X, B, a, b):
    """attack.hip's arithmetic in numpy fp64: the plain sum for mu, sums shifted by the first
    row for sigma, the variance clamped at 0."""
    H = X.shape[0] - B
    x0 = X[0].astype(np.float64)
    s = np.zeros_like(x0)
    u = np.zeros_like(x0)
    v = np.zeros_like(x0)
    for k in range(H):
        xd = X[k].astype(np.float64)
        t = xd - x0
        s = s + xd
        u = u + t
        v = v + t * t
    var = (v - u * (u / H)) / (H - 1.0)
    y = a * (s / H)
    if b != 0:
        y = y + b * np.sqrt(np.where(var < 0, 0.0, var))
    return y


@pytest.mark.parametrize("K,B,d", [c for c in ac.CASES if c[0] * c[2] <= 1 << 21])
def test_shifted_sums_stay_inside_the_fp32_bound(K, B, d):
    X = normal_matrix(K, d)
    for a, b in ((1.0, -ac.ref_z_max(K, B)), (-0.1, 0.0), (1.0, -1.5)):
        ref, slack = ac.ref_affine(X, B, a, b)
        got = _emulate_kernel(X, B, a, b).astype(np.float32)
        assert ac.mismatch_f32(got, ref, slack) == 0


def test_shifted_sums_are_exact_on_constant_columns():
    X = np.empty((20, 4), dtype=np.float32)
    X[:] = np.array([3.0, 1e6 + 7, -0.1, 0.0], dtype=np.float32)
    X[15:] = 99.0
    assert np.array_equal(_emulate_kernel(X, 5, 1.0, -2.0), X[0].astype(np.float64))
    ref, _ = ac.ref_affine(X, 5, 1.0, -2.0)
    assert np.array_equal(ref.astype(np.float32), X[0])
