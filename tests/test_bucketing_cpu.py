"""s-bucketing without a GPU: the assignment, the bucket counts, what is refused before
anything touches a device, the wrapper's name and honestSize rule, the C ABI's argument
checks.  (The kernel itself: tests/test_gpu_bucketing.py.)
"""
import numpy as np
import pytest
import torch

import bucket_cases as bc
import byzantine_aircomp_amd as bz
from byzantine_aircomp_amd import _lib, aggregators as agg


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to reach a GPU context (or to stage a tensor) fails the test."""
    def boom(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(agg, "context", boom)
    monkeypatch.setattr(agg, "_stage", boom)


def test_exported():
    assert bz.bucketing is agg.bucketing and bz.bucketed is agg.bucketed
    assert {"bucketing", "bucketed"} <= set(agg.__all__)


def test_assignment_is_a_seeded_permutation():
    for K, s in [(1, 1), (7, 2), (50, 3), (1000, 4)]:
        p = bz.bucketing.assignment(K, s, torch.Generator().manual_seed(11))
        assert p.dtype == torch.int64 and sorted(p.tolist()) == list(range(K))
        q = bz.bucketing.assignment(K, s, torch.Generator().manual_seed(11))
        assert torch.equal(p, q)
        assert torch.equal(p, torch.randperm(K, generator=torch.Generator().manual_seed(11)))
    torch.manual_seed(5)
    a = bz.bucketing.assignment(100, 2)              # the global CPU generator, one draw
    torch.manual_seed(5)
    assert torch.equal(a, torch.randperm(100))


@pytest.mark.parametrize("K,s,counts", [(7, 2, [2, 2, 2, 1]), (50, 3, [3] * 16 + [2]),
                                        (17, 40, [17]), (17, 17, [17]), (6, 3, [3, 3]),
                                        (5, 1, [1] * 5)])
def test_bucket_counts_of_the_reference(K, s, counts):
    """The numpy reference's buckets: sizes for s not dividing K, s > K, s == K, and the mean
    of exactly those rows."""
    assert bc.n_buckets(K, s) == len(counts)
    X = np.arange(K, dtype=np.float32)[:, None] * np.ones((1, 3), dtype=np.float32)
    perm = bc.seeded_perm(K, s).numpy()
    Y = bc.ref_bucket_means(X, perm, s)
    assert Y.shape == (len(counts), 3)
    at = 0
    for i, c in enumerate(counts):
        assert Y[i, 0] == np.float32(perm[at:at + c].astype(np.float64).sum() / c)
        at += c
    assert at == K


def test_s_1_returns_the_object_and_draws_nothing(no_device):
    X = torch.randn(6, 5)
    torch.manual_seed(123)
    state = torch.get_rng_state()
    before = bz.bucketing.last_perm
    assert bz.bucketing(X, 1) is X
    assert bz.bucketing(X, 1, layout="panels") is X
    assert torch.equal(torch.get_rng_state(), state)
    assert bz.bucketing.last_perm is before
    calls = []
    inner = lambda w, o={}: calls.append((w, o)) or "r"            # noqa: E731
    inner.__name__ = "inner"
    opts = {"honestSize": 4}
    assert bz.bucketed(inner, 1)(X, opts) == "r"
    assert calls[0][0] is X and calls[0][1] is opts
    assert torch.equal(torch.get_rng_state(), state)


@pytest.mark.parametrize("s", [0, -2, 2.0, 1.5, "2", None, True])
def test_bad_s_is_a_value_error(no_device, s):
    X = torch.randn(6, 5)
    with pytest.raises(ValueError):
        bz.bucketing(X, s)
    with pytest.raises(ValueError):
        bz.bucketed(bz.gm2, s)
    with pytest.raises(ValueError):
        bz.bucketing.assignment(6, s)


def test_numpy_integer_s_is_accepted(no_device):
    assert bz.bucketed(bz.gm2, np.int64(3)).__name__ == "gm2_b3"


@pytest.mark.parametrize("perm", [[0, 1, 2, 3, 4, 4], [0, 1, 2, 3, 4], [0, 1, 2, 3, 4, 5, 6],
                                  [0, 1, 2, 3, 4, 6], [-1, 0, 1, 2, 3, 4],
                                  [0.0, 1.0, 2.0, 3.0, 4.0, 5.0], [[0, 1, 2], [3, 4, 5]]])
def test_bad_perm_is_a_value_error_before_any_device(no_device, perm):
    X = torch.randn(6, 5)
    with pytest.raises(ValueError):
        bz.bucketing(X, 2, perm=torch.tensor(perm))


def test_bad_inputs(no_device):
    with pytest.raises(TypeError):
        bz.bucketing(torch.zeros(6, 5, dtype=torch.float64), 2)
    with pytest.raises(ValueError):
        bz.bucketing(torch.zeros(6), 2)
    with pytest.raises(ValueError):
        bz.bucketing(torch.zeros(6, 5), 2, layout="columns")
    with pytest.raises(ValueError):
        bz.bucketed(bz.gm2, 2, layout="columns")


def test_wrapper_name():
    assert bz.bucketed(bz.gm2, 2).__name__ == "gm2_b2"
    assert bz.bucketed(bz.Krum, 3).__name__ == "Krum_b3"
    assert bz.bucketed(bz.cclip.with_options(tau=1.0), 4).__name__ == "cclip_b4"
    assert bz.bucketed(bz.median, 1).__name__ == "median_b1"


def test_honest_size_rule(no_device, monkeypatch):
    """honestSize' = ceil(K/s) - (K - honestSize); < 2 is refused before a device is touched;
    the caller's dict is never modified."""
    seen = []

    def fake_bucketing(w, s, perm=None, generator=None, layout=None):
        seen.append((s, layout))
        return "means"
    monkeypatch.setattr(agg, "bucketing", fake_bucketing)
    calls = []
    inner = lambda w, o={}: calls.append((w, o)) or torch.zeros(3)       # noqa: E731
    inner.__name__ = "inner"
    X = torch.zeros(1000, 3)
    opts = {"honestSize": 800, "maxiter": 7}
    keep = dict(opts)
    bz.bucketed(inner, 2)(X, opts)
    assert opts == keep
    assert calls[-1] == ("means", {"honestSize": 300, "maxiter": 7}) and calls[-1][1] is not opts
    assert seen[-1] == (2, "panels")
    bz.bucketed(inner, 3, layout="rows")(X, opts)                  # Kb = 334, B = 200
    assert calls[-1][1]["honestSize"] == 134 and seen[-1] == (3, "rows")
    no_hs = {"maxiter": 7}
    bz.bucketed(inner, 2)(X, no_hs)                                # no honestSize: untouched
    assert calls[-1][1] is no_hs
    n = len(calls)
    with pytest.raises(ValueError, match="honestSize"):
        bz.bucketed(inner, 5)(X, {"honestSize": 801})              # 200 - 199 = 1
    with pytest.raises(ValueError, match="honestSize"):
        bz.bucketed(inner, 2)(X, {"honestSize": 400})              # 500 - 600 < 0
    assert len(calls) == n and opts == keep
    bz.bucketed(inner, 5)(X, {"honestSize": 802})                  # 200 - 198 = 2: accepted
    assert calls[-1][1]["honestSize"] == 2


def test_abi_bucket_means_argument_checks():
    """No device needed: every refusal happens before the first HIP call."""
    import ctypes as C
    lib = _lib.load()
    assert lib.gm_abi_version() == _lib.ABI_VERSION
    names = {n for n, _, _ in _lib.SIGNATURES}
    assert {"gm_bucket_means_f32", "gm_bucket_means_bf16"} <= names
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    for fn in (lib.gm_bucket_means_f32, lib.gm_bucket_means_bf16):
        assert fn(None, p, 4, 4, 4, 0, None, 2, p, 4, 0, None) == -1       # NULL ctx
        msg = lib.gm_last_error()
        assert msg and b"gm_bucket_means" in msg
        assert fn(None, None, 4, 4, 4, 0, None, 2, None, 4, 0, None) == -1
