"""bf16 client updates, the parts that need no GPU: the ABI additions of gm_weiszfeld_bf16
and ClientPanels(dtype=torch.bfloat16) on the CPU device."""
import pytest
import torch

from byzantine_aircomp_amd import ClientPanels, _lib


def test_panel_width_bf16_table():
    """gm_panel_width_bf16 is the bf16 streaming tile's chunk width: the fp32 tile with 8
    columns per lane instead of 4, so twice gm_panel_width wherever both exist."""
    lib = _lib.load()
    assert lib.gm_panel_width_bf16(0) == 0
    assert lib.gm_panel_width_bf16(4096) == 0
    assert lib.gm_panel_width_bf16(1000) == 64
    for K in (1, 16, 17, 100, 256, 257, 600, 1024, 2048):
        W = lib.gm_panel_width_bf16(K)
        assert W > 0 and W % 8 == 0, (K, W)          # 16-byte lane groups
        assert W == 2 * lib.gm_panel_width(K), (K, W)


def test_abi_version_is_5():
    assert _lib.load().gm_abi_version() == 5 == _lib.ABI_VERSION


def test_bf16_errors_are_reported_not_raised():
    lib = _lib.load()
    rc = lib.gm_weiszfeld_bf16(None, None, 0, 0, 0, None, None, None, None, None)
    assert rc == -1
    msg = lib.gm_last_error()
    assert b"gm_weiszfeld_bf16" in msg and b"NULL" in msg
    for fn in (lib.gm_rows_to_panels_bf16, lib.gm_rows_to_panels_bf16_from_f32):
        assert fn(None, None, 1, 1, 1, None, 8, 8, None) == -1
        assert b"bad args" in lib.gm_last_error()


def test_client_panels_bf16_roundtrip_cpu():
    g = torch.Generator().manual_seed(5)
    K, d = 37, 1000                                   # W = 256: three full panels + 232 columns
    X = torch.randn(K, d, generator=g)
    Xb = X.to(torch.bfloat16)
    P = ClientPanels(K, d, device="cpu", dtype=torch.bfloat16)
    assert P.dtype == torch.bfloat16 and P.W == _lib.load().gm_panel_width_bf16(K)
    assert P.data.shape == (-(-d // P.W), K, P.W)
    for k in range(K):
        P.store(k, Xb[k])
    assert torch.equal(P.to_rows(), Xb)
    assert all(torch.equal(P.row(k), Xb[k]) for k in (0, 17, K - 1))
    assert torch.count_nonzero(P.data[-1, :, d - (P.npan - 1) * P.W:]) == 0   # padding stays 0
    # fp32 rows into bf16 panels round as .to(bfloat16) does; bf16 rows copy exactly
    assert torch.equal(ClientPanels.from_rows(X, device="cpu", dtype=torch.bfloat16).to_rows(), Xb)
    Q = ClientPanels.from_rows(Xb, device="cpu")
    assert Q.dtype == torch.bfloat16 and torch.equal(Q.to_rows(), Xb)
    # the existing default: fp32 rows make fp32 panels
    assert ClientPanels.from_rows(X, device="cpu").dtype == torch.float32
    m = P.mean(0)
    assert m.dtype == torch.float32 and m.shape == (d,)
    want = Xb.double().mean(0)
    # an fp32 sum of K values: K * 2^-24 relative to the column's largest partial sum
    assert (m.double() - want).abs().max() <= K * 2.0 ** -24 * Xb.double().abs().sum(0).max()


def test_client_panels_rejects_other_dtypes():
    with pytest.raises(TypeError):
        ClientPanels(4, 16, device="cpu", dtype=torch.float16)
