"""The one GmOpts builder of the bindings (aggregators._gm_opts), no GPU needed: when it
draws a Philox key from the torch CPU generator.  The host-noise path replays the
reference's torch.normal sequence on that generator, so a draw too many shifts every result
that follows; a draw too few makes two unseeded calls share a key."""
import torch

from byzantine_aircomp_amd import _lib
from byzantine_aircomp_amd.aggregators import _gm_opts

GM = {"maxiter": 5, "tol": 1e-5, "noise_var": 1e-2, "P_max": 1}


def _state_after(fn):
    torch.manual_seed(77)
    fn()
    return torch.random.get_rng_state()


def test_gm_opts_draws_a_key_only_when_philox_needs_one():
    untouched = _state_after(lambda: None)
    one_draw = _state_after(lambda: torch.randint(0, 2 ** 62, (1,)))
    assert not torch.equal(untouched, one_draw)

    made = []
    build = lambda *a, **k: made.append(_gm_opts(*a, **k))                    # noqa: E731
    # the caller's draws: nothing is drawn, the callback is set
    st = _state_after(lambda: build(dict(GM, noise_source="host"), True, _lib.GM_LAYOUT_ROWS,
                                    shape=(8, 100)))
    assert torch.equal(st, untouched)
    assert made[-1].noise_source == _lib.GM_NOISE_HOST and made[-1].noise_cb
    # Philox without a seed: exactly one randint, and its value is the key
    st = _state_after(lambda: build(dict(GM, noise_source="device"), True, _lib.GM_LAYOUT_ROWS))
    assert torch.equal(st, one_draw)
    torch.manual_seed(77)
    assert made[-1].seed == int(torch.randint(0, 2 ** 62, (1,)).item())
    assert made[-1].noise_source == _lib.GM_NOISE_PHILOX
    # a seed given: nothing is drawn
    st = _state_after(lambda: build(dict(GM, noise_source="device", seed=5), True,
                                    _lib.GM_LAYOUT_ROWS))
    assert torch.equal(st, untouched) and made[-1].seed == 5
    # gm2: no key at all; a fused pre-noise without pre_oma_seed draws its one key
    st = _state_after(lambda: build({"maxiter": 5, "tol": 1e-5}, False, _lib.GM_LAYOUT_PANELS))
    assert torch.equal(st, untouched) and made[-1].pre_oma == 0
    st = _state_after(lambda: build({"maxiter": 5, "tol": 1e-5}, False, _lib.GM_LAYOUT_ROWS,
                                    pre_var=1e-2, pre_seed=9))
    assert torch.equal(st, untouched) and made[-1].pre_oma_seed == 9
    st = _state_after(lambda: build({"maxiter": 5, "tol": 1e-5}, False, _lib.GM_LAYOUT_ROWS,
                                    pre_var=1e-2))
    assert torch.equal(st, one_draw) and made[-1].pre_oma == 1
