"""d-sharded centered clipping through gm_cclip_f32's real host loop, on ONE GPU: P virtual
ranks in P threads, each with its own context holding a column shard, their all-reduce
callback summing the (K+2)-vectors across threads (the scheme of test_gpu_sharded.py).
Every rank must derive the same coefficients, a and stop decision from the reduced sums; the
concatenated shards must meet the bar against the fp64 reference and the unsharded call."""
import ctypes as C
import threading

import pytest
import torch

import cclip_cases as cc

pytestmark = pytest.mark.gpu


def _sharded(X, g0, P, tau, iters, panels):
    from byzantine_aircomp_amd import ClientPanels, _lib
    from byzantine_aircomp_amd.aggregators import Context
    from byzantine_aircomp_amd.sharded import _wrap, shard_range

    K, d = X.shape
    dev = X.device
    barrier = threading.Barrier(P, timeout=60)   # a rank-dependent collective count fails here
    bufs = [None] * P
    out = [None] * P
    errs = []

    def run(r):
        try:
            lo, hi = shard_range(d, P, r)
            ctx = Context(dev.index)
            ctx.set_shard(d, lo)

            def allreduce(ptr, count, stream):
                torch.cuda.synchronize(dev)
                t = _wrap(ptr, count, dev)
                bufs[r] = t.clone()
                barrier.wait()
                total = torch.stack(bufs).sum(0)
                barrier.wait()
                t.copy_(total)
                torch.cuda.synchronize(dev)
            ctx.set_allreduce(allreduce)
            Xs = X[:, lo:hi].contiguous()
            ptr, ldx = Xs.data_ptr(), hi - lo
            if panels:
                Xs = ClientPanels.from_rows(Xs)
                ptr, ldx = Xs.data.data_ptr(), Xs.panel_stride
            g = g0[lo:hi].contiguous()
            res = torch.empty(hi - lo, device=dev)
            o = _lib.GmCclipOpts()
            o.tau, o.maxiter, o.tol = tau, iters, -1.0
            o.layout = _lib.GM_LAYOUT_PANELS if panels else _lib.GM_LAYOUT_ROWS
            rr = _lib.GmCclipResult()
            _lib.check(ctx.lib.gm_cclip_f32(ctx.handle, ptr, K, hi - lo, ldx, g.data_ptr(),
                                            res.data_ptr(), C.byref(o), C.byref(rr), None),
                       "sharded cclip")
            torch.cuda.synchronize(dev)
            out[r] = (lo, hi, res, rr.iters, rr.clipped, rr.last_movement)
            ctx.close()
        except Exception as e:  # noqa: BLE001
            errs.append(e)
            barrier.abort()

    th = [threading.Thread(target=run, args=(r,)) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not errs, errs
    full = torch.empty(d, device=dev)
    for lo, hi, res, *_ in out:
        full[lo:hi] = res
    return full, {o_[3] for o_ in out}, {o_[4] for o_ in out}, {o_[5] for o_ in out}


@pytest.mark.parametrize("iters", cc.ITERS)
@pytest.mark.parametrize("panels", [False, True])
@pytest.mark.parametrize("K,d,P", [(17, 2051, 3), (600, 8200, 2)])
def test_sharded_cclip_matches_reference_and_unsharded(K, d, P, panels, iters):
    import byzantine_aircomp_amd as bz
    X, g0 = cc.inputs(K, d)
    tau = cc.tau_of("mid", d)
    vs, clipped, _, margins = cc.reference(X.numpy(), g0.numpy(), tau, iters)
    assert min(margins) >= 0.5, margins
    Xg, g = X.cuda(), g0.cuda()
    whole = bz.cclip(bz.ClientPanels.from_rows(Xg) if panels else Xg,
                     {"tau": tau, "clip_iters": iters, "guess": g})
    whole_clipped = bz.cclip.last_info["clipped"]
    got, it, cl, mv = _sharded(Xg, g, P, tau, iters, panels)
    rel_ref = cc.rel_l2(got.cpu().numpy(), vs[-1])
    rel_whole = cc.rel_l2(got.cpu().numpy(), whole.cpu().numpy())
    print(f"sharded cclip {K}x{d} P={P} panels={panels} iters={iters}: rel_l2 vs reference "
          f"{rel_ref:.3e}, vs unsharded {rel_whole:.3e}, clipped {cl}")
    assert it == {iters}                      # every rank ran the same count ...
    assert cl == {clipped[-1]} == {whole_clipped}   # ... from the same coefficients
    assert len(mv) == 1                       # ... and saw the same movement
    assert rel_ref <= cc.TOL
    assert rel_whole <= cc.TOL


def test_sharded_gm_cclip_world1():
    """ShardedGM.cclip through torch.distributed (one rank, the torch all-reduce callback)."""
    import socket

    import torch.distributed as dist

    import byzantine_aircomp_amd as bz
    from byzantine_aircomp_amd.sharded import ShardedGM
    K, d = 600, 8200
    X, g0 = cc.inputs(K, d)
    tau = cc.tau_of("mid", d)
    vs, clipped, _, _ = cc.ref_case(K, d, "fp32", "mid")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        sg = ShardedGM(d, transport="torch")
        try:
            with pytest.raises(ValueError, match="guess"):
                sg.cclip(X.cuda(), {"tau": tau})
            for W in (X.cuda(), bz.ClientPanels.from_rows(X.cuda())):
                got = sg.cclip(W, {"tau": tau, "clip_iters": 3, "guess": g0.cuda()})
                torch.cuda.synchronize()
                assert sg.last_result.iters == 3 and sg.last_clipped == clipped[2]
                assert cc.rel_l2(got.cpu().numpy(), vs[2]) <= cc.TOL
        finally:
            sg.close()
    finally:
        dist.destroy_process_group()
