"""Nearest-neighbor mixing step by step, against the torch formulation, same process, same box.

    python tools/nnm_bench.py [--out profiles/nnm.jsonl] [--rounds 20] [--d 2000000]

K = 1000 clients, f = 200, d columns, the C3 recipe (gm_fill_clients_f32), on fp32 rows and on
fp32 panels (output in the input's layout).  After one warm-up round, `--rounds` interleaved
rounds of gm_nnm_f32 stopped after the distances (GMAGG_NNM_STOP=1), after the neighbours (=2)
and run whole, each timed by device events around the call, after one untimed call stopped after
the distances (so that all three start from the same state of the caches); a round's step times
are the differences (distances, neighbours - distances, whole - neighbours).  In the same rounds the
formulation a user would write in torch, on the fp32 rows:
    D = torch.cdist(X, X); idx = D.topk(K - f, largest=False).indices
    W = zeros(K, K).scatter_(1, idx, 1); Y = (W @ X) / (K - f)
whose fp32 GEMM does not meet the accuracy contract: context only.  One JSON line per (case,
round); one summary line per case with the medians and mixing / distances, the yardstick (both
are O(K^2 d) over the same tiles).  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K, F = 1000, 200
M = K - F


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--d", type=int, default=2_000_000)
    a = ap.parse_args()
    d = a.d
    import byzantine_aircomp_amd as bz
    from byzantine_aircomp_amd import _lib
    ctx = bz.context()
    stream = torch.cuda.current_stream().cuda_stream
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    X = torch.empty(K, d, device="cuda")
    ctx.call("gm_fill_clients_f32", X.data_ptr(), K, d, d, F, 0.0, 0.05, 0.25, 0.5, 20211, stream)
    P = bz.ClientPanels.from_rows(X)
    Yr = torch.empty(K, d, device="cuda")
    Yp = bz.ClientPanels(K, d, device="cuda")
    ops = {"fp32_rows": (X.data_ptr(), d, _lib.GM_LAYOUT_ROWS, Yr.data_ptr(), d),
           "fp32_panels": (P.data.data_ptr(), P.panel_stride, _lib.GM_LAYOUT_PANELS,
                           Yp.data.data_ptr(), Yp.panel_stride)}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3, out             # us

    def nnm_call(name, stop):
        x, ldx, lay, y, ldy = ops[name]
        os.environ["GMAGG_NNM_STOP"] = str(stop)
        try:
            ctx.call("gm_nnm_f32", x, K, d, ldx, lay, F, y, ldy, lay, None, stream)
        finally:
            os.environ.pop("GMAGG_NNM_STOP", None)

    def torch_nnm():
        D = torch.cdist(X, X)
        idx = D.topk(M, dim=1, largest=False).indices
        W = torch.zeros(K, K, device="cuda").scatter_(1, idx, 1.0)
        return (W @ X) / M

    steps = {n: {"distances": [], "neighbors": [], "mixing": [], "whole": []} for n in ops}
    torch_us = []
    Yt = None
    for rnd in range(-1, a.rounds):                 # round -1: warm-up, not reported
        for name in ops:
            nnm_call(name, 1)                       # untimed: the three timed calls start alike
            t1, _ = timed(lambda: nnm_call(name, 1))
            t2, _ = timed(lambda: nnm_call(name, 2))
            t3, _ = timed(lambda: nnm_call(name, 0))
            if rnd < 0:
                continue
            rec = {"distances": t1, "neighbors": t2 - t1, "mixing": t3 - t2, "whole": t3}
            for k, v in rec.items():
                steps[name][k].append(v)
            emit({"case": f"nnm_{name}", "K": K, "f": F, "d": d, "round": rnd,
                  **{f"{k}_us": v for k, v in rec.items()}})
        Yt = None
        tt, Yt = timed(torch_nnm)
        if rnd >= 0:
            torch_us.append(tt)
            emit({"case": "torch_fp32_rows", "K": K, "f": F, "d": d, "round": rnd, "us": tt})
    for name in ops:
        med = {k: statistics.median(v) for k, v in steps[name].items()}
        emit({"case": f"nnm_{name}", "K": K, "f": F, "d": d, "summary": True, "rounds": a.rounds,
              **{f"{k}_us_median": v for k, v in med.items()},
              "mixing_over_distances": med["mixing"] / med["distances"],
              "mixing_adds_per_s": float(K) * M * d / (med["mixing"] * 1e-6),
              "whole_over_torch_median": med["whole"] / statistics.median(torch_us)})
    emit({"case": "torch_fp32_rows", "K": K, "f": F, "d": d, "summary": True, "rounds": a.rounds,
          "us_median": statistics.median(torch_us), "us_min": min(torch_us),
          "us_max": max(torch_us)})
    # the two agree to fp32 GEMM accuracy, and the layouts bit for bit
    emit({"case": "torch_vs_kernel", "max_abs_diff": (Yt - Yr).abs().max().item(),
          "abs_max": Yr.abs().max().item(),
          "rows_equal_panels": bool(torch.equal(Yp.to_rows(), Yr))})

    if a.out:
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
