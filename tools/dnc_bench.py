"""DnC stage by stage, against the torch formulation, same process, same box.

    python tools/dnc_bench.py [--out profiles/dnc.jsonl] [--rounds 20] [--d 2000000]

K = 1000 clients, f = 200, d columns, b = 10,000 sampled columns, one round, c = 1 (q = 200), the
C3 recipe (gm_fill_clients_f32), on fp32 rows and on fp32 panels.  The columns are drawn once
(dnc.columns) and handed over on the device: the host draw, O(d) per round, is timed apart
(`draw_us`, wall clock).  After one warm-up round, `--rounds` interleaved rounds of gm_dnc_f32
stopped after the gather (GMAGG_DNC_STOP=1), after the selection (=2) and run whole, each timed
by device events around the call (the call's host synchronisations, one per chunk of power
iterations and one for the good rows, fall inside the events); a round's stage times are the
differences (gather, spectral = selection - gather, mean = whole - selection).  In the same
rounds the formulation a user would write in torch, on the fp32 rows:
    S = X[:, cols].double(); C = S - S.mean(0); v = torch.linalg.svd(C, full_matrices=False).Vh[0]
    s = (C @ v) ** 2; keep = s.topk(K - q, largest=False).indices.sort().values
    out = X[keep].mean(0)
One JSON line per (case, round); one summary line per case with the medians.  Needs a GPU:
there is no fallback.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K, F, B = 1000, 200, 10_000
Q = F


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
    t0 = time.perf_counter()
    cols = bz.dnc.columns(d, B, 1, generator=torch.Generator().manual_seed(1))
    draw_us = (time.perf_counter() - t0) * 1e6
    n = cols.shape[1]
    cdev = cols.cuda()
    out = torch.empty(d, device="cuda")
    scores = torch.empty(1, K, dtype=torch.float64, device="cuda")
    good, n_good = (C.c_int32 * K)(), C.c_int64()
    nit, conv = (C.c_int32 * 1)(), (C.c_int32 * 1)()
    ops = {"fp32_rows": (X.data_ptr(), d, _lib.GM_LAYOUT_ROWS),
           "fp32_panels": (P.data.data_ptr(), P.panel_stride, _lib.GM_LAYOUT_PANELS)}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        res = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3, res             # us

    def dnc_call(name, stop):
        x, ldx, lay = ops[name]
        os.environ["GMAGG_DNC_STOP"] = str(stop)
        try:
            ctx.call("gm_dnc_f32", x, K, d, ldx, lay, cdev.data_ptr(), n, 1, Q, 100, 1e-10,
                     out.data_ptr(), scores.data_ptr(), good, C.byref(n_good), nit, conv, stream)
        finally:
            os.environ.pop("GMAGG_DNC_STOP", None)

    def torch_dnc():
        S = X[:, cdev[0]].double()
        Cm = S - S.mean(0)
        v = torch.linalg.svd(Cm, full_matrices=False).Vh[0]
        s = (Cm @ v) ** 2
        keep = s.topk(K - Q, largest=False).indices.sort().values
        return X[keep].mean(0), keep

    steps = {nm: {"gather": [], "spectral": [], "mean": [], "whole": []} for nm in ops}
    torch_us, sel, outs, tsel, tout = [], {}, {}, None, None
    for rnd in range(-1, a.rounds):                 # round -1: warm-up, not reported
        for name in ops:
            dnc_call(name, 1)                       # untimed: the three timed calls start alike
            t1, _ = timed(lambda: dnc_call(name, 1))
            t2, _ = timed(lambda: dnc_call(name, 2))
            t3, _ = timed(lambda: dnc_call(name, 0))
            sel[name], outs[name] = list(good[:n_good.value]), out.clone()
            if rnd < 0:
                continue
            rec = {"gather": t1, "spectral": t2 - t1, "mean": t3 - t2, "whole": t3}
            for k, v in rec.items():
                steps[name][k].append(v)
            emit({"case": f"dnc_{name}", "K": K, "f": F, "d": d, "b": n, "round": rnd,
                  "power_iters": nit[0], "converged": bool(conv[0]),
                  **{f"{k}_us": v for k, v in rec.items()}})
        tout = None
        tt, (tout, tsel) = timed(torch_dnc)
        if rnd >= 0:
            torch_us.append(tt)
            emit({"case": "torch_fp32_rows", "K": K, "f": F, "d": d, "b": n, "round": rnd, "us": tt})
    tmed = statistics.median(torch_us)
    for name in ops:
        med = {k: statistics.median(v) for k, v in steps[name].items()}
        emit({"case": f"dnc_{name}", "K": K, "f": F, "d": d, "b": n, "summary": True,
              "rounds": a.rounds, **{f"{k}_us_median": v for k, v in med.items()},
              "whole_over_torch_median": med["whole"] / tmed})
    emit({"case": "torch_fp32_rows", "K": K, "f": F, "d": d, "b": n, "summary": True,
          "rounds": a.rounds, "us_median": tmed, "us_min": min(torch_us), "us_max": max(torch_us)})
    emit({"case": "host_draw", "d": d, "b": n, "draw_us": draw_us})
    # the selections agree, the layouts bit for bit; torch's mean is an fp32 sum
    emit({"case": "torch_vs_kernel", "same_selection": sel["fp32_rows"] == tsel.tolist(),
          "max_abs_diff": (tout - outs["fp32_rows"]).abs().max().item(),
          "rows_equal_panels": bool(torch.equal(outs["fp32_rows"], outs["fp32_panels"]))
          and sel["fp32_rows"] == sel["fp32_panels"]})

    if a.out:
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
