"""Per-pass time of centered clipping against gm2 on the fused streaming pass, same process.

    python tools/cclip_probe.py [--out profiles/cclip_pass.jsonl] [--rounds 5] [--d 2000000]

K=1000 clients (the C3 recipe, gm_fill_clients_f32), d columns, as fp32 and bf16, on panels
and on rows.  For each (layout, dtype) gm2 and cclip alternate for `--rounds` rounds after
one warm-up call each, both running exactly `--iters` iterations (gm2: a negative tol;
cclip: clip_tol=None) with algo="stream".  One JSON line per call: the STEP time per pass
from gm_ctx_pass_timing and the fraction of 8 TB/s its bytes make; then one summary line per
(layout, dtype) with the medians, the spread of the gm2 runs and cclip's excess over gm2.
On panels both run the same kernel; on fp32 rows at 512 < K <= 1024 gm2 runs the 32-wave rows
kernel (rows_pass.hip) and cclip the generic tile, so a gap is expected there (DESIGN.md
§3.1, §3.4).  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--K", type=int, default=1000)
    ap.add_argument("--d", type=int, default=2_000_000)
    a = ap.parse_args()
    import byzantine_aircomp_amd as bz
    from byzantine_aircomp_amd import _lib
    ctx = bz.context()
    stream = torch.cuda.current_stream().cuda_stream
    K, d = a.K, a.d
    X = torch.empty(K, d, device="cuda")
    _lib.check(ctx.lib.gm_fill_clients_f32(ctx.handle, X.data_ptr(), K, d, d, K // 5, 0.0, 0.05,
                                           0.25, 0.5, 20211, stream), "fill")
    g0 = torch.empty(d, device="cuda")
    _lib.check(ctx.lib.gm_fill_normal_f32(ctx.handle, g0.data_ptr(), d, 0.0, 0.01, 20212, stream),
               "fill")
    tau = 0.2 * d ** 0.5                       # clips the Byzantine rows only
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    def operands():
        yield "panels", "fp32", bz.ClientPanels.from_rows(X)
        yield "panels", "bf16", bz.ClientPanels.from_rows(X, dtype=torch.bfloat16)
        yield "rows", "fp32", X
        yield "rows", "bf16", X.to(torch.bfloat16)

    calls = {
        "gm2": lambda W: bz.gm2(W, {"maxiter": a.iters, "tol": -1.0, "guess": g0,
                                    "algo": "stream"}),
        "cclip": lambda W: bz.cclip(W, {"tau": tau, "clip_iters": a.iters, "guess": g0}),
    }
    for layout, dt, W in operands():
        nbytes = (2.0 if dt == "bf16" else 4.0) * K * d
        step = {"gm2": [], "cclip": []}
        for rnd in range(-1, a.rounds):             # round -1: warm-up, not reported
            for agg, call in calls.items():
                ctx.pass_timing(True)
                call(W)
                torch.cuda.synchronize()
                ms, n = ctx.pass_timing(False)
                res = bz.aggregators.last_result
                assert res.iters == a.iters == n, (agg, res, n)
                if rnd < 0:
                    continue
                per = ms / 1e3 / n
                step[agg].append(per)
                emit({"K": K, "d": d, "layout": layout, "dtype": dt, "agg": agg, "round": rnd,
                      "iters": res.iters, "step_us": per * 1e6, "hbm_frac": nbytes / per / HBM})
        m2, mc = statistics.median(step["gm2"]), statistics.median(step["cclip"])
        emit({"K": K, "d": d, "layout": layout, "dtype": dt, "summary": True,
              "gm2_step_us_median": m2 * 1e6, "cclip_step_us_median": mc * 1e6,
              "gm2_spread_us": (max(step["gm2"]) - min(step["gm2"])) * 1e6,
              "cclip_spread_us": (max(step["cclip"]) - min(step["cclip"])) * 1e6,
              "cclip_minus_gm2_us": (mc - m2) * 1e6, "cclip_over_gm2": mc / m2})
        del W
        torch.cuda.empty_cache()

    if a.out:
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
