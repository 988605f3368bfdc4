"""bf16 against fp32 client updates on the fused streaming pass, same process, same box.

    python tools/bf16_bench.py [--out profiles/bf16_bench.jsonl] [--rounds 3] [--only c3,k256]

Two shapes, gm2 on panels, fp32 and bf16 alternating for `--rounds` rounds after one
warm-up call each:
  c3    K=1000 x d=11M, the C3 recipe (gm_fill_clients_f32), packed into fp32 panels and,
        through the converting pack kernel, bf16 panels; both resident at once (44 + 22 GB)
  k256  K=256 x d=15.6M, algo="stream" on both sides (AUTO would take the Gram for fp32)
One JSON line per (shape, dtype, round): the STEP time per pass from gm_ctx_pass_timing,
aggregations/s from the wall time of the call, iterations, `bytes` (element size x K x d,
the matrix the pass reads) over the STEP time as a fraction of 8 TB/s; then one summary line
per shape with the bf16 / fp32 ratio of the median STEP times (the ceiling is 0.5) and the
relative L2 between the two aggregates — they differ by the rounding of the input, so it is
reported, not asserted.  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM = 8.0e12
SHAPES = {"c3": (1000, 11_000_000, 200, "auto"), "k256": (256, 15_600_000, 51, "stream")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="")
    ap.add_argument("--maxiter", type=int, default=1000)
    a = ap.parse_args()
    only = set(filter(None, a.only.split(",")))
    import byzantine_aircomp_amd as bz
    from byzantine_aircomp_amd import _lib
    ctx = bz.context()
    stream = torch.cuda.current_stream().cuda_stream
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    for name, (K, d, B, algo) in SHAPES.items():
        if only and name not in only:
            continue
        X = torch.empty(K, d, device="cuda")
        _lib.check(ctx.lib.gm_fill_clients_f32(ctx.handle, X.data_ptr(), K, d, d, B, 0.0, 0.05,
                                               0.25, 0.5, 20211, stream), "fill")
        g0 = torch.empty(d, device="cuda")
        _lib.check(ctx.lib.gm_fill_normal_f32(ctx.handle, g0.data_ptr(), d, 0.0, 0.01, 20212,
                                              stream), "fill")
        panels = {"fp32": bz.ClientPanels.from_rows(X),
                  "bf16": bz.ClientPanels.from_rows(X, dtype=torch.bfloat16)}
        del X
        torch.cuda.synchronize()
        opts = {"maxiter": a.maxiter, "tol": 1e-5, "guess": g0, "algo": algo}
        outs, step = {}, {"fp32": [], "bf16": []}
        for rnd in range(-1, a.rounds):             # round -1: warm-up, not reported
            for dt, P in panels.items():
                ctx.pass_timing(True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = bz.gm2(P, dict(opts))
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
                ms, n = ctx.pass_timing(False)
                res = bz.aggregators.last_result
                if rnd < 0:
                    continue
                outs[dt] = out
                per = ms / 1e3 / max(n, 1)
                nbytes = float(P.data.element_size()) * K * d
                step[dt].append(per)
                emit({"shape": name, "K": K, "d": d, "dtype": dt, "W": P.W, "round": rnd,
                      "algo": res.algo, "iters": res.iters, "step_passes": n,
                      "step_us": per * 1e6, "agg_per_s": 1.0 / wall, "bytes": nbytes,
                      "hbm_frac": nbytes / per / HBM,
                      "pass_variant": os.environ.get("GMAGG_PASS_VARIANT", "")})
        a32, a16 = outs["fp32"].double(), outs["bf16"].double()
        emit({"shape": name, "K": K, "d": d, "summary": True,
              "step_us_fp32_median": statistics.median(step["fp32"]) * 1e6,
              "step_us_bf16_median": statistics.median(step["bf16"]) * 1e6,
              "bf16_over_fp32_step": statistics.median(step["bf16"]) / statistics.median(step["fp32"]),
              "rel_l2_bf16_vs_fp32": float((a16 - a32).norm() / a32.norm()),
              "pass_variant": os.environ.get("GMAGG_PASS_VARIANT", "")})
        del panels, outs
        torch.cuda.empty_cache()

    if a.out:
        with open(a.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
