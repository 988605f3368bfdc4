"""Time mean / median / trimmed_mean on bf16 client updates against the fp32 entry points, on
the C3 data recipe (tools/select_bench.py's fill), HIP events around each call.

    python tools/select_bf16_bench.py [--K 1000 256] [--d 2000000] [--reps 20] [--rounds 2]
                                      [--out profiles/select_bf16.jsonl]

For each (K, layout, aggregator) three routes of the same call are timed in one process,
alternating, after a warm-up of every one:
    bf16   the bf16 entry point on the bf16 matrix (rows in place / bf16 ClientPanels;
           ``options={"bf16": True}``)
    fp32   the fp32 entry point on the widened matrix, prepared outside the timed region
    cast   what a bf16 caller had to do without the bf16 entry points: widen, then the fp32
           entry point, the cast inside the timed region (rows: ``X.float()``; panels:
           ``P.to_rows().float()``, the cheapest way from bf16 panels to something the fp32
           functions read)
One JSON line per (round, K, layout, aggregator, route): ms (the median of --reps), the fastest
and slowest repetition, and GBps_bf16 = the rate of the one read of the bf16 matrix (2 K d
bytes) for every route, so the lines of one shape compare directly.  The whole schedule runs
--rounds times: the difference between a line of round 1 and the same line of round 2 is the
spread of repeated identical runs.  A final "summary" line per shape gives that spread and the
ratios cast / bf16 and fp32 / bf16 of the round medians.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

AGGS = ("mean", "median", "trimmed_mean")
ROUTES = ("bf16", "fp32", "cast")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, nargs="+", default=[1000, 256])
    ap.add_argument("--d", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--layouts", nargs="+", default=["rows", "panels"], choices=["rows", "panels"])
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    import byzantine_aircomp_amd as bz
    from byzantine_aircomp_amd import _lib
    ctx = bz.context()
    s = torch.cuda.current_stream().cuda_stream
    sink = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    medians = {}
    for rnd in range(1, a.rounds + 1):
        for K in a.K:
            X = torch.empty(K, a.d, device="cuda")
            _lib.check(ctx.lib.gm_fill_clients_f32(ctx.handle, X.data_ptr(), K, a.d, a.d, K // 5,
                                                   0.0, 0.05, 0.25, 0.5, 20211, s), "fill")
            Xb = X.to(torch.bfloat16)
            X.copy_(Xb)                                   # the widened matrix
            for layout in a.layouts:
                if layout == "panels":
                    b16, f32 = bz.ClientPanels.from_rows(Xb), bz.ClientPanels.from_rows(X)
                    widen = lambda: b16.to_rows().float()  # noqa: E731
                else:
                    b16, f32 = Xb, X
                    widen = lambda: b16.float()            # noqa: E731
                for name in AGGS:
                    fn = getattr(bz, name)
                    calls = {"bf16": lambda: fn(b16, {"bf16": True}), "fp32": lambda: fn(f32),
                             "cast": lambda: fn(widen())}
                    outs = {r: calls[r]() for r in ROUTES}          # warm-up, and the same bits
                    torch.cuda.synchronize()
                    same = all(torch.equal(outs["bf16"].view(torch.int32),
                                           outs[r].view(torch.int32)) for r in ("fp32", "cast"))
                    del outs
                    ts = {r: [] for r in ROUTES}
                    for _ in range(a.reps):
                        for r in ROUTES:
                            ts[r].append(timed(calls[r]))
                    for r in ROUTES:
                        ms = statistics.median(ts[r])
                        medians.setdefault((K, layout, name, r), []).append(ms)
                        emit({"round": rnd, "agg": name, "K": K, "d": a.d, "layout": layout,
                              "route": r, "dtype": "fp32" if r == "fp32" else "bf16", "ms": ms,
                              "ms_min": min(ts[r]), "ms_max": max(ts[r]),
                              "GBps_bf16": 2.0 * K * a.d / ms / 1e6,
                              "same_bits_as_fp32": same})
                del b16, f32
            del X, Xb
            torch.cuda.empty_cache()
    for (K, layout, name, r), ms in medians.items():
        if r != "bf16":
            continue
        other = {q: medians[(K, layout, name, q)] for q in ROUTES}
        spread = max((max(v) - min(v)) / min(v) for v in other.values())
        mid = {q: statistics.median(v) for q, v in other.items()}
        emit({"summary": True, "agg": name, "K": K, "d": a.d, "layout": layout,
              "ms": {q: round(mid[q], 4) for q in ROUTES}, "round_spread": round(spread, 4),
              "cast_over_bf16": round(mid["cast"] / mid["bf16"], 3),
              "fp32_over_bf16": round(mid["fp32"] / mid["bf16"], 3)})
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
