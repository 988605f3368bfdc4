"""Time meamed against trimmed_mean, and bulyan's three parts, on the C3 data recipe, HIP events
around each call.

    python tools/robust_bench.py [--K 1000 256] [--d 2000000] [--bulyan-d 1000000] [--reps 5]
                                 [--out profiles/robust_select.jsonl]

One JSON line per measurement (also appended to --out):
  * meamed and trimmed_mean, interleaved in the same run, rows and panels: ms per call (median
    of reps), the HBM rate of the one read of X, and meamed's time over the trimmed mean's;
  * bulyan at K = 1000, f = 100: the whole call (`ms`); `krum_exact_ms`, a whole Krum call on
    the exact path, which stands for the distances but also holds one scoring of every row,
    the argmin, the row copy and the host's wait for the index, so it is an UPPER bound of the
    distances; `stage2_ms` (gm_meamed_f32 on the theta listed rows);
    `stage1_ms_lower` = whole - krum_exact - stage 2, a LOWER bound of the theta selection
    rounds, low by what krum_exact_ms holds beyond the distances (well under 1 ms: a scoring
    of K rows is one of the 800 rounds' two launches).
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, nargs="+", default=[1000, 256])
    ap.add_argument("--d", type=int, default=2_000_000)
    ap.add_argument("--bulyan-K", type=int, default=1000)
    ap.add_argument("--bulyan-f", type=int, default=100)
    ap.add_argument("--bulyan-d", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "robust_select.jsonl"))
    a = ap.parse_args()
    os.environ["GMAGG_KRUM"] = "0"          # the distances part is timed on the exact path
    import byzantine_aircomp_amd as bz
    from byzantine_aircomp_amd import _lib
    ctx = bz.context()
    s = torch.cuda.current_stream().cuda_stream
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def fill(K, d):
        X = torch.empty(K, d, device="cuda")
        _lib.check(ctx.lib.gm_fill_clients_f32(ctx.handle, X.data_ptr(), K, d, d, K // 5, 0.0,
                                               0.05, 0.25, 0.5, 20211, s), "fill")
        return X

    for K in a.K:
        X = fill(K, a.d)
        for layout in ("rows", "panels"):
            Xin = bz.ClientPanels.from_rows(X) if layout == "panels" else X
            opts = {"honestSize": K - K // 5}
            res = {}
            for _ in range(2):              # two interleaved rounds; the second is reported
                res["trimmed_mean"] = timed(lambda: bz.trimmed_mean(Xin), a.reps)
                res["meamed"] = timed(lambda: bz.meamed(Xin, opts), a.reps)
            for name, (ms, lo, hi) in res.items():
                emit({"agg": name, "K": K, "d": a.d, "layout": layout, "ms": ms, "min_ms": lo,
                      "max_ms": hi, "GBps": 4.0 * K * a.d / ms / 1e6,
                      "over_trimmed_mean": ms / res["trimmed_mean"][0]})
            del Xin
        del X

    K, f, d = a.bulyan_K, a.bulyan_f, a.bulyan_d
    X = fill(K, d)
    theta = K - 2 * f
    whole = timed(lambda: bz.bulyan(X, {"honestSize": K - f}), a.reps)
    sel = sorted(bz.bulyan.last_selected)
    dist = timed(lambda: bz.Krum(X, {"honestSize": K - f}), a.reps)
    rows = torch.tensor(sel, dtype=torch.int32, device="cuda")
    o = torch.empty(d, device="cuda")
    stage2 = timed(lambda: ctx.call("gm_meamed_f32", X.data_ptr(), K, d, d, 0, rows.data_ptr(),
                                    theta, theta - 2 * f, o.data_ptr(), s), a.reps)
    emit({"agg": "bulyan", "K": K, "f": f, "d": d, "layout": "rows", "ms": whole[0],
          "min_ms": whole[1], "max_ms": whole[2], "krum_exact_ms": dist[0], "stage2_ms": stage2[0],
          "stage1_ms_lower": whole[0] - dist[0] - stage2[0], "rounds": theta})


if __name__ == "__main__":
    main()
