"""s-bucketing against the project's pure copy (the pack kernel), same process, same box.

    python tools/bucket_bench.py [--out profiles/bucketing.jsonl] [--rounds 5] [--d 2000000]

K = 1000 clients x d columns, the C3 recipe (gm_fill_clients_f32).  After one warm-up round,
`--rounds` interleaved rounds of
  pack      gm_rows_to_panels_f32, fp32 rows -> fp32 panels: reads and writes K d 4 bytes
  bucket    gm_bucket_means_f32 / _bf16 into preallocated fp32 panels, for fp32 and bf16,
            rows in and panels in, s in {2, 4}: reads K d esize bytes, writes ceil(K/s) d 4
each timed by device events around the one launch.  One JSON line per (case, round) with the
microseconds, the bytes actually moved and bytes / time as a fraction of 8 TB/s; one summary
line per case with the median and its ratio to the pack kernel's median.  Then the
end-to-end pair, whole calls timed by the host clock around a device synchronise: gm2 on the
K = 1000 fp32 panels against bucketing(s = 2) + gm2 on the 500 bucket means (same tol, same
guess), each with its iteration count.  Needs a GPU: there is no fallback.
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
K = 1000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
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
    ctx.call("gm_fill_clients_f32", X.data_ptr(), K, d, d, K // 5, 0.0, 0.05, 0.25, 0.5, 20211,
             stream)
    g0 = torch.empty(d, device="cuda")
    ctx.call("gm_fill_normal_f32", g0.data_ptr(), d, 0.0, 0.01, 20212, stream)
    src = {("fp32", "rows"): X, ("bf16", "rows"): X.to(torch.bfloat16)}
    src[("fp32", "panels")] = bz.ClientPanels.from_rows(X)
    src[("bf16", "panels")] = bz.ClientPanels.from_rows(src[("bf16", "rows")])
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(1)).to("cuda", torch.int32)
    packed = bz.ClientPanels(K, d, device="cuda")
    outs = {s: bz.ClientPanels(-(-K // s), d, device="cuda") for s in (2, 4)}

    def pack():
        ctx.call("gm_rows_to_panels_f32", X.data_ptr(), K, d, d, packed.data.data_ptr(), packed.W,
                 packed.panel_stride, stream)
        return 2.0 * K * d * 4

    def bucket(dt, lay, s):
        W = src[(dt, lay)]
        Y = outs[s]
        panels = lay == "panels"
        ctx.call("gm_bucket_means_bf16" if dt == "bf16" else "gm_bucket_means_f32",
                 (W.data if panels else W).data_ptr(), K, d, W.panel_stride if panels else d,
                 _lib.GM_LAYOUT_PANELS if panels else _lib.GM_LAYOUT_ROWS, perm.data_ptr(), s,
                 Y.data.data_ptr(), Y.panel_stride, _lib.GM_LAYOUT_PANELS, stream)
        return float(K) * d * (2 if dt == "bf16" else 4) + float(Y.K) * d * 4

    cases = [("pack_f32_rows_to_panels", pack)]
    for s in (2, 4):
        for dt in ("fp32", "bf16"):
            for lay in ("rows", "panels"):
                cases.append((f"bucket_{dt}_{lay}_to_panels_s{s}",
                              lambda dt=dt, lay=lay, s=s: bucket(dt, lay, s)))
    us = {name: [] for name, _ in cases}
    for rnd in range(-1, a.rounds):                 # round -1: warm-up, not reported
        for name, fn in cases:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            nbytes = fn()
            e1.record()
            torch.cuda.synchronize()
            t = e0.elapsed_time(e1) * 1e-3
            if rnd < 0:
                continue
            us[name].append(t * 1e6)
            emit({"case": name, "K": K, "d": d, "round": rnd, "us": t * 1e6, "bytes": nbytes,
                  "hbm_frac": nbytes / t / HBM})
    pack_med = statistics.median(us["pack_f32_rows_to_panels"])
    for name, _ in cases:
        med = statistics.median(us[name])
        emit({"case": name, "K": K, "d": d, "summary": True, "us_median": med,
              "over_pack_median": med / pack_med})

    # end to end: the whole call, K = 1000 panels against bucketing(s = 2) + gm2 on 500 means
    P = src[("fp32", "panels")]
    opts = {"maxiter": 1000, "tol": 1e-5, "guess": g0}
    gen = torch.Generator()
    both = bz.bucketed(bz.gm2, 2, generator=gen, layout="panels")
    wall = {"gm2_K1000_panels": [], "bucketing_s2_plus_gm2_K500_panels": []}
    for rnd in range(-1, a.rounds):
        for name, fn in (("gm2_K1000_panels", bz.gm2), ("bucketing_s2_plus_gm2_K500_panels", both)):
            gen.manual_seed(1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(P, dict(opts))
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
            res = bz.aggregators.last_result
            if rnd < 0:
                continue
            wall[name].append(t)
            emit({"case": name, "K": K, "d": d, "round": rnd, "wall_us": t * 1e6,
                  "iters": res.iters, "algo": res.algo})
    m0, m1 = (statistics.median(v) for v in wall.values())
    emit({"case": "end_to_end", "K": K, "d": d, "summary": True, "gm2_K1000_us_median": m0 * 1e6,
          "bucketed_s2_us_median": m1 * 1e6, "bucketed_over_plain": m1 / m0})

    if a.out:
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
