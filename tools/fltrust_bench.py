"""FLTrust against the torch formulation, same process, same box.

    python tools/fltrust_bench.py [--out profiles/fltrust.jsonl] [--rounds 20] [--d 2000000]
                                  [--kernel-stats DIR]
    rocprofv3 --kernel-trace --stats -d DIR/<variant> -- \
        python tools/fltrust_bench.py --profile-only <variant> [--rounds 5]

K = 1000 clients, d columns: c = 0.07 N, a true direction t = 0.01 N, the server update
g = t + 0.005 N, honest updates t + 0.02 N, and the last B = 200 rows sign-flipped (-3 u: TS = 0,
so pass B reads 800 rows).  Variants: fp32 and bf16, rows and panels, and fp32 rows one element
into their buffer with an odd row stride (no 16-byte alignment: the one-column path).  After
one warm-up round, `--rounds` rounds alternate, per variant, between
  fltrust   bz.fltrust (gm_fltrust_f32 / _bf16): the whole call
  torch     U = X - c; a = U @ g; n = (U * U).sum(1); out = c + coef @ U on the same dtype's
            rows (bf16 rows are widened first, as the kernels do in registers)
each timed by device events around the call.  One JSON line per variant: the whole call's
median, min and max, the torch formulation's from the same run, their ratio, the algorithmic
bytes of each pass (A: K d esz, B: m d esz) and, with --kernel-stats, the per-pass kernel
times of a separate `rocprofv3 --kernel-trace --stats` run of `--profile-only <variant>` (DIR
holds one sub-directory per variant) with each pass's HBM rate from those bytes.
Needs a GPU: there is no fallback.
"""
import argparse
import csv
import glob
import json
import os
import sqlite3
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K, B = 1000, 200
VARIANTS = ("fp32_rows", "fp32_panels", "bf16_rows", "bf16_panels", "fp32_rows_misaligned")
PASSES = {"flt_row_stats": "pass_a", "flt_reduce": "reduce", "flt_kspace": "kspace",
          "flt_weighted_rows": "pass_b"}


def build(d):
    """(X fp32 [K, d], s [d], c [d]) on the GPU, drawn in row blocks."""
    gen = torch.Generator(device="cuda").manual_seed(20212)
    N = lambda *shape: torch.randn(*shape, generator=gen, device="cuda")  # noqa: E731
    c, t = 0.07 * N(d), 0.01 * N(d)
    s = c + t + 0.005 * N(d)
    X = torch.empty(K, d, device="cuda")
    for k0 in range(0, K, 50):
        u = t + 0.02 * N(50, d)
        if k0 >= K - B:
            u = -3.0 * u
        X[k0:k0 + 50] = c + u
    return X, s, c


def kernel_stats(root, variant):
    """Average, min and max µs per launch of the four kernels of a variant's kernel trace:
    rocprofv3's results database (its `kernels` view), or its kernel stats CSV where it wrote one."""
    out = {}
    for path in glob.glob(os.path.join(root, variant, "**", "*.db"), recursive=True):
        con = sqlite3.connect(path)
        rows = con.execute("select name, count(*), avg(end - start), min(end - start), "
                           "max(end - start) from kernels group by name").fetchall()
        con.close()
        for name, calls, avg, lo, hi in rows:
            for key, label in PASSES.items():
                if key in name:
                    out.update({label + "_us": avg * 1e-3, label + "_us_min": lo * 1e-3,
                                label + "_us_max": hi * 1e-3, label + "_calls": int(calls)})
    for path in glob.glob(os.path.join(root, variant, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Name") or row.get("KernelName") or ""
                for key, label in PASSES.items():
                    if key in name and label + "_us" not in out:
                        out[label + "_us"] = float(row.get("AverageNs") or row["Average"]) * 1e-3
                        out[label + "_calls"] = int(float(row.get("Calls", 0)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--d", type=int, default=2_000_000)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--profile-only", default=None, choices=VARIANTS)
    a = ap.parse_args()
    d = a.d
    import byzantine_aircomp_amd as bz
    X, s, c = build(d)
    opts = {"server_update": s, "guess": c}

    def operand(name):
        dt = torch.bfloat16 if name.startswith("bf16") else torch.float32
        if name.endswith("panels"):
            return bz.ClientPanels.from_rows(X, dtype=dt)
        if name.endswith("misaligned"):
            # one element into its buffer, an odd row stride: the one-column path of both passes
            ld = d + 1 if d % 2 == 0 else d + 2
            buf = torch.empty(K * ld + 1, device="cuda")
            view = buf[1:].view(K, ld)[:, :d]
            view.copy_(X)
            return view
        return X if dt == torch.float32 else X.to(dt)

    if a.profile_only:
        W = operand(a.profile_only)
        for _ in range(a.rounds):
            bz.fltrust(W, opts)
        torch.cuda.synchronize()
        return

    def torch_fltrust(R):
        U = R.float() - c if R.dtype != torch.float32 else R - c
        g = s - c
        av, nv, ng = U @ g, (U * U).sum(1), g @ g
        ts = torch.relu(av / torch.sqrt(nv * ng))
        coef = ts * torch.sqrt(ng / nv) / ts.sum()
        return c + coef @ U

    lines = []
    for name in VARIANTS:
        W = operand(name)
        R = W if isinstance(W, torch.Tensor) else (X if name.startswith("fp32") else X.to(W.dtype))
        esz = 2 if name.startswith("bf16") else 4
        us = {"fltrust": [], "torch": []}
        res = {}
        for rnd in range(-1, a.rounds):              # round -1: warm-up, not reported
            for who, fn in (("fltrust", lambda: bz.fltrust(W, opts)),
                            ("torch", lambda: torch_fltrust(R))):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                res[who] = fn()
                e1.record()
                torch.cuda.synchronize()
                if rnd >= 0:
                    us[who].append(e0.elapsed_time(e1) * 1e3)
        m = int((bz.fltrust.last_info["trust"] > 0).sum())
        med = {k: statistics.median(v) for k, v in us.items()}
        rec = {"case": f"fltrust_{name}", "K": K, "B": B, "d": d, "rounds": a.rounds, "m": m,
               "us_median": med["fltrust"], "us_min": min(us["fltrust"]),
               "us_max": max(us["fltrust"]), "torch_us_median": med["torch"],
               "torch_us_min": min(us["torch"]), "torch_us_max": max(us["torch"]),
               "over_torch_median": med["fltrust"] / med["torch"],
               "pass_a_bytes": float(K) * d * esz, "pass_b_bytes": float(m) * d * esz,
               "max_abs_diff_vs_torch": (res["fltrust"] - res["torch"]).abs().max().item(),
               "out_abs_max": res["fltrust"].abs().max().item()}
        if a.kernel_stats:
            ks = kernel_stats(a.kernel_stats, name)
            rec.update(ks)
            for p in ("pass_a", "pass_b"):
                if p + "_us" in ks:
                    rec[p + "_bytes_per_s"] = rec[p + "_bytes"] / (ks[p + "_us"] * 1e-6)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del W, R
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
