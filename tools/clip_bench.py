"""Norm clipping (ARC) against the torch formulation, same process, same box.

    python tools/clip_bench.py [--out profiles/clip.jsonl] [--rounds 20] [--d 2000000]
                               [--kernel-stats DIR]
    rocprofv3 --kernel-trace --stats -d DIR/<variant> -- \
        python tools/clip_bench.py --profile-only <variant> [--rounds 5]

K = 1000 clients, f = 200, d columns: c = 0.07 N, a true direction t = 0.01 N, honest updates
t + 0.02 N, and the last 200 rows scaled (100 u).  ARC clips k = (2 f (K - f)) // K = 320 rows.
Variants: fp32 and bf16, rows and panels, out of place, and fp32 rows and panels in place (X
restored from a copy before every call, outside the timed region).  After one warm-up round,
`--rounds` rounds alternate, per variant, between
  arc     bz.arc (gm_clip_rows_f32 / _bf16): the whole call
  torch   U = X - c; n = fp64 norms of U; T = the (k + 1)-th largest; Y = c + s[:, None] * U
          on the same dtype's rows (bf16 rows are widened first, as the kernels do in registers)
each timed by device events around the call.  One JSON line per variant: the whole call's
median, min and max, the torch formulation's from the same run, their ratio, the algorithmic
bytes of each pass (1: K d esz read; 2: out of place K d esz read + K d 4 written, in place
m d 4 read + m d 4 written, m the clipped rows) and, with --kernel-stats, the per-pass kernel
times of a separate `rocprofv3 --kernel-trace --stats` run of `--profile-only <variant>` (DIR
holds one sub-directory per variant) with each pass's HBM rate from those bytes.  Every line
also carries the median of a device-to-device copy of the fp32 matrix from the same run (2 K d 4
bytes moved): the yardstick for pass 2, which writes as many bytes as it reads.  The profiled
run also calls bz.fltrust on the same operand, so FLTrust's pass A (K d esz read) and pass B
(m' d esz read, m' its trusted rows) are re-measured next to pass 1 and pass 2.
Needs a GPU: there is no fallback.
"""
import argparse
import glob
import json
import os
import sqlite3
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K, F = 1000, 200
VARIANTS = ("fp32_rows", "fp32_panels", "bf16_rows", "bf16_panels", "fp32_rows_inplace",
            "fp32_panels_inplace")
PASSES = {"clip_row_norms": "pass_1", "clip_reduce": "reduce", "clip_kspace": "kspace",
          "clip_apply": "pass_2", "flt_row_stats": "flt_pass_a", "flt_weighted_rows": "flt_pass_b"}


def build(d):
    """(X fp32 [K, d], c [d], s [d]: a server update for the FLTrust passes) on the GPU."""
    gen = torch.Generator(device="cuda").manual_seed(20213)
    N = lambda *shape: torch.randn(*shape, generator=gen, device="cuda")  # noqa: E731
    c, t = 0.07 * N(d), 0.01 * N(d)
    s = c + t + 0.005 * N(d)
    X = torch.empty(K, d, device="cuda")
    for k0 in range(0, K, 50):
        u = t + 0.02 * N(50, d)
        if k0 >= K - F:
            u = 100.0 * u
        X[k0:k0 + 50] = c + u
    return X, c, s


def kernel_stats(root, variant):
    """Average, min and max µs per launch of the kernels of a variant's kernel trace (rocprofv3's
    results database, its `kernels` view), as tools/fltrust_bench.py reads them."""
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
    X, c, srv = build(d)
    k = (2 * F * (K - F)) // K

    def operand(name):
        dt = torch.bfloat16 if name.startswith("bf16") else torch.float32
        if "panels" in name:
            return bz.ClientPanels.from_rows(X, dtype=dt)
        if name.endswith("inplace"):
            return X.clone()
        return X if dt == torch.float32 else X.to(dt)

    def restore(W, keep):
        (W.data if isinstance(W, bz.ClientPanels) else W).copy_(keep)

    if a.profile_only:
        name = a.profile_only
        W = operand(name)
        inplace = name.endswith("inplace")
        keep = (W.data if isinstance(W, bz.ClientPanels) else W).clone() if inplace else None
        for _ in range(a.rounds):
            bz.fltrust(W, {"server_update": srv, "guess": c})
            bz.arc(W, F, centre=c, inplace=inplace)
            if inplace:
                restore(W, keep)
        torch.cuda.synchronize()
        return

    def torch_arc(R):
        U = R.float() - c if R.dtype != torch.float32 else R - c
        n = torch.linalg.vector_norm(U, dim=1, dtype=torch.float64)
        T = torch.topk(n, k + 1).values[-1]
        s = torch.clamp(T / n, max=1.0)
        return c + s[:, None].to(torch.float32) * U

    # the yardstick for pass 2, which writes as many bytes as it reads: a device-to-device copy
    # of the fp32 matrix (K d 4 bytes read, as many written), timed the same way
    Yc = torch.empty_like(X)
    cus = []
    for rnd in range(-1, a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        Yc.copy_(X)
        e1.record()
        torch.cuda.synchronize()
        if rnd >= 0:
            cus.append(e0.elapsed_time(e1) * 1e3)
    del Yc
    copy_us = statistics.median(cus)

    lines = []
    for name in VARIANTS:
        W = operand(name)
        inplace = name.endswith("inplace")
        panels = isinstance(W, bz.ClientPanels)
        R = W if not panels else (X if name.startswith("fp32") else X.to(W.dtype))
        keep = (W.data if panels else W).clone() if inplace else None
        R = keep.view_as(R) if inplace and not panels else R
        esz = 2 if name.startswith("bf16") else 4
        us = {"arc": [], "torch": []}
        res = {}
        for rnd in range(-1, a.rounds):              # round -1: warm-up, not reported
            for who, fn in (("arc", lambda: bz.arc(W, F, centre=c, inplace=inplace)),
                            ("torch", lambda: torch_arc(R))):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                out = fn()
                e1.record()
                torch.cuda.synchronize()
                if rnd >= 0:
                    us[who].append(e0.elapsed_time(e1) * 1e3)
                if rnd == a.rounds - 1:
                    res[who] = (out.to_rows() if isinstance(out, bz.ClientPanels) else out).clone()
                del out
                if inplace and who == "arc":
                    restore(W, keep)
        m = int(bz.arc.last_info["clipped"])
        bz.fltrust(W, {"server_update": srv, "guess": c})
        mt = int((bz.fltrust.last_info["trust"] > 0).sum())
        med = {key: statistics.median(v) for key, v in us.items()}
        p2 = 2.0 * m * d * 4 if inplace else float(K) * d * (esz + 4)
        rec = {"case": f"arc_{name}", "K": K, "f": F, "k": k, "d": d, "rounds": a.rounds,
               "clipped": m, "us_median": med["arc"], "us_min": min(us["arc"]),
               "us_max": max(us["arc"]), "torch_us_median": med["torch"],
               "torch_us_min": min(us["torch"]), "torch_us_max": max(us["torch"]),
               "over_torch_median": med["arc"] / med["torch"],
               "pass_1_bytes": float(K) * d * esz, "pass_2_bytes": p2,
               "copy_us_median": copy_us, "copy_bytes_per_s": 2.0 * K * d * 4 / (copy_us * 1e-6),
               "max_abs_diff_vs_torch": (res["arc"] - res["torch"]).abs().max().item()}
        if a.kernel_stats:
            ks = kernel_stats(a.kernel_stats, name)
            rec.update(ks)
            for p in ("pass_1", "pass_2"):
                if p + "_us" in ks:
                    rec[p + "_bytes_per_s"] = rec[p + "_bytes"] / (ks[p + "_us"] * 1e-6)
            if "flt_pass_a_us" in ks:
                rec["flt_pass_a_bytes_per_s"] = float(K) * d * esz / (ks["flt_pass_a_us"] * 1e-6)
            if "flt_pass_b_us" in ks:
                rec["flt_trusted"] = mt
                rec["flt_pass_b_bytes_per_s"] = float(mt) * d * esz / (ks["flt_pass_b_us"] * 1e-6)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del W, R, res, keep
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
