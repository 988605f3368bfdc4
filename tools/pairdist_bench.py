"""The pair distances on fp32 (exact), bf16 (exact) and bf16 (MFMA), and the whole nnm and
multi_krum calls on each, same process, same box.

    python tools/pairdist_bench.py [--out profiles/pairdist_bf16.jsonl] [--rounds 20]
                                   [--d 2000000] [--small]

K = 1000 clients, f = 200, d columns, the C3 recipe (gm_fill_clients_f32) and its rounding to
bf16, on rows and on panels; then K = 256 at the same d and K = 4096 at d / 16 (rows only where K
has no panel width).  After one warm-up round, `--rounds` rounds in which the variants alternate,
each call timed by device events: the distance step alone (gm_nnm_* stopped after the distances,
GMAGG_NNM_STOP=1), the whole nnm call and the whole multi_krum call.  One JSON line per (case,
variant, round) and one summary line per (case, variant) with the medians; the MFMA summary adds
its speed-up over the bf16 exact tier of the same run, the matrix-core rate it reaches (the FLOPs
of the tile pairs it computes, against 2.5 PFLOP/s dense bf16) and the HBM rate of the bytes it
should read (the operand once, against 6.3 TB/s achievable).  A last line holds the largest
measured |D~ - D| / (rho_i + rho_j) against fp64 on a graded 300 x 4120 input, and the library's
beta.  --small shrinks every shape (a smoke run).  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BF16_FLOPS = 2.5e15
HBM_BYTES_PER_S = 6.3e12
VARIANTS = ("fp32_exact", "bf16_exact", "bf16_mfma")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--d", type=int, default=2_000_000)
    ap.add_argument("--small", action="store_true")
    a = ap.parse_args()
    import byzantine_aircomp_amd as bz
    from byzantine_aircomp_amd import _lib
    from byzantine_aircomp_amd.panels import panel_width
    ctx = bz.context()
    stream = torch.cuda.current_stream().cuda_stream
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3                   # us

    def run_case(K, f, d, layouts):
        X = torch.empty(K, d, device="cuda")
        ctx.call("gm_fill_clients_f32", X.data_ptr(), K, d, d, f, 0.0, 0.05, 0.25, 0.5, 20211,
                 stream)
        Xb = X.to(torch.bfloat16)
        Y = torch.empty(K, d, device="cuda")
        nT = -(-K // 128)
        flops = 2.0 * (nT * (nT + 1) // 2) * 128 * 128 * d
        for layout in layouts:
            if layout == "panels":
                w32, w16 = bz.ClientPanels.from_rows(X), bz.ClientPanels.from_rows(Xb)
                args = {"fp32": (w32.data.data_ptr(), w32.panel_stride, _lib.GM_LAYOUT_PANELS),
                        "bf16": (w16.data.data_ptr(), w16.panel_stride, _lib.GM_LAYOUT_PANELS)}
            else:
                w32, w16 = X, Xb
                args = {"fp32": (X.data_ptr(), d, _lib.GM_LAYOUT_ROWS),
                        "bf16": (Xb.data_ptr(), d, _lib.GM_LAYOUT_ROWS)}

            def dist(variant):
                os.environ["GMAGG_NNM_STOP"] = "1"
                try:
                    if variant == "fp32_exact":
                        x, ld, lay = args["fp32"]
                        ctx.call("gm_nnm_f32", x, K, d, ld, lay, f, Y.data_ptr(), d,
                                 _lib.GM_LAYOUT_ROWS, None, stream)
                    else:
                        x, ld, lay = args["bf16"]
                        mode = _lib.GM_DIST_MFMA if variant == "bf16_mfma" else _lib.GM_DIST_EXACT
                        ctx.call("gm_nnm_bf16", x, K, d, ld, lay, f, mode, Y.data_ptr(), d,
                                 _lib.GM_LAYOUT_ROWS, None, stream)
                finally:
                    os.environ.pop("GMAGG_NNM_STOP", None)

            def kw(variant):
                if variant == "fp32_exact":
                    return w32, {}
                return w16, {"bf16": True, "distances": variant.split("_")[1]}

            def whole_nnm(variant):
                w, k = kw(variant)
                bz.nnm(w, f, layout="rows", **k)

            def whole_mk(variant):
                w, k = kw(variant)
                bz.multi_krum(w, dict(k, honestSize=K - f))

            steps = {v: {"distances": [], "nnm": [], "multi_krum": []} for v in VARIANTS}
            for rnd in range(-1, a.rounds):                # round -1: warm-up, not reported
                for v in VARIANTS:
                    rec = {"distances": timed(lambda: dist(v)), "nnm": timed(lambda: whole_nnm(v)),
                           "multi_krum": timed(lambda: whole_mk(v))}
                    if rnd < 0:
                        continue
                    for k_, t in rec.items():
                        steps[v][k_].append(t)
                    emit({"case": f"K{K}_{layout}", "variant": v, "K": K, "f": f, "d": d,
                          "round": rnd, **{f"{k_}_us": t for k_, t in rec.items()}})
            med = {v: {k_: statistics.median(t) for k_, t in steps[v].items()} for v in VARIANTS}
            for v in VARIANTS:
                rec = {"case": f"K{K}_{layout}", "variant": v, "K": K, "f": f, "d": d,
                       "summary": True, "rounds": a.rounds,
                       **{f"{k_}_us_median": t for k_, t in med[v].items()}}
                if v == "bf16_mfma":
                    info = bz.multi_krum.last_info
                    t = med[v]["distances"] * 1e-6
                    rec.update({
                        "tier": info["tier"], "reason": info["reason"], "slices": info["slices"],
                        "distances_speedup_over_bf16_exact":
                            med["bf16_exact"]["distances"] / med[v]["distances"],
                        "nnm_speedup_over_bf16_exact": med["bf16_exact"]["nnm"] / med[v]["nnm"],
                        "multi_krum_speedup_over_bf16_exact":
                            med["bf16_exact"]["multi_krum"] / med[v]["multi_krum"],
                        "fraction_of_bf16_matrix_peak": flops / t / PEAK_BF16_FLOPS,
                        "fraction_of_hbm": 2.0 * K * d / t / HBM_BYTES_PER_S})
                emit(rec)
            del w32, w16

    def has_panels(K):
        try:
            return panel_width(K, torch.bfloat16) > 0 and panel_width(K) > 0
        except ValueError:
            return False

    d = 8192 if a.small else a.d
    for K, f, dd in ((1000, 200, d), (256, 51, d), (4096, 819, max(256, d // 16))):
        run_case(K, f, dd, ("rows", "panels") if has_panels(K) else ("rows",))

    # the bound, measured: graded rows x_k = 1.02^k z_k against fp64
    g = torch.Generator().manual_seed(0)
    Kg, dg = 300, 4120
    z = torch.randn(Kg, dg, generator=g).double()
    Xg = (z * (torch.tensor(1.02, dtype=torch.float64) ** torch.arange(Kg))[:, None]).float()
    Xg = Xg.to(torch.bfloat16)
    Dt = bz.pair_distances(Xg.to("cuda"), bf16=True, distances="mfma").cpu()
    x = Xg.double()
    rho = (x * x).sum(dim=1)
    D = torch.cdist(x, x) ** 2
    D.fill_diagonal_(0.0)
    ratio = ((Dt - D).abs() / (rho[:, None] + rho[None, :])).max().item()
    emit({"case": "bound_graded_300x4120", "max_ratio": ratio,
          "beta": bz.pair_distances.last_info["beta"], "tier": bz.pair_distances.last_info["tier"]})

    if a.out:
        with open(a.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
