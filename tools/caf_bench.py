"""CAF stage by stage, against a torch formulation of the same K-space algorithm, same process,
same box.

    python tools/caf_bench.py [--out profiles/caf.jsonl] [--rounds 20] [--d 2000000]

K = 1000 clients, f = 200, d columns, the C3 recipe (gm_fill_clients_f32), on fp32 rows and on
fp32 panels, power_iters = 100, power_tol = 1e-10.  After one warm-up round, `--rounds`
interleaved rounds of gm_caf_f32 stopped after the distances (GMAGG_CAF_STOP=1), after the last
round of the filter (=2) and run whole, each timed by device events around the call (the call's
host synchronisations, one per round of the filter, fall inside the events); a round's stage times
are the differences (distance, solver = filter - distance, mean = whole - filter).  In the same
rounds the K-space algorithm as a user would write it in torch, fp64 on the GPU, on the squared
distances of the same matrix (formed once, untimed, from fp64 Gram blocks): it is compared with
the solver stage alone.  Recorded with the times: the filter's rounds, its applications of M in
all, and the solver's time per product with D (applications + 2 per round: a = D p and the
closing y = D z).  One JSON line per (case, round); one summary line per case with the medians.
Needs a GPU: there is no fallback.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K, F = 1000, 200
PIT, PTOL = 100, 1e-10


def torch_dist(X, block=1 << 16):
    """fp64 squared distances from Gram blocks of `block` columns."""
    G = torch.zeros(K, K, dtype=torch.float64, device=X.device)
    for j in range(0, X.shape[1], block):
        Xc = X[:, j:j + block].double()
        G += Xc @ Xc.T
    n = G.diagonal()
    return (n[:, None] + n[None, :] - 2 * G).clamp_(min=0).fill_diagonal_(0)


def torch_caf(D, f, pit=PIT, ptol=PTOL):
    """The definition's K-space route (include/gmagg.h): (c*, S*, rounds, applications)."""
    Kk = D.shape[0]
    c = torch.ones(Kk, dtype=torch.float64, device=D.device)
    best, rec, rounds, apps = float("inf"), None, 0, 0
    for t in range(Kk):
        S = c.sum()
        if not float(S) > Kk - 2 * f:
            break
        p = c / S
        sp = p.sqrt()
        a = D @ p
        rho = a - 0.5 * (p @ a)
        r = int(torch.argmax(p * rho))
        m = sp * sp[r] * (0.5 * (rho + rho[r] - D[r]))
        w = m / m.norm()

        def apply(w):
            z = sp * w
            g = 0.5 * (rho * z.sum() + rho @ z - D @ z)
            return sp * g, g
        for _ in range(pit):
            v, _g = apply(w)
            w1 = v / v.norm()
            apps += 1
            mov = float((w1 - w).norm())
            w = w1
            if mov <= ptol:
                break
        v, g = apply(w)
        lam = float(w @ v)
        rounds += 1
        if lam < best:
            best, rec = lam, (c.clone(), S.clone())
        tau = g * g
        pos = c > 0
        tmax = tau[pos].max()
        c = torch.where(pos, c * (1 - tau / tmax), c)
    return rec[0], float(rec[1]), rounds, apps


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
    D = torch_dist(X)
    out = torch.empty(d, device="cuda")
    wts = torch.empty(K, dtype=torch.float64, device="cuda")
    lam, S = C.c_double(), C.c_double()
    rounds, best = C.c_int32(), C.c_int32()
    nit, conv = (C.c_int32 * K)(), (C.c_int32 * K)()
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

    def caf_call(name, stop):
        x, ldx, lay = ops[name]
        os.environ["GMAGG_CAF_STOP"] = str(stop)
        try:
            ctx.call("gm_caf_f32", x, K, d, ldx, lay, F, PIT, PTOL, out.data_ptr(), wts.data_ptr(),
                     C.byref(lam), C.byref(S), C.byref(rounds), C.byref(best), nit, conv, stream)
        finally:
            os.environ.pop("GMAGG_CAF_STOP", None)

    steps = {nm: {"distance": [], "solver": [], "mean": [], "whole": []} for nm in ops}
    torch_us, outs, weights, counts, tres = [], {}, {}, {}, None
    for rnd in range(-1, a.rounds):                 # round -1: warm-up, not reported
        for name in ops:
            caf_call(name, 1)                       # untimed: the three timed calls start alike
            t1, _ = timed(lambda: caf_call(name, 1))
            t2, _ = timed(lambda: caf_call(name, 2))
            t3, _ = timed(lambda: caf_call(name, 0))
            outs[name], weights[name] = out.clone(), wts.clone()
            apps = sum(nit[:rounds.value])
            counts[name] = {"filter_rounds": rounds.value, "best_round": best.value,
                            "applications": apps, "products": apps + 2 * rounds.value}
            if rnd < 0:
                continue
            rec = {"distance": t1, "solver": t2 - t1, "mean": t3 - t2, "whole": t3}
            for k, v in rec.items():
                steps[name][k].append(v)
            emit({"case": f"caf_{name}", "K": K, "f": F, "d": d, "round": rnd, **counts[name],
                  **{f"{k}_us": v for k, v in rec.items()}})
        tt, tres = timed(lambda: torch_caf(D, F))
        if rnd >= 0:
            torch_us.append(tt)
            emit({"case": "torch_kspace_fp64", "K": K, "f": F, "round": rnd, "us": tt,
                  "filter_rounds": tres[2], "applications": tres[3]})
    tmed = statistics.median(torch_us)
    for name in ops:
        med = {k: statistics.median(v) for k, v in steps[name].items()}
        emit({"case": f"caf_{name}", "K": K, "f": F, "d": d, "summary": True, "rounds": a.rounds,
              **counts[name], **{f"{k}_us_median": v for k, v in med.items()},
              "solver_us_per_product": med["solver"] / counts[name]["products"],
              "solver_over_distance_median": med["solver"] / med["distance"],
              "solver_over_torch_median": med["solver"] / tmed})
    emit({"case": "torch_kspace_fp64", "K": K, "f": F, "summary": True, "rounds": a.rounds,
          "us_median": tmed, "us_min": min(torch_us), "us_max": max(torch_us),
          "filter_rounds": tres[2], "applications": tres[3]})
    # the layouts agree bit for bit; torch works on other distances (fp64 Gram blocks)
    emit({"case": "torch_vs_kernel",
          "max_abs_weight_diff": (tres[0] - weights["fp32_rows"]).abs().max().item(),
          "same_filter_rounds": tres[2] == counts["fp32_rows"]["filter_rounds"],
          "rows_equal_panels": bool(torch.equal(outs["fp32_rows"], outs["fp32_panels"]))
          and bool(torch.equal(weights["fp32_rows"], weights["fp32_panels"]))})

    if a.out:
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
