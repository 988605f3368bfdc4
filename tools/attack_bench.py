"""The ALIE kernel against the torch formulation and the bytes floor, same process, same box.

    python tools/attack_bench.py [--out profiles/attacks.jsonl] [--rounds 20] [--d 2000000]

K = 1000 clients, B = 200 Byzantine, d columns, the C3 recipe (gm_fill_clients_f32).  After
one warm-up round, `--rounds` interleaved rounds of
  alie      gm_attack_affine_f32 / _bf16 (a = 1, b = -z_max) on fp32 rows, fp32 panels and
            bf16 panels: reads H d elements, writes B d
  torch     h = X[:H]; X[H:] = h.mean(0) - z * h.std(0) on the fp32 rows
  bucket    gm_bucket_means_* at s = 2 on the same three inputs into fp32 panels, whose bytes
            over time is the streaming rate the floor is taken at
each timed by device events around the call.  One JSON line per (case, round); one summary
line per case with the median; one `floor` line per variant: (H d + B d) esize bytes divided
by that variant's bucketing rate, and the kernel's median over it.  Then min-max and min-sum
(dev "std") on the fp32 panels, whole calls timed by the host clock around a device
synchronise.  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K, B = 1000, 200
H = K - B


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
    ctx.call("gm_fill_clients_f32", X.data_ptr(), K, d, d, B, 0.0, 0.05, 0.25, 0.5, 20211, stream)
    src = {"fp32_rows": X, "fp32_panels": bz.ClientPanels.from_rows(X),
           "bf16_panels": bz.ClientPanels.from_rows(X, dtype=torch.bfloat16)}
    Xt = X.clone()                                   # the torch formulation's own matrix
    z = bz.z_max(K, B)
    means = bz.ClientPanels(K // 2, d, device="cuda")

    def operand(name):
        W = src[name]
        panels = name.endswith("panels")
        return ((W.data if panels else W).data_ptr(), W.panel_stride if panels else d,
                _lib.GM_LAYOUT_PANELS if panels else _lib.GM_LAYOUT_ROWS,
                2 if name.startswith("bf16") else 4)

    def alie(name):
        ptr, ldx, layout, esz = operand(name)
        ctx.call("gm_attack_affine_bf16" if esz == 2 else "gm_attack_affine_f32", ptr, K, d, ldx,
                 layout, B, 1.0, -z, stream)
        return float(K) * d * esz

    def bucket(name):
        ptr, ldx, layout, esz = operand(name)
        ctx.call("gm_bucket_means_bf16" if esz == 2 else "gm_bucket_means_f32", ptr, K, d, ldx,
                 layout, None, 2, means.data.data_ptr(), means.panel_stride,
                 _lib.GM_LAYOUT_PANELS, stream)
        return float(K) * d * esz + float(K // 2) * d * 4

    def torch_alie():
        h = Xt[:H]
        Xt[H:] = h.mean(0) - z * h.std(0)
        return float(K) * d * 4

    cases = [("torch_fp32_rows", torch_alie)]
    for name in src:
        cases.append((f"alie_{name}", lambda name=name: alie(name)))
        cases.append((f"bucket_s2_{name}", lambda name=name: bucket(name)))
    us = {name: [] for name, _ in cases}
    nbytes = {}
    for rnd in range(-1, a.rounds):                 # round -1: warm-up, not reported
        for name, fn in cases:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            nbytes[name] = fn()
            e1.record()
            torch.cuda.synchronize()
            t = e0.elapsed_time(e1) * 1e-3
            if rnd < 0:
                continue
            us[name].append(t * 1e6)
            emit({"case": name, "K": K, "B": B, "d": d, "round": rnd, "us": t * 1e6,
                  "bytes": nbytes[name], "bytes_per_s": nbytes[name] / t})
    med = {name: statistics.median(v) for name, v in us.items()}
    for name, _ in cases:
        emit({"case": name, "K": K, "B": B, "d": d, "summary": True, "rounds": a.rounds,
              "us_median": med[name], "us_min": min(us[name]), "us_max": max(us[name]),
              "over_torch_median": med[name] / med["torch_fp32_rows"]})
    for name in src:
        rate = nbytes[f"bucket_s2_{name}"] / (med[f"bucket_s2_{name}"] * 1e-6)
        floor_us = nbytes[f"alie_{name}"] / rate * 1e6
        emit({"case": f"floor_{name}", "K": K, "B": B, "d": d, "summary": True,
              "bucketing_s2_bytes_per_s": rate, "floor_us": floor_us,
              "alie_us_median": med[f"alie_{name}"],
              "alie_over_floor": med[f"alie_{name}"] / floor_us})

    # the matrices agree: the torch row against the kernel's, on the fp32 rows
    diff = (Xt[H] - X[H]).abs().max().item()
    emit({"case": "torch_vs_kernel_row", "max_abs_diff": diff,
          "row_abs_max": X[H].abs().max().item()})

    P = src["fp32_panels"]
    for name, fn in (("minmax_std_fp32_panels", bz.minmax), ("minsum_std_fp32_panels", bz.minsum)):
        wall = []
        for rnd in range(-1, 3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(P, B)
            torch.cuda.synchronize()
            if rnd >= 0:
                wall.append((time.perf_counter() - t0) * 1e6)
        emit({"case": name, "K": K, "B": B, "d": d, "summary": True, "rounds": 3,
              "wall_us_median": statistics.median(wall), "gamma": fn.last_gamma})

    if a.out:
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
