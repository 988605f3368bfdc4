"""Runs every single-problem shape of tests/resident_cases.py once (gm2, one body, explicit
algo="resident") and writes "CASE K op which d" to stderr ahead of each call.  Started by
tests/test_gpu_resident_tiles.py as a fresh process under GMAGG_RES_VERBOSE=1, which the library
reads once per process and under which it reports each resident launch's nb and stride on
stderr: the parent pairs the lines and compares them with the restated plan, so that every
case is known to have run the CPB it was written for.  Values are not compared here, so the
inputs are drawn on the device."""
import os
import sys

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import resident_cases as rc

OPS = ("rows4", "rows2", "rows1", "panels")


def cases(num_cu):
    """[(K, op, which, d)]"""
    out = []
    for K in rc.EDGE_K:
        for op in OPS:
            if op == "panels" and K > rc.PANEL_K_MAX:
                continue
            out += [(K, op, which, d) for which, d in rc.single_ds(K, op, num_cu).items()]
    return out


def main():
    import byzantine_aircomp_amd as bz
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    gen = torch.Generator(device="cuda").manual_seed(1)
    for K, op, which, d in cases(num_cu):
        X = torch.randn(K, d, generator=gen, device="cuda")
        g = 0.1 * torch.randn(d, generator=gen, device="cuda")
        w = bz.ClientPanels.from_rows(X) if op == "panels" else X
        sys.stderr.write(f"CASE {K} {op} {which} {d}\n")
        sys.stderr.flush()
        out = bz.gm2(w, {"maxiter": 1, "tol": -1.0, "guess": g, "algo": "resident"})
        res = bz.aggregators.last_result
        assert res.algo == "resident" and res.iters == 1 and bool(torch.isfinite(out).all())
    print(len(cases(num_cu)))


if __name__ == "__main__":
    main()
