"""Runs the reduced streaming-pass list and prints one line per case: the sha256 of the output's
bytes, the iteration count and the last movement as hex.  GMAGG_PASS_VARIANT is read once per
process, so tests/test_gpu_stream_tiles.py imports this module for the default schedule and
starts it as a script, one fresh process per forced variant, and requires identical lines
("the results are the same bits", csrc/stream_pass.hip).

The list: per K of stream_cases.MULTI_K and per operand (fp32 rows with V = 4, fp32 panels,
bf16 panels) the operand's multi-chunk shape (stream_cases.multi_d: every block walks at least
3 chunks of the operand's own width: a prologue, a steady state and an epilogue of the rolling
prefetch) and its two-chunk shape, gm2 and cclip with n = 2.  Bits are compared, not values, so
the inputs need no host copy: stream_cases.tile_input's recipe drawn on the device
(device_input), the same in every process on one device."""
import hashlib
import math
import os
import sys

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import stream_cases as sc

OPS = sc.MULTI_OPS
AGGS = ("gm2", "cclip")
N = 2


def shapes(num_cu):
    """[(K, d, operands)]: per K the multi-chunk and the two-chunk shape of each operand, the
    operands of one d together."""
    out = []
    for K in sc.MULTI_K:
        by_d = {}
        for op in OPS:
            for d in (sc.multi_d(K, op, num_cu), sc.small_ds(K, op)[1]):
                by_d.setdefault(d, []).append(op)
        out += [(K, d, ops) for d, ops in sorted(by_d.items())]
    return out


def device_input(K, d):
    """(X [K, d], guess [d]) on the GPU: tile_input's recipe (graded honest rows, K // 5
    Byzantine rows, shuffled) from torch.Generator(device="cuda").manual_seed(5000 + K)."""
    g = torch.Generator(device="cuda").manual_seed(5000 + K)
    nb = K // 5
    H = K - nb
    grade = 0.05 * 4.0 ** (torch.arange(H, dtype=torch.float64) / max(H - 1, 1))
    X = torch.randn(K, d, generator=g, device="cuda")
    X[:H] *= grade.float().cuda()[:, None]
    if nb:
        X[H:] = 0.25 + 0.5 * X[H:]
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(5000 + K))
    g0 = 0.01 * torch.randn(d, generator=g, device="cuda")
    return X[perm.cuda()].contiguous(), g0


def operand(op, X):
    """The fp32 matrix X on the GPU as operand `op` of OPS (never written)."""
    import byzantine_aircomp_amd as bz
    if op == "rows4":
        return X.cuda()
    return bz.ClientPanels.from_rows(X.cuda(),
                                     dtype=torch.bfloat16 if op.startswith("bf16") else None)


def run(agg, w, g, n, tau=None):
    """(out, last_result) of n bodies on the streaming pass."""
    import byzantine_aircomp_amd as bz
    if agg == "cclip":
        out = bz.cclip(w, {"tau": tau, "clip_iters": n, "guess": g})
    else:
        opts = {"maxiter": n, "tol": -1.0, "guess": g, "algo": "stream"}
        if agg != "gm2":
            opts.update(noise_var=sc.GM_NOISE_VAR if agg == "gm_noise" else None, P_max=1,
                        seed=sc.GM_SEED)
        out = (bz.gm2 if agg == "gm2" else bz.gm)(w, opts)
    res = bz.aggregators.last_result
    assert res.algo == "stream" and res.iters == n, (agg, res)
    return out, res


def run_cases():
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    lines = []
    for K, d, ops in shapes(num_cu):
        X, g = device_input(K, d)
        tau = 0.1 * math.sqrt(d)              # between the honest rows' distances: some clip
        for op in ops:
            w = operand(op, X)
            for agg in AGGS:
                out, res = run(agg, w, g, N, tau)
                h = hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()
                lines.append(f"{K} {d} {op} {agg} {h} {res.iters} {float(res.last_movement).hex()}")
            del w
        del X
    return lines


if __name__ == "__main__":
    print("\n".join(run_cases()))
