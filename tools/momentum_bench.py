"""The worker-momentum loop (training.MomentumSGD) and its client kernel on the GPU, on the
MNIST shape F = 784, C = 10, B = 50 with synthetic MNIST-shaped data (no dataset here).

  1. gm_client_grads_f32 (client_grads.hip, one workgroup per client) at K = 50 and K = 1000
     against gm_client_chain_f32 (clients.hip, one workgroup walks the K clients) at K = 50:
     the kernels alternate in one process, each launch between two HIP events, the figure is
     the median of --reps launches.
  2. the per-step time of training.MomentumSGD against training.SGD (K = 50: 45 honest + 5
     classflip) with gm2 and with cclip.with_options(tau=...).

    python tools/momentum_bench.py [--reps 20] [--steps 200] [--out profiles/momentum.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.loop_bench import synthetic_mnist  # noqa: E402

F, C, B = 784, 10, 50


def kernel_times(reps):
    import byzantine_aircomp_amd as bz
    from byzantine_aircomp_amd import _lib
    ctx = bz.context()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    n, d = 60000, C * F + C
    x = (0.3 * torch.randn(n, F, generator=g)).to(dev)
    y = torch.randint(0, C, (n,), generator=g).to(dev)
    W0 = (0.05 * torch.randn(C, F, generator=g)).to(dev)
    b0 = torch.full((C,), 0.01, device=dev)
    W, b = W0.clone(), b0.clone()
    stream = torch.cuda.current_stream().cuda_stream
    runs = {}
    for name, K in (("chain", 50), ("grads", 50), ("grads", 1000)):
        idx = torch.randint(0, n, (K, B), generator=g, dtype=torch.int32).to(dev)
        X = torch.zeros(K, d, device=dev)
        if name == "chain":
            def launch(idx=idx, X=X, K=K):
                _lib.check(ctx.lib.gm_client_chain_f32(
                    ctx.handle, x.data_ptr(), F, y.data_ptr(), F, C, idx.data_ptr(), K, B, K - 5,
                    1, 1e-2, 1e-3, W.data_ptr(), b.data_ptr(), X.data_ptr(), d,
                    _lib.GM_LAYOUT_ROWS, stream), "chain")
        else:
            def launch(idx=idx, X=X, K=K):
                _lib.check(ctx.lib.gm_client_grads_f32(
                    ctx.handle, x.data_ptr(), F, y.data_ptr(), F, C, idx.data_ptr(), K, B,
                    K - K // 10, 1, 0.9, 1e-3, W.data_ptr(), b.data_ptr(), X.data_ptr(), d,
                    _lib.GM_LAYOUT_ROWS, stream), "grads")
        runs[(name, K)] = (launch, [])
    for rep in range(reps + 3):                       # 3 warm-up rounds, untimed
        for key, (launch, ms) in runs.items():
            W.copy_(W0)                               # (the chain steps the model in place)
            b.copy_(b0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch()
            e1.record()
            e1.synchronize()
            if rep >= 3:
                ms.append(e0.elapsed_time(e1))
    chain = statistics.median(runs[("chain", 50)][1])
    lines = []
    for (name, K), (_, ms) in runs.items():
        med = statistics.median(ms)
        lines.append({"what": "client kernel, HIP events, alternating in one process",
                      "kernel": "gm_client_chain_f32" if name == "chain" else "gm_client_grads_f32",
                      "K": K, "F": F, "C": C, "B": B, "reps": reps, "median_us": round(1e3 * med, 1),
                      "min_us": round(1e3 * min(ms), 1), "max_us": round(1e3 * max(ms), 1),
                      "chain_K50_over_this": round(chain / med, 2)})
    return lines


def loop_times(steps):
    import byzantine_aircomp_amd as bz
    from byzantine_aircomp_amd import training as T
    dev = torch.device("cuda", 0)
    tr = torch.utils.data.TensorDataset(*synthetic_mnist(601, 5000))
    va = torch.utils.data.TensorDataset(*synthetic_mnist(602, 500))
    lines = []
    for agg_name, agg in (("gm2", bz.gm2), ("cclip(tau=1)", bz.cclip.with_options(tau=1.0))):
        for loop in (T.SGD, T.MomentumSGD):
            for n_steps in (3, steps):                # the first run warms up, untimed
                model = T.modelFactory(SEED=2021).to(dev)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                loop(model, gamma=1e-2, aggregate=agg, weight_decay=1e-3, honestSize=45,
                     byzantineSize=5, attack=T.classflip, rounds=1, displayInterval=n_steps,
                     SEED=2021, fixSeed=True, loss_func=torch.nn.CrossEntropyLoss(),
                     train_dataset=tr, validate_dataset=va, device=dev, batchSize=50,
                     verbose=False, eval_train=False, client_kernel=True)
                torch.cuda.synchronize(dev)
                total = time.perf_counter() - t0
            lines.append({"what": "training step (K=50: 45 honest + 5 classflip, MLP d=7850, rows)",
                          "loop": loop.__name__, "agg": agg_name, "steps": steps,
                          "ms_per_step": round(1e3 * total / steps, 3),
                          "note": "includes two validation passes (500 samples) per run"})
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = kernel_times(a.reps) + loop_times(a.steps)
    for line in lines:
        print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
