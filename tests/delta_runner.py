"""Runs gm2 on fp32 panels for tests/test_gpu_delta.py.  GMAGG_DELTA is read once per process, so
the test starts this script once per knob value (1: the correction passes at any size, 0: never)
and compares what the two processes saved.

  python delta_runner.py cases OUT.npz   every shape of delta_cases.gpu_shapes: 3, 4 and 5 bodies
        (tol = -1) from delta_cases.guess_of, the run to delta_cases.conv_tol from the recipe's
        guess, and 3 bodies on stream_cases.tile_input at d = 4100 from its row-probe guess (next
        to row 0: the coefficients move by 0.5 and more per body).  Saved per run: the output, iterations, last movement, the correction
        mask and the shadow's status.
  python delta_runner.py shard OUT.json  one rank (RANK / WORLD_SIZE / MASTER_* set) of a
        d-sharded run over gloo on cuda:0: this rank's count, mask and movement.
"""
import json
import os
import sys

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import delta_cases as dc
import stream_cases as sc

REFUSAL_D = 4100
SHARD_K, SHARD_D = 1000, 4100


def _save(store, key, out, res):
    store[key + "/out"] = out.cpu().numpy()
    store[key + "/meta"] = np.array([res.iters, float(res.last_movement), res.corrections,
                                     res.correction_mask,
                                     {"off": 0, "armed": 1, "no_shadow": 2}[res.shadow]],
                                    dtype=np.float64)


def run_cases(path):
    import byzantine_aircomp_amd as bz
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    store = {}
    for K, d in dc.gpu_shapes(num_cu):
        X, g0 = dc.bench_input(K, d)
        P = bz.ClientPanels.from_rows(X.cuda())
        gw = dc.guess_of(K, d).cuda()
        for n in dc.NS:
            out = bz.gm2(P, {"maxiter": n, "tol": -1.0, "guess": gw, "algo": "stream"})
            _save(store, f"n{n}/{K}/{d}", out, bz.aggregators.last_result)
        out = bz.gm2(P, {"maxiter": 100, "tol": dc.conv_tol(d), "guess": g0.cuda(),
                         "algo": "stream"})
        _save(store, f"conv/{K}/{d}", out, bz.aggregators.last_result)
        del P
    for K in dc.KS:
        X = sc.tile_input(K, REFUSAL_D)[0]
        g0 = sc.probe_guess(X, 0)
        P = bz.ClientPanels.from_rows(X.cuda())
        out = bz.gm2(P, {"maxiter": 3, "tol": -1.0, "guess": g0.cuda(), "algo": "stream"})
        _save(store, f"refuse/{K}/{REFUSAL_D}", out, bz.aggregators.last_result)
        del P
    np.savez(path, **store)


def run_shard(path):
    import torch.distributed as dist

    import byzantine_aircomp_amd as bz
    from byzantine_aircomp_amd.sharded import ShardedGM
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    sg = ShardedGM(SHARD_D, device=torch.device("cuda", 0), transport="torch")
    X, g0 = dc.bench_input(SHARD_K, SHARD_D)
    P = bz.ClientPanels.from_rows(X[:, sg.lo:sg.hi].contiguous().cuda())
    sg.gm2(P, {"maxiter": 100, "tol": dc.conv_tol(SHARD_D), "guess": g0[sg.lo:sg.hi].cuda()})
    r = sg.last_result
    torch.cuda.synchronize()
    with open(path, "w") as f:
        json.dump({"rank": sg.rank, "lo": sg.lo, "hi": sg.hi, "iters": r.iters,
                   "mask": r.correction_mask, "corrections": r.corrections, "shadow": r.shadow,
                   "movement": float(r.last_movement).hex()}, f)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    {"cases": run_cases, "shard": run_shard}[sys.argv[1]](sys.argv[2])
