"""Hit fraction of the frontier label cache (dm_frontier_cache_stats) on the
bench's C3 sequence: the same batches in the same order as `bench.py`
(synth.c3_pool, bench origin, default parameters), one synchronous frontier
pass per batch -- a pass's hits depend on the map states only, not on how the
passes are pipelined.  Prints hits / misses per pass and the totals over the
passes after the warm-up.
  python tools/frontier_cache_probe.py [--pool 6] [--steps 60] [--warmup 20]"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "distributed-autonomous-exploration-and-mapping_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dm  # noqa: E402
from dm import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pool", type=int, default=6)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    G, res, S, N = 16384, 0.05, 64, 4096
    half = G * res / 2
    _, _, pool = synth.c3_pool(0, G, S, N, a.pool, 1, 0, res)
    dev = torch.device("cuda", 0)
    dpool = [(torch.from_numpy(synth.pose4(p)).to(dev), torch.from_numpy(np.ascontiguousarray(r)).to(dev))
             for p, r in pool]
    torch.cuda.synchronize()
    amin, inc = float(synth.LD06_ANGLE_MIN), float(synth.ld06_angle_increment(N))
    p = dm.default_params(G, G, resolution=res)
    p.origin_x = p.origin_y = -half
    th = tm = 0
    with dm.OccupancyMapper(p) as m:
        for k in range(a.warmup + a.steps):
            p4, r = dpool[k % len(dpool)]
            m.integrate_device(p4.data_ptr(), p4.shape[0], r.data_ptr(), N, amin, inc)
            fr = m.frontiers()
            h, ms = m.frontier_cache_stats()
            print(f"pass {k:3d}: hits {h:5d} misses {ms:5d} clusters {len(fr.clusters)}")
            if k >= a.warmup:
                th += h
                tm += ms
    print(f"pool {a.pool}: passes {a.warmup}..{a.warmup + a.steps - 1}: hits {th} misses {tm} "
          f"hit fraction {th / max(1, th + tm):.4f}")


if __name__ == "__main__":
    main()
