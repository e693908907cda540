#!/usr/bin/env python3
"""GPU probe: the per-rank integral footprint of integral sharding (include/pymes_amd.h, pymes_set_integral_shard) at
(50,200).  A stubbed rank 0 of N in {2, 4, 8} (pymes_amd/dist.py, stub: collectives are no-ops, energies meaningless) runs
CCSD with the integrals formed on the device from the factors, replicated and sharded, and prints per configuration the
integral bytes the context holds (pymes_integral_bytes), the device memory in use at its peak (free-memory samples after
the integrals, after set-up and after the timed passes) and the time per iteration.
    python3 tools/probe_shard_memory.py [--steps K] [--worlds 2,4,8]"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from oracle.io_oracle import synthetic_factors  # noqa: E402
from pymes_amd import dist as pdist  # noqa: E402
from pymes_amd.integral.device import DeviceIntegrals  # noqa: E402
from pymes_amd.solver.ccsd import CCSD  # noqa: E402


def one(no, nv, B, f, world, shard, steps):
    pdist.stub(0, world)
    try:
        t0 = time.perf_counter()
        ints = DeviceIntegrals.from_factors(no, B, shard=(0, world) if shard else None, device=0)
        ints.ctx.sync()
        t_ints = time.perf_counter() - t0
        used = []

        def sample():
            free, total = ints.ctx.mem_info()
            used.append(total - free)
        try:
            sample()
            s = CCSD(no, device=0, shard_integrals=shard)
            with contextlib.redirect_stdout(io.StringIO()):
                st = s.setup(f, ints)
                s.iterate(st)                 # warm-up pass (static packs, staging buffers)
                ints.ctx.sync()
                sample()
                t0 = time.perf_counter()
                for _ in range(steps):
                    s.iterate(st)
                ints.ctx.sync()
                ms = (time.perf_counter() - t0) / steps * 1e3
            sample()
            return {"world": world, "mode": "sharded" if shard else "replicated", "integral_bytes": ints.ctx.integral_bytes(),
                    "device_peak_bytes": max(used), "ms_per_iteration": round(ms, 3),
                    "integrals_seconds": round(t_ints, 3)}
        finally:
            ints.ctx.close()
    finally:
        pdist._STUB = None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no", type=int, default=50)
    ap.add_argument("--nv", type=int, default=200)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--worlds", default="2,4,8")
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)       # torch's HIP runtime first (the stubbed path allocates its exchange buffers with torch)
    B, eps = synthetic_factors(args.no, args.nv, seed=0)
    f = np.diag(eps)
    rows = []
    for world in [int(x) for x in args.worlds.split(",")]:
        for shard in (False, True):
            r = one(args.no, args.nv, B, f, world, shard, args.steps)
            r.update(no=args.no, nv=args.nv)
            rows.append(r)
            print(json.dumps(r), flush=True)
    print("%6s %11s %14s %14s %10s" % ("N", "mode", "integral GB", "device peak GB", "ms/iter"))
    for r in rows:
        print("%6d %11s %14.2f %14.2f %10.2f" % (r["world"], r["mode"], r["integral_bytes"] / 1e9,
                                                r["device_peak_bytes"] / 1e9, r["ms_per_iteration"]))


if __name__ == "__main__":
    main()
