#!/usr/bin/env python3
"""GPU probe of the factor-direct particle ladder (include/pymes_amd.h, pymes_set_integral_direct).  Prints one JSON line and
writes a text file under profiles/direct/:
  iter      integral bytes (pymes_integral_bytes) of a stored and a factor-direct context at (no, nv) and the time of a CCSD
            iteration on each, the two alternating in one process after a warm-up;
  builders  the row builders on ALL pair rows of (nv, naux): the gemm route and the fused kernel of two factor-direct contexts,
            alternating, host-timed with a synchronisation per chunk; --builder factors|gemm|fused runs one of the three alone
            (dev::ladder_pack_V_factors through a one-rank integral shard), for a kernel trace of its own;
  big       one CCSD iteration on a factor-direct context of a shape whose stored form does not fit the device, with the
            device memory in use afterwards (pymes_mem_info).
    python3 tools/probe_direct.py [--part iter,builders] [--no 50] [--nv 200] [--naux 500] [--steps 5] [--reps 5]"""
import argparse
import contextlib
import ctypes as C
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from oracle.io_oracle import synthetic_factors  # noqa: E402
from pymes_amd.device import Context  # noqa: E402
from pymes_amd.integral.device import DeviceIntegrals  # noqa: E402
from pymes_amd.solver.ccsd import CCSD  # noqa: E402


def used_bytes(ctx):
    free, total = ctx.mem_info()
    return total - free


def part_iter(no, nv, steps):
    B, eps = synthetic_factors(no, nv, seed=0)
    f = np.diag(eps)
    runs = {}
    for mode in ("stored", "direct"):
        ints = DeviceIntegrals.from_factors(no, B, direct=True if mode == "direct" else None, device=0)
        s = CCSD(no, device=0)
        with contextlib.redirect_stdout(io.StringIO()):
            st = s.setup(f, ints)
            for _ in range(2):               # warm-up: static packs, staging buffers, the launch graph
                s.iterate(st)
        ints.ctx.sync()
        runs[mode] = (ints, s, st, [])
    with contextlib.redirect_stdout(io.StringIO()):
        for _ in range(steps):
            for mode in ("stored", "direct"):
                ints, s, st, ms = runs[mode]
                t0 = time.perf_counter()
                s.iterate(st)
                ints.ctx.sync()
                ms.append((time.perf_counter() - t0) * 1e3)
    out = {"no": no, "nv": nv, "naux": int(B.shape[0])}
    for mode, (ints, s, st, ms) in runs.items():
        out[mode] = {"integral_bytes": ints.ctx.integral_bytes(), "ms_per_iteration": [round(x, 3) for x in ms],
                     "median_ms": round(statistics.median(ms), 3)}
        if mode == "direct":
            out[mode]["info"] = ints.ctx.direct_info()
    out["device_used_bytes_both"] = used_bytes(runs["direct"][0].ctx)
    for ints, _, _, _ in runs.values():
        ints.ctx.close()
    out["direct_minus_stored_ms"] = round(out["direct"]["median_ms"] - out["stored"]["median_ms"], 3)
    return out


def build_all(ctx, cap, npp):
    """Every pair row once, chunk by chunk (pymes_direct_rows synchronises after each chunk); seconds."""
    vp, vm, ldp, ldm = C.c_void_p(), C.c_void_p(), C.c_int64(), C.c_int64()
    t0 = time.perf_counter()
    for c0 in range(0, npp, cap):
        ctx.lib.call("pymes_direct_rows", ctx.handle, c0, min(npp, c0 + cap), C.byref(vp), C.byref(vm), C.byref(ldp), C.byref(ldm))
    return time.perf_counter() - t0


def part_builders(nv, naux, reps, which):
    no = 2
    n = no + nv
    B = np.random.default_rng(0).standard_normal((naux, n, n)) * 0.05
    B = 0.5 * (B + B.transpose(0, 2, 1))
    npp = nv * (nv + 1) // 2
    flops = 2.0 * npp * nv * nv * naux
    out = {"nv": nv, "naux": naux, "rows": npp, "flops_per_build": flops, "which": which}
    if which == "factors":           # dev::ladder_pack_V_factors: once per set_V_from_factors of a one-rank integral shard
        for _ in range(reps):
            ctx = Context(no, nv, device=0, shard=(0, 1))
            ctx.set_V_from_factors(B)
            ctx.sync()
            ctx.close()
        return out
    ctxs = {}
    for b in (("gemm", "fused") if which == "alternate" else (which,)):
        os.environ["PYMES_DIRECT_BUILDER"] = b
        ctxs[b] = Context(no, nv, device=0, direct=True)
        ctxs[b].set_V_from_factors(B)
        out[b] = {"chunk_rows": ctxs[b].direct_info()["chunk_rows"], "ms": []}
    os.environ.pop("PYMES_DIRECT_BUILDER", None)
    for b, ctx in ctxs.items():
        build_all(ctx, out[b]["chunk_rows"], npp)          # warm-up
    for _ in range(reps):
        for b, ctx in ctxs.items():
            out[b]["ms"].append(round(build_all(ctx, out[b]["chunk_rows"], npp) * 1e3, 3))
    for b, ctx in ctxs.items():
        out[b]["tflops"] = [round(flops / (ms * 1e-3) / 1e12, 2) for ms in out[b]["ms"]]
        ctx.close()
    if which == "alternate":
        out["every_fused_run_below_every_gemm_run"] = max(out["fused"]["ms"]) < min(out["gemm"]["ms"])
    return out


def part_big(no, nv):
    B, eps = synthetic_factors(no, nv, seed=0)
    f = np.diag(eps)
    n = no + nv
    pitch = lambda x: (x + 15) // 16 * 16                                               # noqa: E731
    npp = nv * (nv + 1) // 2
    out = {"no": no, "nv": nv, "naux": int(B.shape[0]),
           "stored_arithmetic_bytes": 8 * n ** 4 + 8 * npp * (pitch(npp) + pitch(npp - nv))}
    t0 = time.perf_counter()
    ints = DeviceIntegrals.from_factors(no, B, direct=True, device=0)
    ints.ctx.sync()
    out["integrals_seconds"] = round(time.perf_counter() - t0, 2)
    try:
        out["integral_bytes_after_setup"] = ints.ctx.integral_bytes()
        s = CCSD(no, device=0)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            st = s.setup(f, ints)
            t0 = time.perf_counter()
            s.iterate(st)
            ints.ctx.sync()
        out["first_iteration_seconds"] = round(time.perf_counter() - t0, 2)
        out["integral_bytes"] = ints.ctx.integral_bytes()
        out["device_used_bytes"] = used_bytes(ints.ctx)
        out["info"] = ints.ctx.direct_info()
    finally:
        ints.ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="iter,builders")
    ap.add_argument("--no", type=int, default=50)
    ap.add_argument("--nv", type=int, default=200)
    ap.add_argument("--naux", type=int, default=500)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--builder", default="alternate", choices=["alternate", "factors", "gemm", "fused"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "direct", "probe_direct.txt"))
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    res = {}
    for part in args.part.split(","):
        if part == "iter":
            res["iter"] = part_iter(args.no, args.nv, args.steps)
        elif part == "builders":
            res["builders"] = part_builders(args.nv, args.naux, args.reps, args.builder)
        elif part == "big":
            res["big"] = part_big(args.no, args.nv)
        else:
            raise SystemExit("unknown part %r" % part)
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("tools/probe_direct.py %s\n" % " ".join(sys.argv[1:]))
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
