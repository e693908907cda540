"""Which launch form every product of a fixed, seeded list takes, and the bits it produces: the text to diff between two
builds of the library (PYMES_AMD_LIBRARY selects the build; tools/ab_eom.sh says how to build a commit into _ab/).

    python tools/gemm_route_dump.py > new.txt
    PYMES_AMD_LIBRARY=$PWD/_ab/pymes_amd/lib/libpymes_amd.so python tools/gemm_route_dump.py > old.txt && diff old.txt new.txt

The list goes through ctx.dgemm / ctx.contract in four set-ups: (a) per-call profiling on (no phases, every product a launch
of its own), (b) PYMES_PHASE=0 inside ctx.gemm_group(), (c) one ctx.phase_hold() with PYMES_PHASE_LOG=1 and
PYMES_PHASE_MAX_US=1000, (d) the default path.  Per product: the route text (the PYMES_GEMM_LOG line without its time, the
group line, or the [phase] lines of the hold) and the sha256 of the output array.  Nothing printed depends on time, so two
builds that plan alike and sum in the same order print the same text.  Exits 1 when a launch form listed in COVERAGE is
missing from the dump."""
import hashlib
import os
import re
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pymes_amd.device import Context      # noqa: E402


def P(M, N, K, akc=True, bkc=False, alpha=1.0, beta=0.0, pa=0, pb=0, pc=0, nb=1):
    """One product: A K-contiguous (akc) or M-contiguous, B likewise; pa / pb / pc: doubles added to the pitch of A / B / C."""
    return dict(M=M, N=N, K=K, akc=akc, bkc=bkc, alpha=alpha, beta=beta, pa=pa, pb=pb, pc=pc, nb=nb)


# (a) and (d): launches of their own
OWN = [
    P(2048, 2048, 400),                                    # 256 whole tiles of the LDS-DMA kernel
    P(2176, 2048, 800, akc=False, beta=1.0),               # 256 whole + 16 cut
    P(256, 256, 49152, bkc=True, beta=0.25),               # 4 tiles over a huge K
    P(2048, 2048, 128, akc=False),                         # 128 x 128, register-staged (K below the LDS-DMA depth)
    P(32768, 64, 272), P(64, 32768, 272, akc=False, bkc=True, beta=1.0),        # 128 x 64, 64 x 128
    P(320, 320, 2048, beta=1.0),                           # 64 x 64, all tiles cut
    P(321, 323, 2048, akc=False, pa=1, pb=1, pc=1, beta=0.25),                  # odd M, N on even pitches: Mc / Nc, vec=2
    P(321, 323, 2048, akc=False, alpha=-0.5),              # odd pitches: vec=1
    # the shapes of tests/test_gpu_gemm_plans.py SHAPES: under 256 tiles and not deep enough to cut, so 64 x 64 tiles
    P(1250, 1100, 900, bkc=True, alpha=2.0, beta=1.0), P(384, 640, 2000), P(777, 300, 1601, akc=False), P(129, 129, 4100, beta=1.0),
    P(2000, 1600, 400, akc=False, bkc=True),
    P(512, 4096, 128), P(4096, 24, 128, akc=False), P(24, 4096, 100, bkc=True, beta=1.0),      # streaming shapes
    P(4096, 24, 2048, beta=0.25), P(24, 4096, 2048, akc=False, bkc=True), P(4097, 23, 2047, akc=False),        # narrow tiles
    P(1, 6400, 4096), P(1, 6400, 4096, bkc=True, beta=1.0), P(4096, 1, 4096), P(4096, 1, 4096, akc=False, beta=0.25),
    P(1, 6401, 4095, pb=0), P(650, 520, 1000, nb=3, beta=1.0), P(650, 520, 1000, akc=False, bkc=True, nb=3),
]
# (b): inside a group, phases off
GROUP = [
    P(512, 512, 3072), P(640, 384, 1536, beta=1.0), P(513, 511, 3072, pb=1, beta=0.25),      # the LDS-DMA half
    P(40, 48, 320), P(65, 33, 200, akc=False, beta=1.0), P(65, 33, 200, bkc=True, pc=3), P(41, 47, 321, akc=False, bkc=True, alpha=-0.5),
    P(320, 320, 2048, beta=1.0), P(100, 60, 24, nb=4),
]
# (c): tasks of one held phase
PHASE_KSPLIT, PHASE_TAIL = P(64, 6400, 2560), P(2112, 2112, 256, akc=False, beta=1.0)
PHASE = [
    PHASE_KSPLIT, PHASE_TAIL, P(40, 48, 320, beta=0.25), P(65, 33, 200, akc=False, bkc=True), P(41, 47, 321, akc=False, pa=1, pb=1),
    P(24, 300, 700, bkc=True), P(300, 24, 700, beta=1.0), P(1, 6400, 4096), P(4096, 1, 4096, beta=1.0), P(100, 60, 24, nb=4),
]


def prepare(ctx, rng, p):
    """Operands of the product on the device (uploads synchronise: they come before a group or a hold is opened); returns
    (label, call that issues the product, output array, operands to free later)."""
    M, N, K, nb = p["M"], p["N"], p["K"], p["nb"]
    label = "M=%d N=%d K=%d nb=%d akc=%d bkc=%d alpha=%g beta=%g pad=%d,%d,%d" % (
        M, N, K, nb, p["akc"], p["bkc"], p["alpha"], p["beta"], p["pa"], p["pb"], p["pc"])
    if nb > 1:
        A = ctx.array(rng.random((nb, M, K) if p["akc"] else (nb, K, M)) - 0.5)
        B = ctx.array(rng.random((nb, N, K) if p["bkc"] else (nb, K, N)) - 0.5)
        Cm = ctx.array(rng.random((nb, M, N)) - 0.5)
        spec = "%s,%s->zmn" % ("zmk" if p["akc"] else "zkm", "znk" if p["bkc"] else "zkn")
        return label, lambda: ctx.contract(spec, A, B, out=Cm, alpha=p["alpha"], beta=p["beta"], batch="z"), Cm, (A, B)
    lda = (K if p["akc"] else M) + p["pa"]
    ldb = (K if p["bkc"] else N) + p["pb"]
    ldc = N + p["pc"]
    A = ctx.array(rng.random((M if p["akc"] else K, lda)) - 0.5)
    B = ctx.array(rng.random((N if p["bkc"] else K, ldb)) - 0.5)
    Cm = ctx.array(rng.random((M, ldc)) - 0.5)
    a_sm, a_sk = (lda, 1) if p["akc"] else (1, lda)
    b_sk, b_sn = (1, ldb) if p["bkc"] else (ldb, 1)
    return label, lambda: ctx.dgemm(M, N, K, p["alpha"], A, a_sm, a_sk, B, b_sk, b_sn, p["beta"], Cm, ldc), Cm, (A, B)


def run(ctx, rng, p):
    r = prepare(ctx, rng, p)
    r[1]()
    return r


def sha(arr):
    return hashlib.sha256(arr.get().tobytes()).hexdigest()


def finish(out, results):
    for label, _, Cm, ops in results:
        out.append("  %s sha256=%s" % (label, sha(Cm)))
        for x in (Cm,) + ops:
            x.free()


def new_log_lines(path, seen):
    with open(path) as f:
        lines = [re.sub(r" ms=[0-9.eE+-]+$", "", ln.rstrip("\n")) for ln in f]
    return [ln for ln in lines[seen:] if ln != "----"], len(lines)


def set_phase_env(ctx, **env):
    for k in ("PYMES_PHASE", "PYMES_PHASE_LOG", "PYMES_PHASE_MAX_US"):
        os.environ.pop(k, None)
    os.environ.update(env)
    ctx.phase_enable(-1)        # the environment is read again at the next operation


def dump():
    out = []
    tmp = tempfile.mkdtemp()
    log = os.path.join(tmp, "gemm.log")
    open(log, "w").close()
    os.environ["PYMES_GEMM_LOG"] = log
    os.environ.pop("PYMES_GEMM_PLAN", None)
    ctx = Context(6, 20, workspace_bytes=1 << 28)
    rng = np.random.default_rng(20240229)
    seen = 0
    try:
        out.append("== (a) per-call profiling")
        set_phase_env(ctx)
        ctx.prof_enable(True)
        for p in OWN:
            ctx.prof_reset()
            r = run(ctx, rng, p)
            ctx.prof_query(0)
            lines, seen = new_log_lines(log, seen)
            out.extend("  route: " + ln for ln in lines)
            finish(out, [r])
        # the beta term read from another array than the output (Cin != C): the one-index dressings of the integral blocks
        n = ctx.no + ctx.nv
        ctx.set_V_pqrs(rng.random((n, n, n, n)) - 0.5)
        t1 = ctx.array(rng.random((ctx.nv, ctx.no)) - 0.5)
        names = ["abij", "aibj", "abci", "ijka"]
        ctx.prof_reset()
        ctx.dress_V(t1, names)
        ctx.prof_query(0)
        lines, seen = new_log_lines(log, seen)
        out.append("  dress_V (Cin != C in the first transform of every block): %d products" % len(lines))
        out.extend("  route: " + ln for ln in lines)
        for nm in names:
            out.append("  dressed %s sha256=%s" % (nm, sha(ctx.V_block(nm, dressed=True))))
        t1.free()

        out.append("== (b) PYMES_PHASE=0 inside a group")
        set_phase_env(ctx, PYMES_PHASE="0")
        ctx.prof_reset()
        results = [prepare(ctx, rng, p) for p in GROUP]
        with ctx.gemm_group() as g:
            for r in results:
                r[1]()
        ctx.prof_query(0)
        lines, seen = new_log_lines(log, seen)
        out.extend("  route: " + ln for ln in lines)
        out.append("  group launches=%d products=%d" % (g.launches, g.products))
        finish(out, results)
        ctx.prof_enable(False)

        out.append("== (c) one held phase")
        set_phase_env(ctx, PYMES_PHASE="1", PYMES_PHASE_LOG="1", PYMES_PHASE_MAX_US="1000")
        errlog = os.path.join(tmp, "phase.log")
        sys.stderr.flush()
        saved = os.dup(2)
        fd = os.open(errlog, os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
        os.dup2(fd, 2)
        results = [prepare(ctx, rng, p) for p in PHASE]
        try:
            with ctx.phase_hold():
                for r in results:
                    r[1]()
            ctx.sync()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            os.close(fd)
        with open(errlog) as f:
            out.extend("  route: " + ln.rstrip() for ln in f if ln.startswith("[phase]"))
        out.append("  phase_stats %s" % sorted(ctx.phase_stats().items()))
        finish(out, results)

        out.append("== (d) default path")
        set_phase_env(ctx)
        for p in OWN + GROUP:
            finish(out, [run(ctx, rng, p)])
        out.append("  phase_stats %s" % sorted(ctx.phase_stats().items()))
    finally:
        ctx.close()
    return out


def blocks_of(p, bm, bn):
    return -(-p["M"] // bm) * -(-p["N"] // bn) * p["nb"]


# (what, a pattern that some line of the dump must match)
COVERAGE = [("tile=%s" % t, r"tile=%s " % t) for t in ("128x128", "128x64", "64x128", "64x64", "64x64s", "64x32s?", "32x64s?")] + [
    ("vec=1", r"tile=.* vec=1 "), ("vec=2", r"tile=.* vec=2 "),
    ("LDS-DMA, whole tiles only", r"dma=1 .*plan=\d+\+0/1$"),
    ("LDS-DMA with a cut tail", r"dma=1 split=-\d+ .*plan=\d+\+[1-9]\d*/([2-9]|\d\d)$"),
    ("register-staged launch with a cut tail", r"dma=0 split=-\d+ "),
    ("LDS-DMA group with a k-split member", r"route: LDS-DMA group of \d+ products, \d+ blocks, [1-9]\d* k-split"),
    ("64 x 64 group with a k-split member", r"route: group of \d+ products, \d+ blocks, [1-9]\d* k-split"),
    ("gemv=cols", r"gemv=cols"), ("gemv=rows", r"gemv=rows"),
    ("batched product", r"batch=([2-9]|\d\d+) tile="),
    ("beta = 0", r"beta=0 pad"), ("beta = 1", r"beta=1 pad"), ("beta term from another array", r"dress_V \(Cin != C.*: [1-9]\d* products"),
    # all 100 tiles of PHASE_KSPLIT cut 10 ways, reduced one level later
    ("phase: gemm task and its splitk task", r"\[phase\]\s+L\d+ .*\bgemm:%d:" % (blocks_of(PHASE_KSPLIT, 64, 64) * 10)),
    ("phase: splitk task", r"\[phase\]\s+L\d+ .*\bsplitk:%d:" % (blocks_of(PHASE_KSPLIT, 64, 64) * 16)),
    # PHASE_TAIL: 1089 tiles = one round of 1024 + 65 cut in two
    ("phase: main part", r"\[phase\]\s+L\d+ .*\bgemm:1024:"),
    ("phase: tail part", r"\[phase\]\s+L\d+ .*\bgemm:%d:" % ((blocks_of(PHASE_TAIL, 64, 64) - 1024) * 2)),
]


def main():
    out = dump()
    print("\n".join(out))
    missing = [what for what, pat in COVERAGE if not any(re.search(pat, ln) for ln in out)]
    for what in missing:
        print("coverage: no line for: " + what, file=sys.stderr)
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main())
