"""GPU: the fat edge tiling of the LDS-DMA fp64 GEMM (kernels.hip: dgemm_glds_fat_kernel, fat_edges) against numpy.matmul.
A ragged edge of 1..16 rows / columns of a product with A K-contiguous and B N-contiguous becomes a ninth row / column of
16 x 16 blocks of the neighbouring 128 x 128 tile (144 x 128, 128 x 144 and one 144 x 144 corner tile).  Covered: whole fat
tiles of every kind, the partial last k-tile with strips, k-cut fat tiles and their reduction, determinism, the route (one
launch of kernel class 1, `fat=` in the PYMES_GEMM_LOG line), the default rule (512 tiles, no explicit plan), remainder 17 and
the layouts that are never folded.  The bound is the one of tests/test_gpu_gemm_plans.py: err < 1e-13 sqrt(K) relative to
max(1, |ref|max).

The host simulator (tests/hostsim) has no such kernel and no launch planner: nothing of this runs without a GPU."""
import os

import numpy as np
import pytest

from pymes_amd.device import Context

pytestmark = pytest.mark.gpu

ALPHAS, BETAS = (1.0, -0.5, 2.0), (0.0, 1.0, 0.25)


class Product:
    """A [M][K], B [K][N], C0 [M][N] on host and device, A @ B computed once."""

    def __init__(self, ctx, M, N, K, seed):
        rng = np.random.default_rng(seed)
        self.ctx, self.M, self.N, self.K = ctx, M, N, K
        self.A, self.B, self.C0 = rng.standard_normal((M, K)), rng.standard_normal((K, N)), rng.standard_normal((M, N))
        self.AB = self.A @ self.B
        self.dA, self.dB, self.dC0 = ctx.array(self.A), ctx.array(self.B), ctx.array(self.C0)

    def ref(self, alpha, beta):
        return alpha * self.AB + beta * self.C0

    def err(self, got, alpha, beta):
        ref = self.ref(alpha, beta)
        return np.abs(got - ref).max() / max(1.0, np.abs(ref).max())

    def run(self, alpha, beta, fat, plan=None, cin=False, log=None):
        """One product; fat: "0" / "1" / None (PYMES_GEMM_FAT); cin: the beta term from another array than C.
        Returns (C, launches of kernel class 1, route lines)."""
        ctx, M, N, K = self.ctx, self.M, self.N, self.K
        dC = ctx.array(np.full((M, N), 7.0) if cin else self.C0)
        for name, val in (("PYMES_GEMM_FAT", fat), ("PYMES_GEMM_PLAN", plan), ("PYMES_GEMM_LOG", log)):
            if val is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = val
        try:
            ctx.prof_reset()
            ctx.dgemm(M, N, K, alpha, self.dA, K, 1, self.dB, N, 1, beta, dC, N, Cin=self.dC0 if cin else None)
            n1 = ctx.prof_query(kernel_class=1)["launches"]
            lines = []
            if log is not None:
                open(log, "w").close()
                ctx.prof_query()
                lines = [ln for ln in open(log).read().splitlines() if ln.startswith("M=")]
        finally:
            for name in ("PYMES_GEMM_FAT", "PYMES_GEMM_PLAN", "PYMES_GEMM_LOG"):
                os.environ.pop(name, None)
        got = dC.get()
        dC.free()
        return got, n1, lines

    def free(self):
        for x in (self.dA, self.dB, self.dC0):
            x.free()


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    c = Context(4, 4, workspace_bytes=1 << 28, lib=gpu_lib)
    c.prof_enable(True)          # (per-call events: what prof_query counts)
    yield c
    c.prof_enable(False)
    c.close()


def route(lines):
    assert len(lines) == 1, lines
    return lines[0].split(" ms=")[0]


# (M, N, K, the fat kinds expected in the route text)
WHOLE = [(2064, 2064, 800, "mn"), (2049, 2176, 800, "m"), (2176, 2060, 800, "n"),
         (2064, 2064, 806, "mn"), (2064, 2064, 794, "mn"), (2064, 2064, 402, "mn")]      # ... and partial last k-tiles: 6, 10, 2


@pytest.mark.parametrize("M,N,K,kinds", WHOLE)
def test_whole_fat_tiles(ctx, tmp_path, M, N, K, kinds):
    """256 (272, 256) tiles: the smallest grids that reach the LDS-DMA kernel on their own, every alpha / beta, the beta term
    in place and from another array.  The partial last k-tile with strips needs an even K (see test_odd_k below)."""
    p = Product(ctx, M, N, K, seed=M + 7 * N + 13 * K)
    log = str(tmp_path / "gemm.log")
    try:
        bound = 1e-13 * K ** 0.5
        for ia, alpha in enumerate(ALPHAS):
            for ib, beta in enumerate(BETAS):
                cin = beta != 0.0 and (ia + ib) % 2 == 1
                fat, n1, lines = p.run(alpha, beta, "1", cin=cin, log=log)
                what = dict(shape=(M, N, K), alpha=alpha, beta=beta, cin=cin)
                assert n1 == 1, what
                assert " fat=%s plan=" % kinds in route(lines), (what, lines)
                e = p.err(fat, alpha, beta)
                print("fat %s err %.3e (bound %.3e)" % (what, e, bound))
                assert e < bound, (what, e)
                if ia == ib:      # today's tiling on the same product: its own launch, values within the bound of the fat run
                    plain, n1, lines = p.run(alpha, beta, "0", cin=cin, log=log)
                    assert n1 == 1 and " fat=" not in route(lines), (what, lines)
                    d = np.abs(plain - fat).max() / max(1.0, np.abs(plain).max())
                    print("fat vs plain %.3e" % d)
                    assert d < bound, (what, d)
                    assert p.err(plain, alpha, beta) < bound
    finally:
        p.free()


@pytest.mark.parametrize("K", [805, 795])
def test_odd_k(ctx, tmp_path, K):
    """K = 805 / 795 on (2064, 2064): with an odd K the rows of a K-contiguous A are not 16-byte aligned, the product has no
    16-byte loads and never reaches the LDS-DMA kernel (describe_product: vec = 1) — so it is not folded either; the
    same route and bits as with PYMES_GEMM_FAT=0.  (The partial last k-tile of the fat kinds is run at K = 806 / 794 / 402.)"""
    p = Product(ctx, 2064, 2064, K, seed=K)
    log = str(tmp_path / "gemm.log")
    try:
        fat, n1, lines = p.run(-0.5, 0.25, "1", log=log)
        plain, n0, lines0 = p.run(-0.5, 0.25, "0", log=log)
        assert n1 == 0 and n0 == 0 and " fat=" not in route(lines) and route(lines) == route(lines0), (lines, lines0)
        assert np.array_equal(fat, plain)
        assert p.err(fat, -0.5, 0.25) < 1e-13 * K ** 0.5
    finally:
        p.free()


def test_remainder_17_is_not_folded(ctx, tmp_path):
    """2065 = 16 x 128 + 17: not a fat edge.  The same route text and the same bits with PYMES_GEMM_FAT=1, =0 and unset."""
    p = Product(ctx, 2065, 2048, 800, seed=17)
    log = str(tmp_path / "gemm.log")
    try:
        outs = [p.run(2.0, 0.25, fat, log=log) for fat in ("1", "0", None)]
        for got, n1, lines in outs:
            assert n1 == 1 and " fat=" not in route(lines), lines
            assert route(lines) == route(outs[1][2])
            assert np.array_equal(got, outs[1][0])
        assert p.err(outs[0][0], 2.0, 0.25) < 1e-13 * 800 ** 0.5
    finally:
        p.free()


def test_default_rule(ctx, tmp_path):
    """Unset, the fat tiling needs 512 tiles of today's tiling and no explicit plan: 17 x 33 = 561 tiles are folded to 16 x 32,
    17 x 17 = 289 are not, and PYMES_GEMM_PLAN keeps today's tiling and the meaning of its tile counts."""
    log = str(tmp_path / "gemm.log")
    p = Product(ctx, 2064, 4112, 400, seed=3)
    try:
        got, n1, lines = p.run(-0.5, 1.0, None, log=log)
        assert n1 == 1 and " fat=mn plan=512+0/1" in route(lines), lines
        e = p.err(got, -0.5, 1.0)
        print("default rule err %.3e" % e)
        assert e < 1e-13 * 400 ** 0.5
        got, n1, lines = p.run(-0.5, 1.0, None, plan="512,1", log=log)
        assert n1 == 1 and " fat=" not in route(lines) and route(lines).endswith("plan=561+0/1"), lines
        assert p.err(got, -0.5, 1.0) < 1e-13 * 400 ** 0.5
    finally:
        p.free()
    p = Product(ctx, 2064, 2064, 400, seed=4)
    try:
        got, n1, lines = p.run(1.0, 0.0, None, log=log)
        assert n1 == 1 and " fat=" not in route(lines), lines
        assert p.err(got, 1.0, 0.0) < 1e-13 * 400 ** 0.5
    finally:
        p.free()


def test_cut_fat_tiles_deep_k(ctx, tmp_path):
    """(272, 272, 49152): 2 x 2 tiles, one of every kind, all cut along K (the planner's own cut and forced ones; with
    PYMES_GEMM_FAT=1 an explicit plan counts the fat tiling's tiles)."""
    M = N = 272
    K = 49152
    p = Product(ctx, M, N, K, seed=272)
    log = str(tmp_path / "gemm.log")
    try:
        bound = 1e-13 * K ** 0.5
        for i, plan in enumerate((None, "0,2", "0,7", "0,64", "0,128")):
            alpha, beta = ALPHAS[i % 3], BETAS[(i + 1) % 3]
            got, n1, lines = p.run(alpha, beta, "1", plan=plan, cin=(i == 2), log=log)
            r = route(lines)
            assert n1 == 1 and " fat=mn plan=0+4/" in r, lines
            if plan is not None:
                assert r.endswith("plan=0+4/%s" % plan.split(",")[1]), lines
            e = p.err(got, alpha, beta)
            print("cut fat plan %s: %s err %.3e (bound %.3e)" % (plan, r.split("flops")[1], e, bound))
            assert e < bound, (plan, e)
        plain, n1, lines = p.run(1.0, 0.25, "0", log=log)
        fat, _, _ = p.run(1.0, 0.25, "1", log=log)
        assert n1 == 1 and " fat=" not in route(lines)
        assert np.abs(plain - fat).max() / max(1.0, np.abs(plain).max()) < bound
    finally:
        p.free()


# forced plans on the 16 x 16 fat tiles of (2064, 2064, 800): K allows two cuts.  The fat tiles are the last of the tile
# order — 225 plain ones, 15 fat in M, 15 fat in N, the corner —, so a tail of 16 is the fat column with the corner and the
# fat row stays whole; a tail of 32 holds every fat tile and one plain one; a tail of 8 cuts the fat column in two; half
# and all of the tiles cut; whole tiles only
FORCED = ["240,2", "224,2", "0,2", "128,2", "248,2", "256,1"]


def test_cut_fat_tiles_forced_plans_and_determinism(ctx, tmp_path):
    p = Product(ctx, 2064, 2064, 800, seed=99)
    log = str(tmp_path / "gemm.log")
    try:
        bound = 1e-13 * 800 ** 0.5
        for i, plan in enumerate(FORCED):
            alpha, beta = ALPHAS[(i + 1) % 3], BETAS[i % 3]
            whole, cuts = (int(x) for x in plan.split(","))
            got, n1, lines = p.run(alpha, beta, "1", plan=plan, cin=(i == 1), log=log)
            assert n1 == 1 and route(lines).endswith(" fat=mn plan=%d+%d/%d" % (whole, 256 - whole, cuts)), lines
            e = p.err(got, alpha, beta)
            print("forced plan %s err %.3e (bound %.3e)" % (plan, e, bound))
            assert e < bound, (plan, e)
        # a mixed whole + cut fat launch gives the same bits every time (fixed summation order of the cuts)
        outs = [p.run(1.0, 1.0, "1", plan="240,2")[0] for _ in range(3)]
        assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    finally:
        p.free()


def test_other_layouts_and_batches_are_not_folded(ctx, tmp_path):
    """(650, 520, 1000) x 3 = 5 x 128 + 10, 4 x 128 + 8: ragged by less than 16 both ways.  The three other layouts have no
    fat kinds and the batched product runs on 64 x 64 tiles: PYMES_GEMM_FAT=1 changes no bit of any of them."""
    rng = np.random.default_rng(5)
    log = str(tmp_path / "gemm.log")
    # ... and the three other layouts at a shape that IS folded in the fourth: they stay on their own LDS-DMA kernels
    cases = [(650, 520, 1000, 3, a, b) for a, b in ((False, False), (False, True), (True, True), (True, False))]
    cases += [(2064, 2064, 800, 1, a, b) for a, b in ((False, False), (False, True), (True, True))]
    for M, N, K, nb, a_kc, b_kc in cases:
        A = rng.standard_normal((nb, M, K) if a_kc else (nb, K, M))
        B = rng.standard_normal((nb, N, K) if b_kc else (nb, K, N))
        C0 = rng.standard_normal((nb, M, N))
        ref = np.matmul(A if a_kc else A.transpose(0, 2, 1), B.transpose(0, 2, 1) if b_kc else B) + C0
        dA, dB = ctx.array(A), ctx.array(B)
        outs = []
        for fat in ("1", "0"):
            dC = ctx.array(C0)
            os.environ["PYMES_GEMM_FAT"] = fat
            os.environ["PYMES_GEMM_LOG"] = log
            try:
                open(log, "w").close()
                ctx.prof_reset()
                ctx.contract("%s,%s->zmn" % ("zmk" if a_kc else "zkm", "znk" if b_kc else "zkn"), dA, dB, out=dC, alpha=1.0,
                             beta=1.0, batch="z")
                ctx.prof_query()
            finally:
                os.environ.pop("PYMES_GEMM_FAT", None)
                os.environ.pop("PYMES_GEMM_LOG", None)
            assert " fat=" not in open(log).read()
            outs.append(dC.get())
            dC.free()
        assert np.array_equal(outs[0], outs[1]), (a_kc, b_kc)
        assert np.abs(outs[0] - ref).max() / max(1.0, np.abs(ref).max()) < 1e-13 * K ** 0.5, (a_kc, b_kc)
        dA.free()
        dB.free()
