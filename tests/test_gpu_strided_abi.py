"""GPU: the kernels behind the stride arguments of the C-ABI.  The seeded strided / offset / stride-0 / batch-label cases of
tests/_strided_views.py (host-planner twin: tests/test_strided_abi.py) through pymes_contract and pymes_permute with phase
launches on, off and inside open groups of products; fixed larger products whose 16-byte-load and LDS-DMA eligibility
(describe_product, gemv_dispatch in csrc/kernels.hip) hangs on the alignment of a base pointer, a pitch or a batch stride;
fixed permutations for each path of dev::permute; the integral setters from strided device views."""
import numpy as np
import pytest

from pymes_amd.device import Context
from tests import _strided_views as sv

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ["env", "nophase", "group"])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_strided_contractions_gpu(gpu_lib, seed, mode):
    sv.check_strided_contractions(gpu_lib, seed, 120, mode=mode)


@pytest.mark.parametrize("mode", ["env", "nophase"])
@pytest.mark.parametrize("seed", [0, 1])
def test_strided_permutations_gpu(gpu_lib, seed, mode):
    worst = sv.check_strided_permutations(gpu_lib, seed, mode=mode)
    print(f"strided permutations seed {seed} mode {mode}: worst err/bound {worst:.3g}")


def test_strided_integrals_gpu(gpu_lib):
    sv.check_strided_integrals(gpu_lib)


def test_lds_dma_eligibility_follows_alignment(gpu_lib):
    """(2176, 2048, 800) of tests/test_gpu_gemm_plans.py as column slices of wider bases: the LDS-DMA kernel takes the product
    when A starts at an even element offset on an even pitch, and does not when the base is moved by one element or the
    pitch is odd (describe_product: aligned16(g.A), even(a_ld)); then a batched product under an even and an odd batch
    stride.  Every case meets the bound of the products whichever kernel takes it."""
    M, N, K = 2176, 2048, 800
    rng = np.random.default_rng(11)
    Am, Bm = rng.standard_normal((M, K)), rng.standard_normal((K, N))
    ref0 = Am @ Bm
    vB = sv.padded_view(rng, "kn", dict(k=K, n=N), "kn", dict(n=4), lead=4, values=Bm)
    ctx = Context(4, 4, workspace_bytes=1 << 28, lib=gpu_lib)
    try:
        ctx.prof_enable(True)            # (per-call events: what prof_query counts)
        for name, pad, lead, dma, beta in (("aligned", 6, 2, 1, 0.0), ("aligned accumulate", 6, 2, 1, 1.0),
                                           ("base moved by one element", 6, 3, 0, 0.0), ("odd pitch", 7, 2, 0, -0.5)):
            vA = sv.padded_view(rng, "mk", dict(m=M, k=K), "mk", dict(k=pad), lead=lead, values=Am)
            vC = sv.padded_view(rng, "mn", dict(m=M, n=N), "mn", dict(n=3), lead=1)
            ctx.prof_reset()
            r = sv.run_contraction(ctx, rng, "mk,kn->mn", vA, vB, vC, 1.0, beta, ref0=ref0, what=name)
            print(f"LDS-DMA product, {name}: err/bound {r:.3g}")
            assert ctx.prof_query(kernel_class=1)["launches"] == dma, name
        # three batches of 1024 x 1024 x 1200 (192 tiles, deep enough to stay on 128 x 128): the same rule for the batch
        # stride of A (describe_product: even(g.a_b1)); B is shared by the batch with stride 0
        e = dict(z=3, m=1024, k=1200, n=1024)
        Az, Bz = rng.standard_normal((3, 1024, 1200)), rng.standard_normal((1200, 1024))
        ref0 = Az @ Bz
        vB = sv.padded_view(rng, "zkn", e, "zkn", dict(n=2), lead=2, broadcast="z", values=Bz)
        for name, gap, dma in (("even batch stride", 2, 1), ("odd batch stride", 1, 0)):
            stride_z = 1024 * 1202 + gap
            vA = sv.strided_view(rng, [3, 1024, 1200], 2, [stride_z, 1202, 1], 2 + 3 * stride_z, values=Az)
            vC = sv.padded_view(rng, "zmn", e, "zmn", dict(n=1, m=1), lead=1)
            ctx.prof_reset()
            r = sv.run_contraction(ctx, rng, "zmk,zkn->zmn", vA, vB, vC, -1.0, 1.0, ref0=ref0, what=name)
            print(f"LDS-DMA batched product, {name}: err/bound {r:.3g}")
            assert ctx.prof_query(kernel_class=1)["launches"] == dma, name
    finally:
        ctx.prof_enable(False)
        ctx.close()


def test_fixed_strided_products(gpu_lib, monkeypatch, tmp_path):
    """Larger products through strided views, each with the route it is meant for: per-call profiling writes one line per
    product (PYMES_GEMM_LOG), and the line must name the kernel family, the load width and the orientation."""
    log = tmp_path / "gemm.log"
    log.write_text("")
    monkeypatch.setenv("PYMES_GEMM_LOG", str(log))
    rng = np.random.default_rng(12)
    ctx = Context(4, 4, workspace_bytes=1 << 28, lib=gpu_lib)
    P = sv.padded_view
    seen = [0]

    def run(route, spec, vA, vB, vC, alpha, beta, **kw):
        ctx.prof_reset()
        sv.run_contraction(ctx, rng, spec, vA, vB, vC, alpha, beta, what=route, **kw)
        ctx.prof_query(0)                    # (writes the lines of the calls since prof_reset)
        lines = [ln for ln in log.read_text().splitlines() if ln != "----"]
        new, seen[0] = lines[seen[0]:], len(lines)
        assert len(new) == 1 and all(part in new[0] + " " for part in route), (route, new)
    try:
        ctx.prof_enable(True)
        # three batches zmk,zkn->zmn: an odd batch stride of A (one more element between the matrices; describe_product:
        # even(g.a_b1)) and a B shared by the batch with stride 0: 8-byte loads ...
        e = dict(z=3, m=640, k=1000, n=512)
        stride_z = e["m"] * (e["k"] + 2) + 1
        vA = sv.strided_view(rng, [3, 640, 1000], 2, [stride_z, e["k"] + 2, 1], 2 + 3 * stride_z)
        run(("M=640 N=512 K=1000 batch=3 ", " vec=1 "), "zmk,zkn->zmn", vA, P(rng, "zkn", e, "zkn", dict(n=2), broadcast="z"),
            P(rng, "zmn", e, "zmn", dict(n=1), lead=1), -1.0, 1.0)
        # ... and with everything even and a B of its own per batch: 16-byte loads
        run(("M=640 N=512 K=1000 batch=3 ", " vec=2 "), "zmk,zkn->zmn", P(rng, "zmk", e, "zmk", dict(k=2), lead=2),
            P(rng, "zkn", e, "zkn", dict(n=2), lead=4), P(rng, "zmn", e, "zmn", dict(n=2)), 0.5, 0.0)
        # matrix-vector kernels (gemv_dispatch: aligned16(it.W), even(ld)), K = 100000.  M = 1, weighted column sums of a
        # column-sliced matrix at an odd offset on an odd pitch, then on an aligned even one
        e = dict(k=100000, n=96)
        for pad, lead, vec in ((5, 1, 1), (4, 2, 2)):
            run(("M=1 N=96 K=100000 ", " gemv=cols ", f" vec={vec} "), "k,kn->n", P(rng, "k", e, "k", {}, lead=1),
                P(rng, "kn", e, "kn", dict(n=pad), lead=lead), P(rng, "n", e, "n", {}, lead=1), 1.0, 0.0)
        # N = 1, one dot per row of a K-contiguous matrix at an odd offset (then aligned), into a result with ldc = 3
        e = dict(m=512, k=100000)
        W, x = rng.standard_normal((512, 100000)), rng.standard_normal(100000)
        for pad, lead, vec in ((3, 1, 1), (2, 2, 2)):
            run(("M=512 N=1 K=100000 ", " gemv=rows ", f" vec={vec} "), "mk,k->m",
                P(rng, "mk", e, "mk", dict(k=pad), lead=lead, values=W), P(rng, "k", e, "k", {}, values=x), _column(rng, 512, 3),
                0.5, 1.0, ref0=W @ x)
        # N = 1 with an M-contiguous matrix (column sums), result with ldc = 2
        e = dict(m=96, k=100000)
        col = lambda e=e: (P(rng, "km", e, "km", dict(m=3), lead=3), P(rng, "k", e, "k", {}, lead=1), _column(rng, 96, 2))
        run(("M=96 N=1 K=100000 ", " gemv=cols ", " vec=1 "), "km,k->m", *col(), -1.0, -0.5)
        # the transposed orientation C^T = B^T A^T: C has its unit stride on the M label, so the kernel's M is the
        # contraction's N; two batch labels that pads keep unmerged; ragged 129 x 65 x 400
        e = dict(y=2, z=3, m=129, n=65, k=400)
        run(("M=65 N=129 K=400 batch=6 ",), "yzmk,yzkn->yznm", P(rng, "yzmk", e, "yzmk", dict(z=1, k=1), lead=1),
            P(rng, "yzkn", e, "zykn", dict(n=3, y=1)), P(rng, "yznm", e, "yznm", dict(m=1, z=1), lead=2), 1.0, 1.0)
        # without per-call profiling the small matrix-vector product is a task of the open phase: the same numbers
        ctx.prof_enable(False)
        sv.run_contraction(ctx, rng, "km,k->m", *col(), 0.5, 0.0)
    finally:
        ctx.prof_enable(False)
        ctx.close()


def _column(rng, n, step):
    """A length-n output view with element stride ``step``."""
    return sv.strided_view(rng, [n], 1, [step], 1 + n * step)
