"""The stride arguments of the C-ABI (pymes_contract, pymes_permute, pymes_set_V_pqrs, pymes_set_V_block) on the CPU
stand-in: the host planner of Engine::contract under sliced, pitched, offset and stride-0 views with batch labels — merge of
groups and batch dims, the eight-way choice of copies, the host loop over outer batch dims, the write-back of a copied C —
and what the interface refuses.  The kernels under the same inputs: tests/test_gpu_strided_abi.py."""
import ctypes as C

import pytest

from pymes_amd._lib import i64_array
from pymes_amd.device import Context
from tests import _strided_views as sv


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_strided_contractions_host_logic(hostsim_lib, seed):
    sv.check_strided_contractions(hostsim_lib, seed, 120, mode="env")


def test_strided_contractions_grouped_host_logic(hostsim_lib):
    sv.check_strided_contractions(hostsim_lib, 0, 120, mode="group")


@pytest.mark.parametrize("seed", [0, 1])
def test_strided_permutations_host_logic(hostsim_lib, seed):
    sv.check_strided_permutations(hostsim_lib, seed)


def test_strided_integrals_host_logic(hostsim_lib):
    sv.check_strided_integrals(hostsim_lib)


def test_planner_mirror_on_known_layouts():
    """plan_copies (the mirror of Engine::contract's choice that the fuzz classifies its cases with) on layouts whose answer is
    known by hand."""
    # contiguous ab,bc->ac: nothing copied
    assert sv.plan_copies("ab", "bc", "ac", "", ([4, 5], [5, 1]), ([5, 6], [6, 1]), ([4, 6], [6, 1]), 0.0) == (False, False, False)
    # C with a step of 2 on both axes has no unit stride: copied, the inputs are not
    assert sv.plan_copies("ab", "bc", "ac", "", ([4, 5], [5, 1]), ([5, 6], [6, 1]), ([4, 6], [24, 2]), 1.0) == (False, False, True)
    # A[m1, k, m2] contiguous: its M labels do not merge around k
    assert sv.plan_copies("akb", "kc", "abc", "", ([2, 3, 4], [12, 4, 1]), ([3, 5], [5, 1]), ([2, 4, 5], [20, 5, 1]), 0.0)[0]


def test_refusals(hostsim_lib):
    lib = hostsim_lib
    ctx = Context(2, 2, lib=lib)
    try:
        buf = ctx.zeros((4096,))
        p = C.c_void_p(buf.ptr)
        before = sv.live_allocations(lib)

        def contract(la, da, lb, db, lc, dc, batch="", sa=None, sb=None, sc=None):
            return lambda: lib.call("pymes_contract", ctx.handle, 1.0, p, la.encode(), i64_array(da), i64_array(sa),
                                    p, lb.encode(), i64_array(db), i64_array(sb), 0.0, p, lc.encode(), i64_array(dc),
                                    i64_array(sc), batch.encode())

        def permute(li, di, lo, si=None, so=None):
            return lambda: lib.call("pymes_permute", ctx.handle, 1.0, p, li.encode(), i64_array(di), i64_array(si), 0.0, p,
                                    lo.encode(), i64_array(so))
        sv.refused(contract("abcdefg", [1] * 7, "ga", [1, 1], "bcdef", [1] * 5), "tensor rank must be 0..6")
        sv.refused(permute("abcdefg", [1] * 7, "abcdefg"), "tensor rank must be 0..6")
        sv.refused(contract("aab", [2, 2, 3], "bc", [3, 2], "ac", [2, 2]), "repeated label in 'aab'")
        sv.refused(contract("ab", [2, 3], "bc", [3, 2], "acd", [2, 2, 2]), "label 'd' appears in only one tensor")
        sv.refused(contract("ab", [2, 3], "bc", [3, 2], "ac", [2, 2], batch="b"), "batch label 'b' must be an output index")
        sv.refused(contract("ab", [2, 3], "bc", [4, 2], "ac", [2, 2]), "extent mismatch for label 'b'")
        sv.refused(permute("abc", [2, 3, 4], "abd"), "output label missing from input")
        sv.refused(permute("abc", [2, 3, 4], "aab"), "repeated label in 'aab'")
        # negative strides: refused by the name of the argument (include/pymes_amd.h), never run
        sv.refused(contract("ab", [2, 3], "bc", [3, 2], "ac", [2, 2], sa=[3, -1]), "strideA: negative stride -1 at axis 1")
        sv.refused(contract("ab", [2, 3], "bc", [3, 2], "ac", [2, 2], sb=[-2, 1]), "strideB: negative stride -2 at axis 0")
        sv.refused(contract("ab", [2, 3], "bc", [3, 2], "ac", [2, 2], sc=[-2, 1]), "strideC: negative stride")
        sv.refused(permute("ab", [2, 3], "ba", si=[-3, 1]), "stride_in: negative stride")
        sv.refused(permute("ab", [2, 3], "ba", so=[1, -3]), "stride_out: negative stride")
        sv.refused(lambda: lib.call("pymes_set_V_pqrs", ctx.handle, p, 1, i64_array([64, 16, -4, 1])), "strides: negative stride")
        sv.refused(lambda: lib.call("pymes_set_V_block", ctx.handle, b"ijab", p, 16, 1, i64_array([8, 4, 2, -1])),
                   "strides: negative stride")
        assert sv.live_allocations(lib) == before
        assert not buf.get().any()                        # nothing was written by a refused call
    finally:
        ctx.close()
