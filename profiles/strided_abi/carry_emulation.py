"""The digit walk of permute_direct_body (csrc/kernels.hip) on the CPU, with and without its carry, for the fixed case
"direct 2.3e6" of tests/_strided_views.py: canonical dims (61, 13, 41, 71), a grid of 8192 x 256 threads.  Prints how many of
the sampled threads that make a second trip land on the right element.  Nothing here runs a kernel.

    python profiles/strided_abi/carry_emulation.py
"""
import numpy as np

DIMS = [61, 13, 41, 71]          # sorted by output stride, as dev::permute canonicalises them
STRIDE = 8192 * 256              # grid_for(total, 256, 256 * 32) blocks of 256 threads


def digits(x):
    out = []
    for d in reversed(DIMS[1:]):
        out.append(x % d)
        x //= d
    return [x] + out[::-1]


def second_trip(idx, carry):
    c, sd = digits(idx), digits(STRIDE)
    k = 0
    for d in range(len(DIMS) - 1, 0, -1):
        c[d] += sd[d] + (k if carry else 0)
        k = 1 if c[d] >= DIMS[d] else 0
        c[d] -= DIMS[d] if k else 0
    c[0] += sd[0] + (k if carry else 0)
    return c


if __name__ == "__main__":
    total = int(np.prod(DIMS))
    sample = range(0, total - STRIDE, 997)
    for carry in (True, False):
        wrong = sum(second_trip(i, carry) != digits(i + STRIDE) for i in sample)
        print(f"carry={carry}: {total - STRIDE} threads make a second trip; of {len(sample)} sampled, {wrong} land on a wrong element")
