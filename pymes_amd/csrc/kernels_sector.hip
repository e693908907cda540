// Kernels of the momentum-sector CCD / DCD path (pymes_amd/solver/ueg_cc.py; DESIGN "Momentum sectors"): a ragged batched
// fp64 product over a device-resident task table, the gathers between the three sector layouts, and the element-wise tails;
// and of the momentum-blocked (T) on the same path: the W slab, the energy partials and their ordered sum;
// and the two-slab instantiation of the energy kernel for the Lambda-(T) (what the two share: DESIGN 8m); and the
// bin sums, the fused V_abcd transfer sums and the gamma sums of the sector densities; and the per-target
// preparation, the operand packing and the assembly of the sector IP- / EA-EOM-CCD sigma; and one Arnoldi step on a
// device-resident basis for the sector spectral functions; and the direct particle ladder, the ragged product with
// V_abcd generated from ladder terms instead of read.
// Included at the end of kernels.hip (one code object for the library), not compiled on its own.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/pymes_amd.h"
#include "device_api.h"
#include "device_util.h"
#include "launch.h"

namespace {

constexpr int kSgBM = PYMES_SECTOR_TILE_M, kSgBN = PYMES_SECTOR_TILE_N, kSgBK = 64;
static_assert(kSgBM == 32 && kSgBN == 16, "the thread maps below are written for 32 x 16 tiles of 256 threads");
static_assert(sizeof(pymes_sector_task) == 112, "pymes_sector_task is 14 eight-byte fields");

// One 64-deep panel of a tile's operands in registers: 8 elements of A and 4 of B per thread, read along the contiguous
// direction of each operand as stored (A: k when m x k, m when k x m; B: n when k x n, k when n x k).  Nothing outside the
// block is read: what lies beyond m, n or k is 0.
struct SectorPanel { double a[8], b[4]; };
__device__ __forceinline__ void sector_panel_load(SectorPanel& p, const pymes_sector_task& t, const double* __restrict__ Ab,
                                                  const double* __restrict__ Bb, bool ta, bool tb, long row0, long col0, long k0,
                                                  int tid) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int kk = ta ? (tid >> 5) + 8 * i : (tid & 63), r = ta ? (tid & 31) : (tid >> 6) + 4 * i;
        const long gk = k0 + kk, gr = row0 + r;
        p.a[i] = (gr < t.m && gk < t.k) ? (ta ? Ab[gk * t.lda + gr] : Ab[gr * t.lda + gk]) : 0.0;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = tid + 256 * i;
        const int kk = tb ? (idx & 63) : (idx >> 4), c = tb ? (idx >> 6) : (idx & 15);
        const long gk = k0 + kk, gc = col0 + c;
        p.b[i] = (gk < t.k && gc < t.n) ? (tb ? Bb[gc * t.ldb + gk] : Bb[gk * t.ldb + gc]) : 0.0;
    }
}

// C^t = alpha op(A^t) op(B^t) + beta C^t for every task t of the table: one workgroup per 32 x 16 tile of an output block,
// tiles numbered task after task (tile0), so the work of a launch and the order of every sum are fixed by the table alone
// -- no atomics, identical calls give identical bits.  The operands go through LDS in 64-deep panels; the next panel is
// already on its way into registers while the current one is multiplied, so a workgroup that streams a long A (the ladder:
// n is tiny, V_abcd is read once) keeps its loads in flight.  Each thread keeps 2 rows x 1 column and adds k in ascending
// order with fp64 vector FMAs.  With beta == 0 the output is not read.
__global__ void __launch_bounds__(256) sector_gemm_kernel(const pymes_sector_task* __restrict__ tasks, int ntask,
                                                          const double* __restrict__ A, const double* __restrict__ B, double* C) {
    __shared__ double As[kSgBK][kSgBM + 1];
    __shared__ double Bs[kSgBK][kSgBN + 1];
    const long tile = blockIdx.x;
    int lo = 0, hi = ntask - 1;
    while (lo < hi) {                                   // the last task that starts at or before this tile
        const int mid = (lo + hi + 1) >> 1;
        if (tasks[mid].tile0 <= tile) lo = mid; else hi = mid - 1;
    }
    const pymes_sector_task t = tasks[lo];
    const long tiles_n = (t.n + kSgBN - 1) / kSgBN, tiles_m = (t.m + kSgBM - 1) / kSgBM, local = tile - t.tile0;
    if (local < 0 || local >= tiles_m * tiles_n) return;
    const long row0 = (local / tiles_n) * kSgBM, col0 = (local % tiles_n) * kSgBN;
    const bool ta = t.flags & PYMES_SECTOR_TRANS_A, tb = t.flags & PYMES_SECTOR_TRANS_B;
    const double* __restrict__ Ab = A + t.a;
    const double* __restrict__ Bb = B + t.b;
    const int tid = threadIdx.x, col = tid & 15, rg = (tid >> 4) * 2;
    double acc[2] = {0.0, 0.0};
    SectorPanel p;
    if (t.k > 0) sector_panel_load(p, t, Ab, Bb, ta, tb, row0, col0, 0, tid);
    for (long k0 = 0; k0 < t.k; k0 += kSgBK) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int kk = ta ? (tid >> 5) + 8 * i : (tid & 63), r = ta ? (tid & 31) : (tid >> 6) + 4 * i;
            As[kk][r] = p.a[i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + 256 * i;
            Bs[tb ? (idx & 63) : (idx >> 4)][tb ? (idx >> 6) : (idx & 15)] = p.b[i];
        }
        __syncthreads();
        if (k0 + kSgBK < t.k) sector_panel_load(p, t, Ab, Bb, ta, tb, row0, col0, k0 + kSgBK, tid);
#pragma unroll 16
        for (int kk = 0; kk < kSgBK; ++kk) {
            const double b = Bs[kk][col];
            acc[0] = fma(As[kk][rg], b, acc[0]);
            acc[1] = fma(As[kk][rg + 1], b, acc[1]);
        }
        __syncthreads();
    }
    const long gc = col0 + col;
    if (gc >= t.n) return;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const long gr = row0 + rg + i;
        if (gr >= t.m) continue;
        double* out = C + t.c + gr * t.ldc + gc;
        const double v = __dmul_rn(t.alpha, acc[i]);       // (rounded on its own: the update is v + beta C, not an fma)
        *out = t.beta == 0.0 ? v : __dadd_rn(v, __dmul_rn(t.beta, *out));
    }
}

// ---- the direct particle ladder (include/pymes_amd.h, pymes_sector_ladder_direct) ------------------------------------
// sector_gemm_kernel with an A that is never read: A^t[(a,b),(c,d)] = sum_q coef_q w_q(a,b,c,d), w_q the element of ladder term q
// (ueg_pair_element, kernels_integrals.hip: the body of ueg_list_kernel), generated panel by panel straight into LDS.  Rows and
// columns are entries first[t] + r of the vv pair list (absolute orbital indices).  One workgroup takes a 32 x 32 tile: n = |OO_P|
// is at most 27 for 54 electrons, so every element of A is generated once.  The tiles are found through the task table's tile0,
// which counts 32 x 16 tiles: a workgroup whose number lies beyond the 32 x 32 tiles of its task leaves at once.
constexpr int kLdBM = 32, kLdBN = 32, kLdBK = 64, kLdTerms = PYMES_SECTOR_LADDER_MAX_TERMS;
struct LadderTerms {             // by value: the terms of one launch
    int n;
    double coef[kLdTerms];
    UegK u[kLdTerms];
    const double* umat[kLdTerms];
    const int* uidx[kLdTerms];
    const double* E[kLdTerms];
};
struct LadderPair { UegOrb x, y; };          // one entry of the vv pair list with the momenta of its two orbitals
__device__ __forceinline__ LadderPair ladder_pair(const UegK& u, const int* __restrict__ vv_rows, const int* __restrict__ k_int,
                                                  long row) {
    LadderPair p;
    p.x = ueg_orb(u, k_int, vv_rows[2 * row]);
    p.y = ueg_orb(u, k_int, vv_rows[2 * row + 1]);
    return p;
}
// B^t[k0 .. k0 + 64, col0 .. col0 + 32) into registers, read along n; 0 beyond k or n
__device__ __forceinline__ void ladder_b_load(double (&b)[8], long k, long n, long ldb, const double* __restrict__ Bb, long col0,
                                              long k0, int tid) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int idx = tid + 256 * i;
        const long gk = k0 + (idx >> 5), gc = col0 + (idx & 31);
        b[i] = (gk < k && gc < n) ? Bb[gk * ldb + gc] : 0.0;
    }
}

// Every output element adds its k products in ascending order with fma from +0.0 and ends with the tail of sector_gemm_kernel:
// for one term with coefficient 1 the bits of pymes_sector_gemm on the stored block.  Several terms are combined as
// pymes_lincomb combines stored arenas (s = 0; s = s + w_q coef_q in ascending q, product and sum rounded one after the other:
// whether lincomb_body contracts them does not matter for a coefficient that is a power of two, and a scaled stored arena was
// rounded once already).  Per panel: the columns' momenta and the B panel (loaded one panel ahead into registers) go into
// LDS; each thread generates 8 elements of its row (tid & 31) of A into LDS; then 64 steps of 2 rows x 2 columns per thread.
// The float momenta 2 pi k / L are staged with the integer ones (the host checks that the terms share L), so an element costs
// no global gather for modes 0 and 3, one u_mat lookup for mode 1 and two E lookups for mode 2.  No atomics; with beta == 0
// the output is not read; nothing outside m, n, k is read or written.
__global__ void __launch_bounds__(256) sector_ladder_direct_kernel(const pymes_sector_task* __restrict__ tasks, int ntask,
                                                                   const long* __restrict__ first, const int* __restrict__ vv_rows,
                                                                   const int* __restrict__ k_int, const LadderTerms T,
                                                                   const double* __restrict__ B, double* C) {
    __shared__ double As[kLdBK][kLdBM + 1];
    __shared__ double Bs[kLdBK][kLdBN + 1];
    __shared__ LadderPair cols[kLdBK];
    const long tile = blockIdx.x;
    int lo = 0, hi = ntask - 1;
    while (lo < hi) {                                   // the last task that starts at or before this tile
        const int mid = (lo + hi + 1) >> 1;
        if (tasks[mid].tile0 <= tile) lo = mid; else hi = mid - 1;
    }
    // (the fields are read where they are needed, the four of the tail after the loop: the whole record held in scalar
    // registers across the generation would not fit next to the terms' parameters)
    const pymes_sector_task* __restrict__ tp = tasks + lo;
    struct { long m, n, k, ldb, tile0; } t = {tp->m, tp->n, tp->k, tp->ldb, tp->tile0};
    const long tiles_n = (t.n + kLdBN - 1) / kLdBN, tiles_m = (t.m + kLdBM - 1) / kLdBM, local = tile - t.tile0;
    if (local < 0 || local >= tiles_m * tiles_n) return;
    const long row0 = (local / tiles_n) * kLdBM, col0 = (local % tiles_n) * kLdBN, f0 = first[lo];
    const bool ta = tp->flags & PYMES_SECTOR_TRANS_A;
    const double* __restrict__ Bb = B + tp->b;
    const int tid = threadIdx.x, tx = tid & 15, rg = (tid >> 4) * 2, grow = tid & 31, gk0 = tid >> 5;
    const bool row_live = row0 + grow < t.m;
    LadderPair rp;
    if (row_live) rp = ladder_pair(T.u[0], vv_rows, k_int, f0 + row0 + grow);
    double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    double b[8];
    if (t.k > 0) ladder_b_load(b, t.k, t.n, t.ldb, Bb, col0, 0, tid);
    for (long k0 = 0; k0 < t.k; k0 += kLdBK) {
        if (tid < kLdBK && k0 + tid < t.k) cols[tid] = ladder_pair(T.u[0], vv_rows, k_int, f0 + k0 + tid);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int idx = tid + 256 * i;
            Bs[idx >> 5][idx & 31] = b[i];
        }
        __syncthreads();
        if (k0 + kLdBK < t.k) ladder_b_load(b, t.k, t.n, t.ldb, Bb, col0, k0 + kLdBK, tid);
#pragma unroll 1
        for (int i = 0; i < 8; ++i) {
            const int kk = gk0 + 8 * i;
            double a = 0.0;
            if (row_live && k0 + kk < t.k) {
                const LadderPair cp = cols[kk];
                const LadderPair& bra = ta ? cp : rp;
                const LadderPair& ket = ta ? rp : cp;
                for (int q = 0; q < T.n; ++q) {
                    const double w = ueg_pair_element(T.u[q], T.umat[q], T.uidx[q], T.E[q], bra.x, bra.y, ket.x, ket.y);
                    a = __dadd_rn(a, __dmul_rn(w, T.coef[q]));
                }
            }
            As[kk][grow] = a;
        }
        __syncthreads();
#pragma unroll 16
        for (int kk = 0; kk < kLdBK; ++kk) {
            const double b0 = Bs[kk][tx], b1 = Bs[kk][tx + 16], a0 = As[kk][rg], a1 = As[kk][rg + 1];
            acc[0][0] = fma(a0, b0, acc[0][0]);
            acc[0][1] = fma(a0, b1, acc[0][1]);
            acc[1][0] = fma(a1, b0, acc[1][0]);
            acc[1][1] = fma(a1, b1, acc[1][1]);
        }
        __syncthreads();
    }
    const long c0 = tp->c, ldc = tp->ldc;
    const double alpha = tp->alpha, beta = tp->beta;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const long gr = row0 + rg + i;
        if (gr >= t.m) continue;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const long gc = col0 + tx + 16 * j;
            if (gc >= t.n) continue;
            double* out = C + c0 + gr * ldc + gc;
            const double v = __dmul_rn(alpha, acc[i][j]);      // (the tail of sector_gemm_kernel)
            *out = beta == 0.0 ? v : __dadd_rn(v, __dmul_rn(beta, *out));
        }
    }
}

// dst[i] = beta dst[i] + a1 s1[m1[i]] (+ a2 s2[m2[i]]); with beta == 0 dst is not read
__global__ void sector_gather_kernel(double* __restrict__ dst, long n, double beta, double a1, const double* __restrict__ s1,
                                     const long* __restrict__ m1, double a2, const double* __restrict__ s2,
                                     const long* __restrict__ m2) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        double v = a1 * s1[m1[i]];
        if (s2) v += a2 * s2[m2[i]];
        dst[i] = beta == 0.0 ? v : beta * dst[i] + v;
    }
}

// ---- the diagonal X_ac / X_ki terms in the direct layout: row g = (a,i) of some D^q, `len[g]` elements from `start[g]` on
// s[g] = sum_c Tt[g,c] W1[g,c], columns in ascending order
__global__ void sector_rowsum_kernel(const double* __restrict__ Tt, const double* __restrict__ W1, const long* __restrict__ start,
                                     const long* __restrict__ len, long rows, double* __restrict__ s) {
    const long g = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (g >= rows) return;
    const double* __restrict__ x = Tt + start[g];
    const double* __restrict__ y = W1 + start[g];
    double acc = 0.0;
    for (long c = 0; c < len[g]; ++c) acc = fma(x[c], y[c], acc);
    s[g] = acc;
}
// x[i] = eps[i] + w sum_a s[row(a,i)],  x[no + a] = eps[no + a] - w sum_i s[row(a,i)]      (ccd.py:213-220, diagonal here)
__global__ void sector_xdiag_kernel(const double* __restrict__ s, const long* __restrict__ row_of, const double* __restrict__ eps,
                                    double w, int no, int nv, double* __restrict__ x) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= no + nv) return;
    double acc = 0.0;
    if (p < no) {
        for (long a = 0; a < nv; ++a) acc += s[row_of[a * no + p]];
        x[p] = eps[p] + w * acc;
    } else {
        const long a = p - no;
        for (int i = 0; i < no; ++i) acc += s[row_of[a * no + i]];
        x[p] = eps[p] - w * acc;
    }
}
// Ex[g,:] += (x_vv[a] - x_oo[i]) D[g,:]
__global__ void sector_rowscale_kernel(const double* __restrict__ D, const long* __restrict__ start, const long* __restrict__ len,
                                       const long* __restrict__ ai_of, long rows, const double* __restrict__ x, int no,
                                       double* __restrict__ Ex) {
    const long g = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (g >= rows) return;
    const long ai = ai_of[g];
    const double f = x[no + ai / no] - x[ai % no];
    const double* __restrict__ d = D + start[g];
    double* __restrict__ e = Ex + start[g];
    for (long c = 0; c < len[g]; ++c) e[c] = fma(f, d[c], e[c]);
}

// dt = r / (den + shift), t_out = t_in + dt   (t_in null: t_out = dt, the MP2 start; dt null: not stored)
__global__ void sector_update_kernel(double* __restrict__ t_out, double* __restrict__ dt, const double* __restrict__ t_in,
                                     const double* __restrict__ r, const double* __restrict__ den, double shift, long n) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const double d = r[i] / (den[i] + shift);
        if (dt) dt[i] = d;
        t_out[i] = t_in ? t_in[i] + d : d;
    }
}

// ---- momentum-blocked (T) (include/pymes_amd.h, pymes_sector_triples) ---------------------------------------------
// Every operand has its implied index left out: Vv[i,a,b] = V[i,f*,a,b], Vo[i,j,a] = V[i,j,a,m*], Tc[i,j,a] = T[a,b*,i,j],
// m_of[i,j,a] = m* or -1; a position whose implied orbital does not exist holds an exact 0.  For a triple (i,j,k) and a pair
// (a,b) the third virtual c is the orbital with k_i + k_j + k_k - k_a - k_b, if there is one: W_ijk is a v x v slab Wt[a,b].
struct TriplesBox { int lo[3], dim[3]; };
constexpr int kTrTile = 32;          // a 32 x 32 tile of (a,b) per 256-thread workgroup: thread (ty, tx) keeps a = a0 + ty + 8 q, b = b0 + tx

// t = i (i+1) (i+2) / 6 + j (j+1) / 2 + k, i >= j >= k: the order of pymes_ccsd_t
__device__ __forceinline__ void triple_of(long t, int& i, int& j, int& k) {
    int ii = 0;
    while ((long)(ii + 1) * (ii + 2) * (ii + 3) / 6 <= t) ++ii;
    const long r = t - (long)ii * (ii + 1) * (ii + 2) / 6;
    int jj = 0;
    while ((long)(jj + 1) * (jj + 2) / 2 <= r) ++jj;
    i = ii;
    j = jj;
    k = (int)(r - (long)jj * (jj + 1) / 2);
}
// the orbital that carries (x,y,z), -1 if none: every axis is checked against the box, nothing is wrapped into it
__device__ __forceinline__ int triples_orb(const int* __restrict__ orb_of, const TriplesBox& bx, int x, int y, int z) {
    x -= bx.lo[0];
    y -= bx.lo[1];
    z -= bx.lo[2];
    if (x < 0 || x >= bx.dim[0] || y < 0 || y >= bx.dim[1] || z < 0 || z >= bx.dim[2]) return -1;
    return orb_of[((long)x * bx.dim[1] + y) * bx.dim[2] + z];
}
// w(xyz;pqr) = Vv[x,p,q] Tc[z,y,r] - Vo[x,y,p] Tc[m_of[x,y,p],z,q]; `vv` = Vv[x,p,q], read by the caller
__device__ __forceinline__ double triples_w(double vv, int x, int y, int z, int p, int q, int r, int no, long v,
                                            const int* __restrict__ m_of, const double* __restrict__ Tc,
                                            const double* __restrict__ Vo) {
    const long xyp = ((long)x * no + y) * v + p;
    const int m = m_of[xyp];
    double w = vv * Tc[((long)z * no + y) * v + r];
    if (m >= 0) w = fma(-Vo[xyp], Tc[((long)m * no + z) * v + q], w);
    return w;
}
// the 32 x 32 tile X[b0 .., a0 ..] of a row-major v x v slab into LDS, read along the contiguous index: tr[b - b0][a - a0]
__device__ __forceinline__ void triples_stage(double (*tr)[kTrTile + 1], const double* __restrict__ X, int nv, int a0, int b0,
                                              int tx, int ty) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int bb = b0 + ty + 8 * q, aa = a0 + tx;
        tr[ty + 8 * q][tx] = (bb < nv && aa < nv) ? X[(long)bb * nv + aa] : 0.0;
    }
    __syncthreads();
}

// What the W kernel and the energy kernel know of their place before they touch a slab: the triple of the grid row, the
// 32 x 32 tile of the grid column, the thread's (ty, tx) in it and its column b.  Every thread takes part in triples_stage;
// only one with b < nv then asks for the momenta, and for the third virtual of its rows a = row(q) < nv.
struct TriplesTile {
    int i, j, k, a0, b0, tx, ty, b, K[3], kb[3];
    __device__ __forceinline__ TriplesTile(long t0, int nv) {
        triple_of(t0 + blockIdx.y, i, j, k);
        const int tiles_b = (nv + kTrTile - 1) / kTrTile;
        a0 = (blockIdx.x / tiles_b) * kTrTile;
        b0 = (blockIdx.x % tiles_b) * kTrTile;
        tx = threadIdx.x & 31;
        ty = threadIdx.x >> 5;
        b = b0 + tx;
    }
    __device__ __forceinline__ int row(int q) const { return a0 + ty + 8 * q; }
    // K = k_i + k_j + k_k and k_b
    __device__ __forceinline__ void momenta(const int* __restrict__ k_int, int no) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            K[d] = k_int[3 * i + d] + k_int[3 * j + d] + k_int[3 * k + d];
            kb[d] = k_int[3 * (no + b) + d];
        }
    }
    // the virtual c of (a,b), counted from the first virtual; negative if there is none
    __device__ __forceinline__ int third(const int* __restrict__ k_int, const int* __restrict__ orb_of, const TriplesBox& bx,
                                         int no, int a) const {
        const int* ka = k_int + 3 * (no + a);
        return triples_orb(orb_of, bx, K[0] - ka[0] - kb[0], K[1] - ka[1] - kb[1], K[2] - ka[2] - kb[2]) - no;
    }
};

// Wt[a,b] of the triple t0 + blockIdx.y: the twelve products in the order of the formula, 0 where c is no virtual.  Every
// element of the slab is written here.  Global reads along b (Vv[i,a,b], Tc[.,.,b], the store) are contiguous; Vv[j,b,a]
// comes through the transposed LDS tile; what is indexed by c is a gather inside rows that the L2 holds.
__global__ void __launch_bounds__(256) sector_triples_w_kernel(int no, int nv, const int* __restrict__ k_int,
                                                               const int* __restrict__ orb_of, TriplesBox bx,
                                                               const int* __restrict__ m_of, const double* __restrict__ Tc,
                                                               const double* __restrict__ Vv, const double* __restrict__ Vo,
                                                               long t0, double* __restrict__ Wt) {
    __shared__ double tr[kTrTile][kTrTile + 1];
    TriplesTile tl(t0, nv);
    const int i = tl.i, j = tl.j, k = tl.k, b = tl.b;
    const long v = nv, vv = v * v;
    const double* __restrict__ Vi = Vv + i * vv;
    const double* __restrict__ Vj = Vv + j * vv;
    const double* __restrict__ Vk = Vv + k * vv;
    triples_stage(tr, Vj, nv, tl.a0, tl.b0, tl.tx, tl.ty);
    if (b >= nv) return;
    tl.momenta(k_int, no);
    double* __restrict__ W = Wt + (long)blockIdx.y * vv;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int a = tl.row(q);
        if (a >= nv) continue;
        const int c = tl.third(k_int, orb_of, bx, no, a);
        double w = 0.0;
        if (c >= 0) {
            w = triples_w(Vi[a * v + b], i, j, k, a, b, c, no, v, m_of, Tc, Vo);                 // w(ijk;abc)
            w += triples_w(Vi[a * v + c], i, k, j, a, c, b, no, v, m_of, Tc, Vo);                // w(ikj;acb)
            w += triples_w(tr[tl.tx][tl.ty + 8 * q], j, i, k, b, a, c, no, v, m_of, Tc, Vo);     // w(jik;bac)
            w += triples_w(Vj[b * v + c], j, k, i, b, c, a, no, v, m_of, Tc, Vo);                // w(jki;bca)
            w += triples_w(Vk[c * v + a], k, i, j, c, a, b, no, v, m_of, Tc, Vo);                // w(kij;cab)
            w += triples_w(Vk[c * v + b], k, j, i, c, b, a, no, v, m_of, Tc, Vo);                // w(kji;cba)
        }
        W[a * v + b] = w;
    }
}

// One partial per workgroup: sum over the tile's (a,b) with a virtual c of
// WR[a,b] (4 WL[a,b] + WL[b,c] + WL[c,a] - 2 WL[c,b] - 2 WL[a,c] - 2 WL[b,a]) / (e_i + e_j + e_k - e_a - e_b - e_c),
// each thread over its four elements in ascending a, then a fixed tree over the 256 threads.  WL[a,b] is read along b,
// WL[b,a] comes through the LDS transpose, the four reads indexed by c are gathers inside rows of WL that the L2 holds.
// (T) is the one-slab instantiation, WR = WL = Wt: WRt is not read and WL[a,b] stands in front as well.  Lambda-(T)
// reads the factor in front from the right-hand slab.
template <bool kTwoSlabs>
__global__ void __launch_bounds__(256) sector_triples_e_kernel(int no, int nv, const double* __restrict__ eps,
                                                               const int* __restrict__ k_int, const int* __restrict__ orb_of,
                                                               TriplesBox bx, long t0, const double* __restrict__ WRt,
                                                               const double* __restrict__ WLt, double* __restrict__ partial) {
    __shared__ double tr[kTrTile][kTrTile + 1];
    __shared__ double red[256];
    TriplesTile tl(t0, nv);
    const int tid = threadIdx.x, b = tl.b;
    const long v = nv;
    const double* __restrict__ WR = WRt + (long)blockIdx.y * v * v;
    const double* __restrict__ WL = WLt + (long)blockIdx.y * v * v;
    triples_stage(tr, WL, nv, tl.a0, tl.b0, tl.tx, tl.ty);
    double acc = 0.0;
    if (b < nv) {
        tl.momenta(k_int, no);
        const double eo = eps[tl.i] + eps[tl.j] + eps[tl.k];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int a = tl.row(q);
            if (a >= nv) continue;
            const int c = tl.third(k_int, orb_of, bx, no, a);
            if (c < 0) continue;
            const double wl = WL[a * v + b];
            const double r = 4.0 * wl + WL[b * v + c] + WL[c * v + a] - 2.0 * WL[c * v + b] - 2.0 * WL[a * v + c]
                             - 2.0 * tr[tl.tx][tl.ty + 8 * q];
            const double wr = kTwoSlabs ? WR[a * v + b] : wl;
            acc += wr * r / (eo - eps[no + a] - eps[no + b] - eps[no + c]);
        }
    }
    red[tid] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) partial[(long)blockIdx.y * gridDim.x + blockIdx.x] = red[0];
}

// per[t] = m_ijk S / 3, S the partials of triple t0 + t added in index order: one workgroup per triple brings 256 partials
// at a time into LDS (one contiguous read), and its first thread adds them one after the other
__global__ void __launch_bounds__(256) sector_triples_sum_kernel(const double* __restrict__ partial, long ntiles, long t0,
                                                                 double* __restrict__ per, double* __restrict__ out) {
    __shared__ double buf[256];
    const int t = blockIdx.x, tid = threadIdx.x;
    const double* __restrict__ p = partial + t * ntiles;
    double s = 0.0;
    for (long q0 = 0; q0 < ntiles; q0 += 256) {
        buf[tid] = q0 + tid < ntiles ? p[q0 + tid] : 0.0;
        __syncthreads();
        if (tid == 0) {
            const int n = (int)(ntiles - q0 < 256 ? ntiles - q0 : 256);
            for (int r = 0; r < n; ++r) s += buf[r];
        }
        __syncthreads();
    }
    if (tid != 0) return;
    int i, j, k;
    triple_of(t0 + t, i, j, k);
    const double m = (i == j && j == k) ? 1.0 : (i == j || j == k) ? 3.0 : 6.0;
    const double val = m * (s / 3.0);
    per[t] = val;
    if (out) out[t] = val;
}

// the lookup box of a triples entry, checked: {lo[3], dims[3]} on the host
TriplesBox triples_box(const std::string& who, const int32_t* box_host) {
    TriplesBox bx;
    int64_t points = 1;
    for (int d = 0; d < 3; ++d) {
        bx.lo[d] = box_host[d];
        bx.dim[d] = box_host[3 + d];
        if (bx.dim[d] < 1) throw std::runtime_error(who + ": empty lookup box");
        points *= bx.dim[d];
        if (points > 0x7fffffffL) throw std::runtime_error(who + ": the lookup box holds more than 2^31 points");
    }
    return bx;
}
void triples_range(const std::string& who, int no, int64_t t_begin, int64_t t_end) {
    const int64_t total = (int64_t)no * (no + 1) * (no + 2) / 6;
    if (t_begin < 0 || t_end < t_begin || t_end > total)
        throw std::runtime_error(who + ": triple range [" + std::to_string(t_begin) + ", " + std::to_string(t_end) +
                                 ") outside [0, " + std::to_string(total) + "]");
}
// the values are added in triple order with the rounding error of every add carried along (Neumaier): thousands of
// terms of one sign would otherwise lose more than the values themselves are good for.  volatile: no reassociation.
struct OrderedSum {
    volatile double sum = 0.0, carry = 0.0;
    void add(double x) {
        const double s = sum + x;
        carry += std::fabs(sum) >= std::fabs(x) ? (sum - s) + x : (x - s) + sum;
        sum = s;
    }
    double value() const { return sum + carry; }
};

// The host side of (T) and Lambda-(T) (dev::sector_triples, dev::sector_triples_lambda): the triples of [t_begin, t_end) in
// batches of as many as `ws` holds, one grid row each.  ws: the slab(s) of the batch, then one partial per tile, then the
// values.  Without `left` there is one slab W (Tc, Vv, Vo) per triple and the energy kernel reads it on both sides.  With it
// there are two, WR from `right` and WL from `left`, by two launches of the unchanged sector_triples_w_kernel: a side index
// on blockIdx.z would put a select of three base pointers in front of every gather of a kernel whose (T) timings are
// recorded, to save one launch (~10 us) per batch of kernels that run for milliseconds.
struct TriplesSide { const double *Tc, *Vv, *Vo; };
double sector_triples_run(const std::string& who, int no, int nv, const double* eps, const int32_t* k_int, const int32_t* orb_of,
                          const int32_t* box_host, const int32_t* m_of, const TriplesSide& right, const TriplesSide* left,
                          int64_t t_begin, int64_t t_end, double* ws, int64_t ws_bytes, double* per_triple, dev::stream_t s) {
    if (no < 1 || nv < 1 || nv > (1 << 20)) throw std::runtime_error(who + ": bad orbital counts");
    if (!eps || !k_int || !orb_of || !box_host || !m_of || !right.Tc || !right.Vv || !right.Vo || !ws ||
        (left && (!left->Tc || !left->Vv || !left->Vo)))
        throw std::runtime_error(who + ": null argument");
    triples_range(who, no, t_begin, t_end);
    const TriplesBox bx = triples_box(who, box_host);
    const int64_t tiles1 = (nv + kTrTile - 1) / kTrTile, ntiles = tiles1 * tiles1, slab = (int64_t)nv * nv;
    const int64_t each = (left ? 2 : 1) * slab + ntiles + 1;  // per triple: the slab(s), one partial per tile, the value
    const int64_t fit = ws_bytes / 8 / each;
    if (fit < 1)
        throw std::runtime_error(who + ": the workspace does not hold one triple (" + std::to_string(8 * each) + " bytes)");
    const int64_t nb = std::min<int64_t>(fit, 65535);         // triples per batch: one grid row each
    double* WR = ws;
    double* WL = left ? ws + nb * slab : ws;
    double* partial = WL + nb * slab;
    double* per = partial + nb * ntiles;
    hipStream_t st = (hipStream_t)s;
    std::vector<double> host((size_t)std::min<int64_t>(nb, std::max<int64_t>(t_end - t_begin, 1)));
    OrderedSum total;
    for (int64_t t0 = t_begin; t0 < t_end; t0 += nb) {
        const int n = (int)std::min<int64_t>(nb, t_end - t0);
        const dim3 grid((unsigned)ntiles, (unsigned)n);
        launch_kernel(sector_triples_w_kernel, grid, dim3(256), 0, st, no, nv, k_int, orb_of, bx, m_of, right.Tc, right.Vv,
                      right.Vo, (long)t0, WR);
        if (left)
            launch_kernel(sector_triples_w_kernel, grid, dim3(256), 0, st, no, nv, k_int, orb_of, bx, m_of, left->Tc, left->Vv,
                          left->Vo, (long)t0, WL);
        launch_kernel(left ? sector_triples_e_kernel<true> : sector_triples_e_kernel<false>, grid, dim3(256), 0, st, no, nv, eps,
                      k_int, orb_of, bx, (long)t0, (const double*)WR, (const double*)WL, partial);
        launch_kernel(sector_triples_sum_kernel, dim3((unsigned)n), dim3(256), 0, st, (const double*)partial, (long)ntiles,
                      (long)t0, per, per_triple ? per_triple + (t0 - t_begin) : (double*)nullptr);
        HIP_CHECK(copy_async(host.data(), per, sizeof(double) * n, hipMemcpyDeviceToHost, st));
        wait_idle(st);
        for (int q = 0; q < n; ++q) total.add(host[q]);       // in triple order, whatever the batch size
    }
    return total.value();
}

// ---- sector densities: sums of a density arena over the bins of the momentum transfer -------------------------------
// out[b] = beta out[b] + alpha sum_j src[list[j]], off[b] <= j < off[b + 1].  A workgroup owns four consecutive bins.  A bin of
// at most kBinShort elements is summed by one wavefront (lane l adds j = off + l, off + l + 64, ... in ascending order, then a
// fixed tree over the 64 lanes); a longer one by the whole workgroup (256 strides, a tree over 256), one long bin after the
// other.  Which of the two a bin takes depends on its length alone: no atomics, identical calls give identical bits.  With
// beta == 0 out is not read.
constexpr long kBinShort = 256;
__global__ void __launch_bounds__(256) sector_bin_sums_kernel(double* __restrict__ out, long nbins, const long* __restrict__ off,
                                                              const long* __restrict__ list, const double* __restrict__ src,
                                                              double alpha, double beta) {
    __shared__ double red[256];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long b0 = blockIdx.x * 4L;
    {
        const long b = b0 + wave;
        bool mine = false;
        double acc = 0.0;
        if (b < nbins) {
            const long lo = off[b], hi = off[b + 1];
            mine = hi - lo <= kBinShort;
            if (mine)
                for (long j = lo + lane; j < hi; j += 64) acc += src[list[j]];
        }
        red[tid] = acc;
        __syncthreads();
        for (int s = 32; s > 0; s >>= 1) {
            if (lane < s) red[tid] += red[tid + s];
            __syncthreads();
        }
        if (mine && lane == 0) {
            const double v = alpha * red[tid];
            out[b] = beta == 0.0 ? v : beta * out[b] + v;
        }
        __syncthreads();
    }
    for (int w = 0; w < 4; ++w) {
        const long b = b0 + w;
        if (b >= nbins) break;
        const long lo = off[b], hi = off[b + 1];
        if (hi - lo <= kBinShort) continue;             // (the same for every thread of the workgroup)
        double acc = 0.0;
        for (long j = lo + tid; j < hi; j += 256) acc += src[list[j]];
        red[tid] = acc;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) red[tid] += red[tid + s];
            __syncthreads();
        }
        if (tid == 0) {
            const double v = alpha * red[0];
            out[b] = beta == 0.0 ? v : beta * out[b] + v;
        }
        __syncthreads();
    }
}

// The V_abcd part of the transfer sums without an array over the v^4 sectors: for the bin vector q,
//   out[bin] = sum over rows (a,b) of the pp layout with c = orb(k_a + q) and d = orb(k_b - q) both virtual of
//              sum_ij lam[(a,b),ij] T[(c,d),ij]
// (k_c + k_d = k_a + k_b, so the row (c,d) lies in the sector of (a,b) and has as many columns).  row_of_pair[c nv + d] is the
// row of the virtual pair, -1 if it has none.  One workgroup owns a bin and the workgroups stride over the bins: thread t
// takes the rows t, t + 256, ... in ascending order, each dot in ascending ij, then a fixed tree over the 256 partials -- the
// value of a bin does not depend on the grid.  A bin that no row reaches is an exact +0.0.
__global__ void __launch_bounds__(256) sector_pair_transfer_kernel(
        double* __restrict__ out, long nbins, const int* __restrict__ bin_q, const int* __restrict__ k_int,
        const int* __restrict__ orb_of, TriplesBox bx, int no, int nv, long rows, const int* __restrict__ vv_pairs,
        const long* __restrict__ row_start, const long* __restrict__ row_len, const long* __restrict__ row_of_pair,
        const double* __restrict__ lam, const double* __restrict__ T) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    for (long bin = blockIdx.x; bin < nbins; bin += gridDim.x) {
        const int qx = bin_q[3 * bin], qy = bin_q[3 * bin + 1], qz = bin_q[3 * bin + 2];
        double acc = 0.0;
        for (long r = tid; r < rows; r += 256) {
            const int a = no + vv_pairs[2 * r], b = no + vv_pairs[2 * r + 1];
            const int c = triples_orb(orb_of, bx, k_int[3 * a] + qx, k_int[3 * a + 1] + qy, k_int[3 * a + 2] + qz);
            if (c < no) continue;
            const int d = triples_orb(orb_of, bx, k_int[3 * b] - qx, k_int[3 * b + 1] - qy, k_int[3 * b + 2] - qz);
            if (d < no) continue;
            const long r2 = row_of_pair[(long)(c - no) * nv + (d - no)];
            if (r2 < 0) continue;
            const long len = row_len[r];
            const double* __restrict__ x = lam + row_start[r];
            const double* __restrict__ y = T + row_start[r2];
            double dot = 0.0;
            for (long j = 0; j < len; ++j) dot = fma(x[j], y[j], dot);
            acc += dot;
        }
        red[tid] = acc;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) red[tid] += red[tid + s];
            __syncthreads();
        }
        if (tid == 0) out[bin] = red[0];
        __syncthreads();
    }
}

// rho[g] = sum_c x[g,c] y[g,c] over the rows of the direct layout (the kernel of sector_xdiag, which keeps its sums to itself);
// gamma[no + a] = sum_i rho[row(a,i)], gamma[i] = -sum_a rho[row(a,i)], in ascending order
__global__ void sector_gamma_kernel(const double* __restrict__ rho, const long* __restrict__ row_of, int no, int nv,
                                    double* __restrict__ gamma) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= no + nv) return;
    double acc = 0.0;
    if (p < no) {
        for (long a = 0; a < nv; ++a) acc += rho[row_of[a * no + p]];
        gamma[p] = -acc;
    } else {
        const long a = p - no;
        for (int i = 0; i < no; ++i) acc += rho[row_of[a * no + i]];
        gamma[p] = acc;
    }
}

// ---- sector IP- / EA-EOM-CCD (include/pymes_amd.h, pymes_sector_ipea_*) ------------------------------------------------
// One momentum block of the operator: the singles element r1[p] and the doubles R[x,y] with their implied virtual b* left out
// (IP: x = i, y = j, k_b = k_i + k_j - k_p; EA: x = a, y = j, k_b = k_p + k_j - k_a).  The kernels below are written once for
// both kinds: they see positions t = x no + y, the maps of sectors.QuasiparticleTables (-1 outside the space) and, in the
// prepare kernel, the kind as a template argument.
constexpr int kQpMax = 32;
struct QpIn {            // the k <= 32 vectors of one call, by value: r1_z (one element) and r2_z (npos elements)
    const double* r1[kQpMax];
    const double* r2[kQpMax];
};
struct QpOut {
    double* s1[kQpMax];
    double* s2[kQpMax];
};
__device__ __forceinline__ int qp_virtual(const int* __restrict__ orb_of, const TriplesBox& bx, int no, int x, int y, int z) {
    return triples_orb(orb_of, bx, x, y, z) - no;           // counted from the first virtual; negative: none, or occupied
}

// What depends on the target alone, one thread per position t = (x,y), every sum in ascending index order:
//   d2[t]  IP  L_b* - L_i - L_j                      EA  L_a + L_b* - L_j                    (`outside` where b* does not exist)
//   W[t]   IP  -2 Vo[j,i,b*] + Vo[i,j,b*]            EA  2 Vv[j,b*,a] - Vv[j,a,b*]           (s1 = -+ L_pp r1 + sum_t W[t] R[t])
//   U[t]   everything r1 multiplies in s2[t], the formulas of include/pymes_amd.h (pymes_sector_ipea_prepare)
// The implied orbital of each inner sum comes from the lookup box; Tc and the four lists hold an exact 0 where theirs does
// not exist.  p: the target, an orbital index over all no + nv.
template <bool kIp>
__global__ void __launch_bounds__(256) sector_qp_prepare_kernel(int p, int no, int nv, const int* __restrict__ k_int,
                                                                const int* __restrict__ orb_of, TriplesBox bx,
                                                                const int* __restrict__ b_of, const double* __restrict__ L,
                                                                const double* __restrict__ Tc, const double* __restrict__ Vv,
                                                                const double* __restrict__ Vo, const double* __restrict__ VvR,
                                                                const double* __restrict__ VoR, double outside,
                                                                double* __restrict__ U, double* __restrict__ W,
                                                                double* __restrict__ d2) {
    const long npos = (long)(kIp ? no : nv) * no;
    const long t = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (t >= npos) return;
    const int b = b_of[t];
    if (b < 0) {
        U[t] = 0.0;
        W[t] = 0.0;
        d2[t] = outside;
        return;
    }
    const int x = (int)(t / no), y = (int)(t % no);
    const long v = nv;
    auto oov = [&](int i, int j, int a) { return ((long)i * no + j) * v + a; };
    auto ovv = [&](int i, int a, int c) { return ((long)i * v + a) * v + c; };
    const int* kp = k_int + 3 * p;
    double u;
    if (kIp) {
        const int i = x, j = y;
        const int *ki = k_int + 3 * i, *kj = k_int + 3 * j;
        d2[t] = L[no + b] - L[i] - L[j];
        W[t] = -2.0 * Vo[oov(j, i, b)] + Vo[oov(i, j, b)];
        u = -VoR[oov(j, i, b)];
        for (int k = 0; k < no; ++k) {
            const int* kk = k_int + 3 * k;
            int c = qp_virtual(orb_of, bx, no, kk[0] + kp[0] - ki[0], kk[1] + kp[1] - ki[1], kk[2] + kp[2] - ki[2]);
            if (c >= 0)
                u += Vo[oov(k, p, c)] * (-2.0 * Tc[oov(k, j, c)] + Tc[oov(j, k, c)]) + Vo[oov(p, k, c)] * Tc[oov(k, j, c)];
            c = qp_virtual(orb_of, bx, no, kk[0] + kp[0] - kj[0], kk[1] + kp[1] - kj[1], kk[2] + kp[2] - kj[2]);
            if (c >= 0) u += Vo[oov(p, k, c)] * Tc[oov(i, k, c)];
        }
        for (int c = 0; c < nv; ++c) {
            const int* kc = k_int + 3 * (no + c);
            const int d = qp_virtual(orb_of, bx, no, ki[0] + kj[0] - kc[0], ki[1] + kj[1] - kc[1], ki[2] + kj[2] - kc[2]);
            if (d >= 0) u -= Vv[ovv(p, c, d)] * Tc[oov(i, j, c)];
        }
    } else {
        const int a = x, j = y, pv = p - no;
        const int *ka = k_int + 3 * (no + a), *kb = k_int + 3 * (no + b), *kj = k_int + 3 * j;
        d2[t] = L[no + a] + L[no + b] - L[j];
        W[t] = 2.0 * Vv[ovv(j, b, a)] - Vv[ovv(j, a, b)];
        u = VvR[ovv(j, b, a)];
        for (int k = 0; k < no; ++k) {
            const int* kk = k_int + 3 * k;
            int c = qp_virtual(orb_of, bx, no, kk[0] + ka[0] - kp[0], kk[1] + ka[1] - kp[1], kk[2] + ka[2] - kp[2]);
            if (c >= 0)
                u += Vv[ovv(k, c, pv)] * (2.0 * Tc[oov(k, j, c)] - Tc[oov(j, k, c)]) - Vv[ovv(k, pv, c)] * Tc[oov(k, j, c)];
            c = qp_virtual(orb_of, bx, no, kk[0] + kb[0] - kp[0], kk[1] + kb[1] - kp[1], kk[2] + kb[2] - kp[2]);
            if (c >= 0) u -= Vv[ovv(k, pv, c)] * Tc[oov(j, k, c)];
            const int m = triples_orb(orb_of, bx, kp[0] + kj[0] - kk[0], kp[1] + kj[1] - kk[1], kp[2] + kj[2] - kk[2]);
            if (m >= 0 && m < no) u += Vo[oov(k, m, pv)] * Tc[oov(k, m, a)];
        }
    }
    U[t] = u;
}

// Forward: the k vectors into the three operands of the products, the vector index running fastest.  Block (bx, z) takes 256
// positions of vector z:  XR[ph[t], z] = R_z[t],  XX[ph[t], z] = R_z[partner[t]] (the exchanged element),  XP[pair[t], z] = R_z[t].
// The maps are bijections of the space onto [0, count), so every element of the three is written, each once.
__global__ void __launch_bounds__(256) sector_qp_pack_kernel(QpIn in, int k, long npos, const long* __restrict__ ph,
                                                             const long* __restrict__ partner, const long* __restrict__ pair,
                                                             double* __restrict__ XR, double* __restrict__ XX,
                                                             double* __restrict__ XP) {
    const int z = blockIdx.y;
    const long t = blockIdx.x * 256L + threadIdx.x;
    if (t >= npos) return;
    const long g = ph[t];
    if (g < 0) return;
    const double* __restrict__ r2 = in.r2[z];
    const double a = r2[t];
    XR[g * k + z] = a;
    XX[g * k + z] = r2[partner[t]];
    XP[pair[t] * k + z] = a;
}

// Backward: s2_z[t] = d2[t] R_z[t] + r1_z U[t] + G1[ph[t], z] + G2[ph_partner[t], z] + H[pair[t], z], added in this order, and an
// exact +0.0 at a position outside the space; the last block of every vector z adds s1_z = d1 r1_z + sum_t W[t] R_z[t]
// (each thread over t = tid, tid + 256, ... in ascending order, then a fixed tree): no atomics, identical calls, identical bits.
__global__ void __launch_bounds__(256) sector_qp_assemble_kernel(QpIn in, QpOut out, int k, long npos, const long* __restrict__ ph,
                                                                 const long* __restrict__ ph_partner,
                                                                 const long* __restrict__ pair, const double* __restrict__ d2,
                                                                 const double* __restrict__ U, const double* __restrict__ W,
                                                                 double d1, const double* __restrict__ G1,
                                                                 const double* __restrict__ G2, const double* __restrict__ H) {
    __shared__ double red[256];
    const int z = blockIdx.y, tid = threadIdx.x;
    const double* r2 = in.r2[z];
    const double r1 = in.r1[z][0];
    if (blockIdx.x == gridDim.x - 1) {
        double acc = 0.0;
        for (long t = tid; t < npos; t += 256) acc = fma(W[t], r2[t], acc);
        red[tid] = acc;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) red[tid] += red[tid + s];
            __syncthreads();
        }
        if (tid == 0) out.s1[z][0] = d1 * r1 + red[0];
        return;
    }
    const long t = blockIdx.x * 256L + tid;
    if (t >= npos) return;
    const long g = ph[t];
    double v = 0.0;
    if (g >= 0) {
        v = fma(r1, U[t], d2[t] * r2[t]);
        v += G1[g * k + z];
        v += G2[ph_partner[t] * k + z];
        v += H[pair[t] * k + z];
    }
    out.s2[z][t] = v;
}

void qp_check(const char* who, int k, int64_t npos) {
    if (k < 1 || k > kQpMax) throw std::runtime_error(std::string(who) + ": 1 <= k <= 32 vectors per call");
    if (npos < 1 || (npos + 255) / 256 + 1 > 0x7fffffffL) throw std::runtime_error(std::string(who) + ": bad number of positions");
}

// ---- one Arnoldi step on a device-resident basis (include/pymes_amd.h, pymes_sector_arnoldi_step) ---------------------
// Rows 0..j of the basis are orthonormal, row j+1 holds w = H v_j.  Two rounds of classical Gram-Schmidt, cut along the vector
// into chunks of kArnChunkSmall or kArnChunkLarge doubles (by len alone), four launches, no host round trip:
//   dots      p1[c][i] = <V_i, w> on chunk c (one wave per row), wn[c] = |w|^2 on chunk c
//   update 1  h = sum_c p1[c][.]; w' = w - sum_i h_i V_i on chunk c (ascending i); p2[c][i] = <V_i, w'> on the same chunk, which
//             the update has just pulled through the cache
//   update 2  h' = sum_c p2[c][.]; w'' = w' - sum_i h'_i V_i on chunk c; pn[c] = |w''|^2 on chunk c; hess[i,j] = h_i + h'_i
//   scale     |w''|^2 = sum_c pn[c], |w|^2 = sum_c wn[c]; row j+1 = w'' / |w''|, or +0.0 on breakdown; hess[j+1,j]; status
// Every dot is a fixed tree: a lane adds its elements of a chunk in ascending order, a butterfly over the 64 lanes, and the
// chunks one after the other in ascending order -- nothing depends on j, pitch, the grid or the rows allocated.  No atomics.
// Nothing at or beyond len is read or written.
constexpr int kArnMax = PYMES_SECTOR_ARNOLDI_MAX;
constexpr int kArnChunkSmall = 256, kArnChunkLarge = 1024;
constexpr long kArnLargeFrom = 1L << 18;     // len from which the large chunk is taken: below it the small one gives more
                                             // workgroups (a chunk is one workgroup of the update kernels), beyond it the
                                             // partial sums every workgroup adds up again would outgrow its own chunk
constexpr int kArnRowsPerBlock = 16;         // rows of one block of the dots kernel: 4 waves x 4 rows
static_assert(kArnMax == 512, "hs[] below and the header agree on the cap");

__device__ __forceinline__ double arn_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
// <row, w> on one chunk for one wave: lane l takes the elements l, l + 64, ... (nvalid of them exist), w in registers
template <int KPL>
__device__ __forceinline__ double arn_wave_dot(const double* __restrict__ row, const double (&w)[KPL], long nvalid, int lane) {
    double v[KPL];
#pragma unroll
    for (int k = 0; k < KPL; ++k) v[k] = (lane + 64 * k < nvalid) ? row[lane + 64 * k] : 0.0;
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < KPL; ++k) acc = fma(v[k], w[k], acc);
    return arn_wave_sum(acc);
}
// hs[i] = sum_c p[c R + i], c ascending, for the rows 0..j
__device__ __forceinline__ void arn_reduce_rows(const double* __restrict__ p, int nch, int R, int j, double* hs, int tid) {
    for (int i = tid; i <= j; i += 256) {
        double s = 0.0;
        for (int c = 0; c < nch; ++c) s += p[(long)c * R + i];
        hs[i] = s;
    }
}
// sum_c x[c]: thread t over c = t, t + 256, ... ascending, then a fixed tree; every thread gets the sum
__device__ __forceinline__ double arn_block_total(const double* __restrict__ x, int nch, double* red, int tid) {
    double s = 0.0;
    for (int c = tid; c < nch; c += 256) s += x[c];
    __syncthreads();
    red[tid] = s;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) red[tid] += red[tid + st];
        __syncthreads();
    }
    return red[0];
}
// acc[k] = w[e_k] - sum_i hs[i] V_i[e_k], i ascending, for the thread's elements e_k = c0 + tid + 256 k below len (0.0 beyond)
template <int EPT>
__device__ __forceinline__ void arn_update(const double* __restrict__ basis, long pitch, long len, int j, long c0,
                                           const double* hs, double (&acc)[EPT], int tid) {
    // (an element beyond len reads the last valid one instead, so the row loop has no branch, and is set to 0.0 at the end;
    // 16 / EPT rows are unrolled: the loads of 16 elements are in flight before the first fma needs one)
    long at[EPT];
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
        const long e = c0 + tid + 256 * k;
        at[k] = e < len ? e : len - 1;
        acc[k] = (basis + (long)(j + 1) * pitch)[at[k]];
    }
#pragma unroll 16 / EPT
    for (int i = 0; i <= j; ++i) {
        const double* __restrict__ row = basis + (long)i * pitch;
        const double h = hs[i];
#pragma unroll
        for (int k = 0; k < EPT; ++k) acc[k] = fma(-h, row[at[k]], acc[k]);
    }
#pragma unroll
    for (int k = 0; k < EPT; ++k)
        if (c0 + tid + 256 * k >= len) acc[k] = 0.0;
}

template <int KPL>
__global__ void __launch_bounds__(256) sector_arnoldi_dots_kernel(const double* __restrict__ basis, long pitch, long len, int j,
                                                                  int R, double* __restrict__ p1, double* __restrict__ wn) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = blockIdx.x;
    const long c0 = (long)c * (64 * KPL), nvalid = len - c0;
    const double* __restrict__ wrow = basis + (long)(j + 1) * pitch + c0;
    double w[KPL];
#pragma unroll
    for (int k = 0; k < KPL; ++k) w[k] = (lane + 64 * k < nvalid) ? wrow[lane + 64 * k] : 0.0;
    if (blockIdx.y == 0 && wave == 0) {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < KPL; ++k) acc = fma(w[k], w[k], acc);
        acc = arn_wave_sum(acc);
        if (lane == 0) wn[c] = acc;
    }
#pragma unroll
    for (int r = 0; r < kArnRowsPerBlock / 4; ++r) {
        const int i = blockIdx.y * kArnRowsPerBlock + wave + 4 * r;          // (a row past j reads row j and writes nothing: no
        const double d = arn_wave_dot<KPL>(basis + (long)(i <= j ? i : j) * pitch + c0, w, nvalid, lane);     // branch between rows)
        if (lane == 0 && i <= j) p1[(long)c * R + i] = d;
    }
}

template <int EPT>
__global__ void __launch_bounds__(256) sector_arnoldi_first_kernel(double* __restrict__ basis, long pitch, long len, int j, int nch,
                                                                   int R, const double* __restrict__ p1, double* __restrict__ p2,
                                                                   double* __restrict__ h1) {
    __shared__ double hs[kArnMax];
    __shared__ double wl[256 * EPT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = blockIdx.x;
    const long c0 = (long)c * (256 * EPT);
    arn_reduce_rows(p1, nch, R, j, hs, tid);
    __syncthreads();
    if (c == 0)
        for (int i = tid; i <= j; i += 256) h1[i] = hs[i];
    double acc[EPT];
    arn_update<EPT>(basis, pitch, len, j, c0, hs, acc, tid);
    double* __restrict__ wrow = basis + (long)(j + 1) * pitch;
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
        const long e = c0 + tid + 256 * k;
        wl[tid + 256 * k] = acc[k];
        if (e < len) wrow[e] = acc[k];
    }
    __syncthreads();
    constexpr int KPL = 4 * EPT;
    double w[KPL];
#pragma unroll
    for (int k = 0; k < KPL; ++k) w[k] = wl[lane + 64 * k];
    for (int i = wave; i <= j; i += 4) {
        const double d = arn_wave_dot<KPL>(basis + (long)i * pitch + c0, w, len - c0, lane);
        if (lane == 0) p2[(long)c * R + i] = d;
    }
}

template <int EPT>
__global__ void __launch_bounds__(256) sector_arnoldi_second_kernel(double* __restrict__ basis, long pitch, long len, int j, int nch,
                                                                    int R, const double* __restrict__ p2,
                                                                    const double* __restrict__ h1, double* __restrict__ pn,
                                                                    double* __restrict__ hess, long ldh) {
    __shared__ double hs[kArnMax];
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const int c = blockIdx.x;
    const long c0 = (long)c * (256 * EPT);
    arn_reduce_rows(p2, nch, R, j, hs, tid);
    __syncthreads();
    if (c == 0)
        for (int i = tid; i <= j; i += 256) hess[(long)i * ldh + j] = h1[i] + hs[i];
    double acc[EPT];
    arn_update<EPT>(basis, pitch, len, j, c0, hs, acc, tid);
    double* __restrict__ wrow = basis + (long)(j + 1) * pitch;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
        const long e = c0 + tid + 256 * k;
        if (e < len) wrow[e] = acc[k];
        s = fma(acc[k], acc[k], s);
    }
    red[tid] = s;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) red[tid] += red[tid + st];
        __syncthreads();
    }
    if (tid == 0) pn[c] = red[0];
}

template <int EPT>
__global__ void __launch_bounds__(256) sector_arnoldi_scale_kernel(double* __restrict__ basis, long pitch, long len, int j, int nch,
                                                                   const double* __restrict__ wn, const double* __restrict__ pn,
                                                                   double breakdown, double* __restrict__ hess, long ldh,
                                                                   long* __restrict__ status) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const long c0 = (long)blockIdx.x * (256 * EPT);
    const double nrm = sqrt(arn_block_total(pn, nch, red, tid));
    const double wnorm = sqrt(arn_block_total(wn, nch, red, tid));
    const bool broke = !(nrm > breakdown * wnorm);
    double* __restrict__ wrow = basis + (long)(j + 1) * pitch;
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
        const long e = c0 + tid + 256 * k;
        if (e < len) wrow[e] = broke ? 0.0 : wrow[e] / nrm;
    }
    if (blockIdx.x == 0 && tid == 0) {
        hess[(long)(j + 1) * ldh + j] = broke ? 0.0 : nrm;
        if (broke && status[0] == 0) status[0] = j + 1;
    }
}

template <int EPT>
void arnoldi_launch(double* basis, long pitch, long len, int j, int nch, double* hess, long ldh, double breakdown, double* ws,
                    long* status, hipStream_t st) {
    const int R = j + 1;
    double *p1 = ws, *p2 = p1 + (long)nch * R, *wn = p2 + (long)nch * R, *pn = wn + nch, *h1 = pn + nch;
    const dim3 chunks((unsigned)nch), block(256);
    launch_kernel(sector_arnoldi_dots_kernel<4 * EPT>, dim3((unsigned)nch, (unsigned)((R + kArnRowsPerBlock - 1) / kArnRowsPerBlock)),
                  block, 0, st, (const double*)basis, pitch, len, j, R, p1, wn);
    launch_kernel(sector_arnoldi_first_kernel<EPT>, chunks, block, 0, st, basis, pitch, len, j, nch, R, (const double*)p1, p2, h1);
    launch_kernel(sector_arnoldi_second_kernel<EPT>, chunks, block, 0, st, basis, pitch, len, j, nch, R, (const double*)p2,
                  (const double*)h1, pn, hess, ldh);
    launch_kernel(sector_arnoldi_scale_kernel<EPT>, chunks, block, 0, st, basis, pitch, len, j, nch, (const double*)wn,
                  (const double*)pn, breakdown, hess, ldh, status);
}

}  // namespace

namespace dev {

int64_t sector_arnoldi_step(double* basis, int64_t pitch, int64_t len, int j, double* hess, int64_t ldh, double breakdown,
                            double* ws, int64_t ws_doubles, int64_t* status, stream_t s) {
    const std::string who = "sector_arnoldi_step";
    if (len < 1 || len > (1L << 40)) throw std::runtime_error(who + ": bad vector length");
    if (j < 0 || j >= kArnMax) throw std::runtime_error(who + ": j must lie in [0, " + std::to_string(kArnMax) + ")");
    const long chunk = len < kArnLargeFrom ? kArnChunkSmall : kArnChunkLarge;
    const long nch = (len + chunk - 1) / chunk;
    const int64_t need = 2 * nch * (j + 1) + 2 * nch + (j + 1);
    if (!ws) return need;                                   // the query form: nothing is launched
    if (!basis || !hess || !status) throw std::runtime_error(who + ": null argument");
    if (pitch < len || pitch % 32) throw std::runtime_error(who + ": pitch must be a multiple of 32 doubles and at least len");
    if (ldh < j + 1) throw std::runtime_error(who + ": ldh is too small for column j");
    if (!(breakdown >= 0.0) || !std::isfinite(breakdown)) throw std::runtime_error(who + ": the breakdown threshold must be finite and not negative");
    if (ws_doubles < need)
        throw std::runtime_error(who + ": the workspace is too small (" + std::to_string(need) + " doubles are needed)");
    if (chunk == kArnChunkSmall)
        arnoldi_launch<1>(basis, pitch, len, j, (int)nch, hess, ldh, breakdown, ws, reinterpret_cast<long*>(status), (hipStream_t)s);
    else
        arnoldi_launch<4>(basis, pitch, len, j, (int)nch, hess, ldh, breakdown, ws, reinterpret_cast<long*>(status), (hipStream_t)s);
    return need;
}

void sector_gemm(const pymes_sector_task* tasks_dev, int ntask, int64_t ntiles, const double* A, const double* B, double* C,
                 stream_t s) {
    if (ntask < 0 || ntiles < 0 || ntiles > 0x7fffffffL) throw std::runtime_error("sector_gemm: bad task or tile count");
    if (ntask == 0 || ntiles == 0) return;
    if (!tasks_dev || !A || !B || !C) throw std::runtime_error("sector_gemm: null argument");
    launch_kernel(sector_gemm_kernel, dim3((unsigned)ntiles), dim3(256), 0, (hipStream_t)s, tasks_dev, ntask, A, B, C);
}

void sector_ladder_direct(const pymes_sector_task* tasks_dev, int ntask, int64_t ntiles, const int64_t* first_dev,
                          const int32_t* vv_rows_dev, const int32_t* k_int_dev, int n_p, int nterms,
                          const UegLadderTerm* const* terms, const double* coef_host, const double* B, double* C, stream_t s) {
    const std::string who = "sector_ladder_direct";
    if (ntask < 0 || ntiles < 0 || ntiles > 0x7fffffffL) throw std::runtime_error(who + ": bad task or tile count");
    if (nterms < 1 || nterms > kLdTerms)
        throw std::runtime_error(who + ": between 1 and " + std::to_string(kLdTerms) + " terms per call");
    if (!terms || !coef_host) throw std::runtime_error(who + ": null argument");
    LadderTerms T{};
    T.n = nterms;
    for (int q = 0; q < nterms; ++q) {
        if (!terms[q]) throw std::runtime_error(who + ": null term");
        const UegPrepared& p = terms[q]->s;
        if (p.u.n_p != n_p) throw std::runtime_error(who + ": a term was made for another basis (" + std::to_string(p.u.n_p) +
                                                     " orbitals, the call names " + std::to_string(n_p) + ")");
        if (p.u.L != terms[0]->s.u.L) throw std::runtime_error(who + ": the terms were made for different box lengths");
        if (!std::isfinite(coef_host[q])) throw std::runtime_error(who + ": a coefficient is not finite");
        T.coef[q] = coef_host[q];
        T.u[q] = p.u;
        T.umat[q] = p.umat;
        T.uidx[q] = p.uidx;
        T.E[q] = p.E;
    }
    if (ntask == 0 || ntiles == 0) return;
    if (!tasks_dev || !first_dev || !vv_rows_dev || !k_int_dev || !B || !C) throw std::runtime_error(who + ": null argument");
    launch_kernel(sector_ladder_direct_kernel, dim3((unsigned)ntiles), dim3(256), 0, (hipStream_t)s, tasks_dev, ntask,
                  reinterpret_cast<const long*>(first_dev), vv_rows_dev, k_int_dev, T, B, C);
}

void sector_gather(double* dst, int64_t n, double beta, double a1, const double* s1, const int64_t* m1, double a2, const double* s2,
                   const int64_t* m2, stream_t s) {
    if (n < 0) throw std::runtime_error("sector_gather: negative length");
    if (n == 0) return;
    if (!dst || !s1 || !m1 || (s2 && !m2)) throw std::runtime_error("sector_gather: null argument");
    launch_kernel(sector_gather_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)s, dst, (long)n, beta, a1, s1,
                  reinterpret_cast<const long*>(m1), a2, s2, reinterpret_cast<const long*>(m2));
}

void sector_xdiag(const double* Tt, const double* W1, const double* D, double* Ex, const double* eps, double w, int no, int nv,
                  const int64_t* row_start, const int64_t* row_len, const int64_t* row_of, const int64_t* ai_of, double* ws,
                  stream_t s) {
    if (no < 1 || nv < 1) throw std::runtime_error("sector_xdiag: bad orbital counts");
    if (!Tt || !W1 || !D || !Ex || !eps || !row_start || !row_len || !row_of || !ai_of || !ws)
        throw std::runtime_error("sector_xdiag: null argument");
    const long rows = (long)no * nv;
    double* sums = ws;              // rows doubles
    double* x = ws + rows;          // no + nv doubles
    hipStream_t st = (hipStream_t)s;
    const long* start = reinterpret_cast<const long*>(row_start);
    const long* len = reinterpret_cast<const long*>(row_len);
    const unsigned row_blocks = (unsigned)((rows + 255) / 256);
    launch_kernel(sector_rowsum_kernel, dim3(row_blocks), dim3(256), 0, st, Tt, W1, start, len, rows, sums);
    launch_kernel(sector_xdiag_kernel, dim3((unsigned)((no + nv + 63) / 64)), dim3(64), 0, st, (const double*)sums,
                  reinterpret_cast<const long*>(row_of), eps, w, no, nv, x);
    launch_kernel(sector_rowscale_kernel, dim3(row_blocks), dim3(256), 0, st, D, start, len, reinterpret_cast<const long*>(ai_of),
                  rows, (const double*)x, no, Ex);
}

void sector_update(double* t_out, double* dt, const double* t_in, const double* r, const double* den, double shift, int64_t n,
                   stream_t s) {
    if (n < 0) throw std::runtime_error("sector_update: negative length");
    if (n == 0) return;
    if (!t_out || !r || !den) throw std::runtime_error("sector_update: null argument");
    launch_kernel(sector_update_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)s, t_out, dt, t_in, r, den, shift, (long)n);
}

double sector_triples(int no, int nv, const double* eps, const int32_t* k_int, const int32_t* orb_of, const int32_t* box_host,
                      const int32_t* m_of, const double* Tc, const double* Vv, const double* Vo, int64_t t_begin, int64_t t_end,
                      double* ws, int64_t ws_bytes, double* per_triple, stream_t s) {
    return sector_triples_run("sector_triples", no, nv, eps, k_int, orb_of, box_host, m_of, {Tc, Vv, Vo}, nullptr, t_begin, t_end,
                              ws, ws_bytes, per_triple, s);
}

// Lambda-(T): a right-hand slab WR (VvR, VoR, Tc) and a left-hand slab WL (VvL, VoL, Lc) per triple
double sector_triples_lambda(int no, int nv, const double* eps, const int32_t* k_int, const int32_t* orb_of,
                             const int32_t* box_host, const int32_t* m_of, const double* Tc, const double* Lc, const double* VvR,
                             const double* VoR, const double* VvL, const double* VoL, int64_t t_begin, int64_t t_end, double* ws,
                             int64_t ws_bytes, double* per_triple, stream_t s) {
    const TriplesSide left{Lc, VvL, VoL};
    return sector_triples_run("sector_triples_lambda", no, nv, eps, k_int, orb_of, box_host, m_of, {Tc, VvR, VoR}, &left,
                              t_begin, t_end, ws, ws_bytes, per_triple, s);
}

void sector_bin_sums(double* out, int64_t nbins, const int64_t* off, const int64_t* list, const double* src, double alpha,
                     double beta, stream_t s) {
    if (nbins < 0 || nbins > 4 * 0x7fffffffL) throw std::runtime_error("sector_bin_sums: bad bin count");
    if (nbins == 0) return;
    if (!out || !off || !list || !src) throw std::runtime_error("sector_bin_sums: null argument");
    launch_kernel(sector_bin_sums_kernel, dim3((unsigned)((nbins + 3) / 4)), dim3(256), 0, (hipStream_t)s, out, (long)nbins,
                  reinterpret_cast<const long*>(off), reinterpret_cast<const long*>(list), src, alpha, beta);
}

void sector_pair_transfer(double* out, int64_t nbins, const int32_t* bin_q, const int32_t* k_int, const int32_t* orb_of,
                          const int32_t* box_host, int no, int nv, int64_t rows, const int32_t* vv_pairs, const int64_t* row_start,
                          const int64_t* row_len, const int64_t* row_of_pair, const double* lam, const double* T, int max_groups,
                          stream_t s) {
    if (no < 1 || nv < 1 || nv > (1 << 20)) throw std::runtime_error("sector_pair_transfer: bad orbital counts");
    if (nbins < 0 || rows < 0 || max_groups < 0) throw std::runtime_error("sector_pair_transfer: negative count");
    if (nbins == 0) return;
    if (!out || !bin_q || !k_int || !orb_of || !box_host || !vv_pairs || !row_start || !row_len || !row_of_pair || !lam || !T)
        throw std::runtime_error("sector_pair_transfer: null argument");
    const TriplesBox bx = triples_box("sector_pair_transfer", box_host);
    int64_t grid = std::min<int64_t>(nbins, 0x7fffffffL);
    if (max_groups > 0) grid = std::min<int64_t>(grid, max_groups);
    launch_kernel(sector_pair_transfer_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)s, out, (long)nbins, bin_q, k_int,
                  orb_of, bx, no, nv, (long)rows, vv_pairs, reinterpret_cast<const long*>(row_start),
                  reinterpret_cast<const long*>(row_len), reinterpret_cast<const long*>(row_of_pair), lam, T);
}

void sector_gamma(const double* x, const double* y, int no, int nv, const int64_t* row_start, const int64_t* row_len,
                  const int64_t* row_of, double* gamma, double* ws, stream_t s) {
    if (no < 1 || nv < 1) throw std::runtime_error("sector_gamma: bad orbital counts");
    if (!x || !y || !row_start || !row_len || !row_of || !gamma || !ws) throw std::runtime_error("sector_gamma: null argument");
    const long rows = (long)no * nv;
    hipStream_t st = (hipStream_t)s;
    launch_kernel(sector_rowsum_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, x, y,
                  reinterpret_cast<const long*>(row_start), reinterpret_cast<const long*>(row_len), rows, ws);
    launch_kernel(sector_gamma_kernel, dim3((unsigned)((no + nv + 63) / 64)), dim3(64), 0, st, (const double*)ws,
                  reinterpret_cast<const long*>(row_of), no, nv, gamma);
}

void sector_ipea_prepare(int kind, int target, int no, int nv, const int32_t* k_int, const int32_t* orb_of, const int32_t* box_host,
                         const int32_t* b_of, const double* L, const double* Tc, const double* Vv, const double* Vo,
                         const double* VvR, const double* VoR, double outside, double* U, double* W, double* d2, stream_t s) {
    const std::string who = "sector_ipea_prepare";
    if (no < 1 || nv < 1 || nv > (1 << 20)) throw std::runtime_error(who + ": bad orbital counts");
    if (kind != 0 && kind != 1) throw std::runtime_error(who + ": kind must be 0 (IP) or 1 (EA)");
    if (kind == 0 ? (target < 0 || target >= no) : (target < no || target >= no + nv))
        throw std::runtime_error(who + (kind == 0 ? ": the target is not an occupied orbital" : ": the target is not a virtual orbital"));
    if (!k_int || !orb_of || !box_host || !b_of || !L || !Tc || !Vv || !Vo || !VvR || !VoR || !U || !W || !d2)
        throw std::runtime_error(who + ": null argument");
    if (!(outside != 0.0) || !std::isfinite(outside)) throw std::runtime_error(who + ": the value outside the space must be finite and non-zero");
    const TriplesBox bx = triples_box(who, box_host);
    const long npos = (long)(kind == 0 ? no : nv) * no;
    const dim3 grid((unsigned)((npos + 255) / 256));
    launch_kernel(kind == 0 ? sector_qp_prepare_kernel<true> : sector_qp_prepare_kernel<false>, grid, dim3(256), 0, (hipStream_t)s,
                  target, no, nv, k_int, orb_of, bx, b_of, L, Tc, Vv, Vo, VvR, VoR, outside, U, W, d2);
}

void sector_ipea_pack(int k, const double* const* r2, int64_t npos, const int64_t* ph, const int64_t* partner, const int64_t* pair,
                      double* XR, double* XX, double* XP, stream_t s) {
    qp_check("sector_ipea_pack", k, npos);
    if (!r2 || !ph || !partner || !pair || !XR || !XX || !XP) throw std::runtime_error("sector_ipea_pack: null argument");
    QpIn in{};
    for (int z = 0; z < k; ++z) {
        if (!r2[z]) throw std::runtime_error("sector_ipea_pack: null vector");
        in.r2[z] = r2[z];
    }
    launch_kernel(sector_qp_pack_kernel, dim3((unsigned)((npos + 255) / 256), (unsigned)k), dim3(256), 0, (hipStream_t)s, in, k,
                  (long)npos, reinterpret_cast<const long*>(ph), reinterpret_cast<const long*>(partner),
                  reinterpret_cast<const long*>(pair), XR, XX, XP);
}

void sector_ipea_assemble(int k, const double* const* r1, const double* const* r2, double* const* s1, double* const* s2,
                          int64_t npos, const int64_t* ph, const int64_t* ph_partner, const int64_t* pair, const double* d2,
                          const double* U, const double* W, double d1, const double* G1, const double* G2, const double* H,
                          stream_t s) {
    qp_check("sector_ipea_assemble", k, npos);
    if (!r1 || !r2 || !s1 || !s2 || !ph || !ph_partner || !pair || !d2 || !U || !W || !G1 || !G2 || !H)
        throw std::runtime_error("sector_ipea_assemble: null argument");
    QpIn in{};
    QpOut out{};
    for (int z = 0; z < k; ++z) {
        if (!r1[z] || !r2[z] || !s1[z] || !s2[z]) throw std::runtime_error("sector_ipea_assemble: null vector");
        in.r1[z] = r1[z];
        in.r2[z] = r2[z];
        out.s1[z] = s1[z];
        out.s2[z] = s2[z];
    }
    launch_kernel(sector_qp_assemble_kernel, dim3((unsigned)((npos + 255) / 256 + 1), (unsigned)k), dim3(256), 0, (hipStream_t)s, in,
                  out, k, (long)npos, reinterpret_cast<const long*>(ph), reinterpret_cast<const long*>(ph_partner),
                  reinterpret_cast<const long*>(pair), d2, U, W, d1, G1, G2, H);
}

}  // namespace dev
