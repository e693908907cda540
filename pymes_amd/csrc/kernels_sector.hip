// Kernels of the momentum-sector CCD / DCD path (pymes_amd/solver/ueg_cc.py; DESIGN "Momentum sectors"): a ragged batched
// fp64 product over a device-resident task table, the gathers between the three sector layouts, and the element-wise tails.
// Included at the end of kernels.hip (one code object for the library), not compiled on its own.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>

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

}  // namespace

namespace dev {

void sector_gemm(const pymes_sector_task* tasks_dev, int ntask, int64_t ntiles, const double* A, const double* B, double* C,
                 stream_t s) {
    if (ntask < 0 || ntiles < 0 || ntiles > 0x7fffffffL) throw std::runtime_error("sector_gemm: bad task or tile count");
    if (ntask == 0 || ntiles == 0) return;
    if (!tasks_dev || !A || !B || !C) throw std::runtime_error("sector_gemm: null argument");
    launch_kernel(sector_gemm_kernel, dim3((unsigned)ntiles), dim3(256), 0, (hipStream_t)s, tasks_dev, ntask, A, B, C);
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

}  // namespace dev
