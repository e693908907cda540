// Kernels of what follows a converged CCSD: the (T) energy, the frozen-natural-orbital density, IP- / EA-EOM-CCSD with the
// Dyson assembly, the Lambda equations with the one-particle and transition densities, the linear response (device_api.h).  Included at the end of
// kernels.hip (one code object for the library), not compiled on its own.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "../../include/pymes_amd.h"      // the PYMES_NOCC_MAX_* limits
#include "device_api.h"
#include "device_util.h"
#include "launch.h"

// ------------------------------------------------------------------------------------
// (T) energy of a batch of occupied triples (cc.cpp, Engine::ccsd_t; include/pymes_amd.h, pymes_ccsd_t)
// ------------------------------------------------------------------------------------
namespace {

// t = i(i+1)(i+2)/6 + j(j+1)/2 + k, i >= j >= k: the library's numbering of the unique triples
__device__ __forceinline__ void unrank_triple(long t, int& i, int& j, int& k) {
    int x = 0;
    while ((long)(x + 1) * (x + 2) * (x + 3) / 6 <= t) ++x;
    long r = t - (long)x * (x + 1) * (x + 2) / 6;
    int y = 0;
    while ((long)(y + 1) * (y + 2) / 2 <= r) ++y;
    i = x;
    j = y;
    k = (int)(r - (long)y * (y + 1) / 2);
}

// One wave per (triple q of the batch, virtual pair a >= b); lane l takes the orbits {a,b,c}, c = l, l + 64, ... <= b.  The six
// permutations of an orbit, P = (abc, bca, cab, cba, acb, bac), are read once each (W, then Y = W + the disconnected term
// formed on the fly); the denominator is the same for all six, and R(Y) on the orbit is
//   R_k = 3 y_k + (sum of the y of k's parity class) - 2 (sum of the other class)      (even: P0..P2, odd: P3..P5),
// so the orbit contributes sum_k w_k R_k / D, divided by the number of times the list repeats a permutation (2 when two
// of a, b, c are equal, 6 when all three are).  The lanes' sums are combined in a fixed order (wave_sum): one double per
// (triple, pair) in `partial`.
__global__ void __launch_bounds__(64) triples_orbit_kernel(const double* __restrict__ W, long t0, const double* __restrict__ Vijab,
                                                           const double* __restrict__ t1, const double* __restrict__ eps,
                                                           double* __restrict__ partial, int no, int nv, long npairs) {
    const long p = blockIdx.x;
    const long q = blockIdx.y;
    int a, b, i, j, k;
    unrank_pair(p, a, b);
    unrank_triple(t0 + q, i, j, k);
    const long v = nv, v2 = v * v;
    const double* __restrict__ Wq = W + q * v2 * v;
    const double dab = eps[i] + eps[j] + eps[k] - eps[no + a] - eps[no + b];
    const double* Vjk = nullptr;
    const double* Vik = nullptr;
    const double* Vij = nullptr;
    double tai = 0.0, tbi = 0.0, taj = 0.0, tbj = 0.0, tak = 0.0, tbk = 0.0;
    if (t1) {
        Vjk = Vijab + ((long)j * no + k) * v2;
        Vik = Vijab + ((long)i * no + k) * v2;
        Vij = Vijab + ((long)i * no + j) * v2;
        tai = t1[(long)a * no + i]; tbi = t1[(long)b * no + i];
        taj = t1[(long)a * no + j]; tbj = t1[(long)b * no + j];
        tak = t1[(long)a * no + k]; tbk = t1[(long)b * no + k];
    }
    double acc = 0.0;
    for (int c = threadIdx.x; c <= b; c += 64) {
        const long A = a, B = b, Cc = c;
        double w[6], y[6];
        w[0] = Wq[A * v2 + B * v + Cc];
        w[1] = Wq[B * v2 + Cc * v + A];
        w[2] = Wq[Cc * v2 + A * v + B];
        w[3] = Wq[Cc * v2 + B * v + A];
        w[4] = Wq[A * v2 + Cc * v + B];
        w[5] = Wq[B * v2 + A * v + Cc];
#pragma unroll
        for (int u = 0; u < 6; ++u) y[u] = w[u];
        if (t1) {
            const double tci = t1[Cc * no + i], tcj = t1[Cc * no + j], tck = t1[Cc * no + k];
            // disc(x,y,z) = V_jk[y,z] t1[x,i] + V_ik[x,z] t1[y,j] + V_ij[x,y] t1[z,k]
            y[0] += Vjk[B * v + Cc] * tai + Vik[A * v + Cc] * tbj + Vij[A * v + B] * tck;     // (a,b,c)
            y[1] += Vjk[Cc * v + A] * tbi + Vik[B * v + A] * tcj + Vij[B * v + Cc] * tak;     // (b,c,a)
            y[2] += Vjk[A * v + B] * tci + Vik[Cc * v + B] * taj + Vij[Cc * v + A] * tbk;     // (c,a,b)
            y[3] += Vjk[B * v + A] * tci + Vik[Cc * v + A] * tbj + Vij[Cc * v + B] * tak;     // (c,b,a)
            y[4] += Vjk[Cc * v + B] * tai + Vik[A * v + B] * tcj + Vij[A * v + Cc] * tbk;     // (a,c,b)
            y[5] += Vjk[A * v + Cc] * tbi + Vik[B * v + Cc] * taj + Vij[B * v + A] * tck;     // (b,a,c)
        }
        const double se = y[0] + y[1] + y[2], so = y[3] + y[4] + y[5];
        const double re = se - 2.0 * so, ro = so - 2.0 * se;
        double s = w[0] * (3.0 * y[0] + re) + w[1] * (3.0 * y[1] + re) + w[2] * (3.0 * y[2] + re) +
                   w[3] * (3.0 * y[3] + ro) + w[4] * (3.0 * y[4] + ro) + w[5] * (3.0 * y[5] + ro);
        const double inv_mult = (a == b && b == c) ? (1.0 / 6.0) : ((a == b || b == c) ? 0.5 : 1.0);
        acc += s * inv_mult / (dab - eps[no + c]);
    }
    acc = wave_sum(acc);
    if (threadIdx.x == 0) partial[q * npairs + p] = acc;
}

// Lambda-CCSD(T) (cc.cpp, Engine::ccsd_t_lambda): the mapping of triples_orbit_kernel with two arrays.  The right triples w_k
// come from WR, the left ones y_k = WL + the disconnected term of l1 (formed on the fly, as above with l1 for t1); the orbit
// contributes sum_k wR_k R_k(yL) / D with the same parity-class form of R and the same multiplicities.
__global__ void __launch_bounds__(64) lambda_triples_orbit_kernel(const double* __restrict__ WR, const double* __restrict__ WL,
                                                                  long t0, const double* __restrict__ Vijab,
                                                                  const double* __restrict__ l1, const double* __restrict__ eps,
                                                                  double* __restrict__ partial, int no, int nv, long npairs) {
    const long p = blockIdx.x;
    const long q = blockIdx.y;
    int a, b, i, j, k;
    unrank_pair(p, a, b);
    unrank_triple(t0 + q, i, j, k);
    const long v = nv, v2 = v * v;
    const double* __restrict__ Rq = WR + q * v2 * v;
    const double* __restrict__ Lq = WL + q * v2 * v;
    const double dab = eps[i] + eps[j] + eps[k] - eps[no + a] - eps[no + b];
    const double* Vjk = nullptr;
    const double* Vik = nullptr;
    const double* Vij = nullptr;
    double lai = 0.0, lbi = 0.0, laj = 0.0, lbj = 0.0, lak = 0.0, lbk = 0.0;
    if (l1) {
        Vjk = Vijab + ((long)j * no + k) * v2;
        Vik = Vijab + ((long)i * no + k) * v2;
        Vij = Vijab + ((long)i * no + j) * v2;
        lai = l1[(long)a * no + i]; lbi = l1[(long)b * no + i];
        laj = l1[(long)a * no + j]; lbj = l1[(long)b * no + j];
        lak = l1[(long)a * no + k]; lbk = l1[(long)b * no + k];
    }
    double acc = 0.0;
    for (int c = threadIdx.x; c <= b; c += 64) {
        const long A = a, B = b, Cc = c;
        const long x[6] = {A * v2 + B * v + Cc, B * v2 + Cc * v + A, Cc * v2 + A * v + B,
                           Cc * v2 + B * v + A, A * v2 + Cc * v + B, B * v2 + A * v + Cc};
        double w[6], y[6];
#pragma unroll
        for (int u = 0; u < 6; ++u) {
            w[u] = Rq[x[u]];
            y[u] = Lq[x[u]];
        }
        if (l1) {
            const double lci = l1[Cc * no + i], lcj = l1[Cc * no + j], lck = l1[Cc * no + k];
            // disc(x,y,z) = V_jk[y,z] l1[x,i] + V_ik[x,z] l1[y,j] + V_ij[x,y] l1[z,k]
            y[0] += Vjk[B * v + Cc] * lai + Vik[A * v + Cc] * lbj + Vij[A * v + B] * lck;     // (a,b,c)
            y[1] += Vjk[Cc * v + A] * lbi + Vik[B * v + A] * lcj + Vij[B * v + Cc] * lak;     // (b,c,a)
            y[2] += Vjk[A * v + B] * lci + Vik[Cc * v + B] * laj + Vij[Cc * v + A] * lbk;     // (c,a,b)
            y[3] += Vjk[B * v + A] * lci + Vik[Cc * v + A] * lbj + Vij[Cc * v + B] * lak;     // (c,b,a)
            y[4] += Vjk[Cc * v + B] * lai + Vik[A * v + B] * lcj + Vij[A * v + Cc] * lbk;     // (a,c,b)
            y[5] += Vjk[A * v + Cc] * lbi + Vik[B * v + Cc] * laj + Vij[B * v + A] * lck;     // (b,a,c)
        }
        const double se = y[0] + y[1] + y[2], so = y[3] + y[4] + y[5];
        const double re = se - 2.0 * so, ro = so - 2.0 * se;
        double s = w[0] * (3.0 * y[0] + re) + w[1] * (3.0 * y[1] + re) + w[2] * (3.0 * y[2] + re) +
                   w[3] * (3.0 * y[3] + ro) + w[4] * (3.0 * y[4] + ro) + w[5] * (3.0 * y[5] + ro);
        const double inv_mult = (a == b && b == c) ? (1.0 / 6.0) : ((a == b || b == c) ? 0.5 : 1.0);
        acc += s * inv_mult / (dab - eps[no + c]);
    }
    acc = wave_sum(acc);
    if (threadIdx.x == 0) partial[q * npairs + p] = acc;
}

// out[q] = m_ijk / 3 * sum_p partial[q][p], summed in a fixed order
__global__ void __launch_bounds__(256) triples_sum_kernel(const double* __restrict__ partial, long t0, long npairs,
                                                          double* __restrict__ out) {
    __shared__ double sh[4];
    const long q = blockIdx.x;
    double s = 0.0;
    for (long p = threadIdx.x; p < npairs; p += 256) s += partial[q * npairs + p];
    s = block_sum(s, sh);
    if (threadIdx.x == 0) {
        int i, j, k;
        unrank_triple(t0 + q, i, j, k);
        const double m = (i == j && j == k) ? 1.0 : ((i == j || j == k) ? 3.0 : 6.0);
        out[q] = m * s / 3.0;
    }
}

}  // namespace

namespace dev {

int64_t triples_partial_doubles(int nv, int64_t nt) { return nt * ((int64_t)nv * (nv + 1) / 2); }

void triples_energy(const double* W, int64_t nt, int64_t t0, const double* Vijab, const double* t1, const double* eps,
                    double* partial, double* out, int no, int nv, stream_t s) {
    if (nt <= 0) return;
    if (!W || !eps || !partial || !out || (t1 && !Vijab)) throw std::runtime_error("triples_energy: null operand");
    const int64_t ntot = (int64_t)no * (no + 1) * (no + 2) / 6;
    if (no < 1 || nv < 1 || t0 < 0 || t0 + nt > ntot) throw std::runtime_error("triples_energy: bad shape or triple range");
    const long npairs = (long)nv * (nv + 1) / 2;
    if (nt > 65535 || npairs > 0x7fffffffL) throw std::runtime_error("triples_energy: grid too large");
    hipStream_t st = (hipStream_t)s;
    launch_kernel(triples_orbit_kernel, dim3((unsigned)npairs, (unsigned)nt), dim3(64), 0, st, W, (long)t0, Vijab, t1, eps,
                 partial, no, nv, npairs);
    launch_kernel(triples_sum_kernel, dim3((unsigned)nt), dim3(256), 0, st, (const double*)partial, (long)t0, npairs, out);
}

void lambda_triples_energy(const double* WR, const double* WL, int64_t nt, int64_t t0, const double* Vijab, const double* l1,
                           const double* eps, double* partial, double* out, int no, int nv, stream_t s) {
    if (nt <= 0) return;
    if (!WR || !WL || !eps || !partial || !out || (l1 && !Vijab)) throw std::runtime_error("lambda_triples_energy: null operand");
    const int64_t ntot = (int64_t)no * (no + 1) * (no + 2) / 6;
    if (no < 1 || nv < 1 || t0 < 0 || t0 + nt > ntot)
        throw std::runtime_error("lambda_triples_energy: bad shape or triple range");
    const long npairs = (long)nv * (nv + 1) / 2;
    if (nt > 65535 || npairs > 0x7fffffffL) throw std::runtime_error("lambda_triples_energy: grid too large");
    hipStream_t st = (hipStream_t)s;
    launch_kernel(lambda_triples_orbit_kernel, dim3((unsigned)npairs, (unsigned)nt), dim3(64), 0, st, WR, WL, (long)t0, Vijab, l1,
                  eps, partial, no, nv, npairs);
    launch_kernel(triples_sum_kernel, dim3((unsigned)nt), dim3(256), 0, st, (const double*)partial, (long)t0, npairs, out);
}

}  // namespace dev

// ---------------------------------------------------------------------------------
// Frozen natural orbitals: the virtual block of the unrelaxed MP2 density and E_MP2 over an occupied window
// ---------------------------------------------------------------------------------
namespace {

// D_ab = 2 sum_K X[a,K] Y[b,K] over K = (i,j,c), i, j in [nf, no), with the amplitudes formed on the fly from V_ijab:
//   X[a,(ijc)] = 2 t[a,c,i,j] - t[c,a,i,j] = (2 V[i,j,a,c] - V[j,i,a,c]) / d_ijac,   Y[b,(ijc)] = t[b,c,i,j] = V[i,j,b,c] / d_ijbc
// (t[c,a,i,j] = V[i,j,c,a] / d = V[j,i,a,c] / d: the exchange symmetry V_pqrs = V_qpsr the caller has checked).  Block = one
// 64 x 64 tile (ta >= tb: D is symmetric, the finish kernel mirrors) and one contiguous split of the flattened K chunks
// (pair (i,j) slow, 32 c fast); wave w computes the 32 x 32 quadrant (w >> 1, w & 1) as 2 x 2 tiles of
// v_mfma_f64_16x16x4_f64 (A: lane holds [row l&15][k l>>4], B: [k l>>4][col l&15], D: col l&15, row (l>>4) + 4 i).  Staging:
// thread t reads c = c0 + (t & 31) of the rows (t >> 5) + 8 h (256-byte row segments), divides by the denominator and writes
// LDS.  The blocks of the column tb = 0 also sum E_MP2 = sum X[a,c] V[i,j,a,c] over their rows.  No atomics: every block
// writes its own partial tile and energy, summed in a fixed order by fno_density_finish_kernel.
constexpr int kFnoT = 64, kFnoK = 32;
__global__ void __launch_bounds__(256) fno_density_kernel(const double* __restrict__ V, const double* __restrict__ eo,
                                                          const double* __restrict__ ev, int no, int nf, int nv, int nt,
                                                          long nchunk, long kc_per, long kc_tot, double* __restrict__ part,
                                                          double* __restrict__ epart) {
    __shared__ double sX[kFnoK][kFnoT + 1], sY[kFnoK][kFnoT + 1];
    __shared__ double sE[256];
    const long ntp = (long)nt * (nt + 1) / 2;
    const long tp = blockIdx.x, split = blockIdx.y;
    int ta, tb;
    unrank_pair(tp, ta, tb);
    const int a0 = ta * kFnoT, b0 = tb * kFnoT;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int wa = (w >> 1) * 32, wb = (w & 1) * 32, l15 = lane & 15, l4 = lane >> 4;
    const int sk = t & 31, sr = t >> 5;
    const long vv = (long)nv * nv;
    const int noa = no - nf;
    const bool do_e = tb == 0;
    const long kc0 = split * kc_per, kc1 = min(kc_tot, kc0 + kc_per);
    v4d acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = v4d{0.0, 0.0, 0.0, 0.0};
    double esum = 0.0;
    for (long kc = kc0; kc < kc1; ++kc) {
        const long pr = kc / nchunk;
        const int c = (int)(kc - pr * nchunk) * kFnoK + sk;
        const int i = nf + (int)(pr / noa), j = nf + (int)(pr % noa);
        const double* __restrict__ Vij = V + ((long)i * no + j) * vv;
        const double* __restrict__ Vji = V + ((long)j * no + i) * vv;
        const bool cok = c < nv;
        const double dc = eo[i] + eo[j] - (cok ? ev[c] : 0.0);
#pragma unroll
        for (int h = 0; h < 8; ++h) {
            const int r = sr + 8 * h, a = a0 + r, b = b0 + r;
            double x = 0.0, y = 0.0;
            if (cok && a < nv) {
                const double vij = Vij[(long)a * nv + c];
                x = (2.0 * vij - Vji[(long)a * nv + c]) / (dc - ev[a]);
                if (do_e) esum += x * vij;
            }
            if (cok && b < nv) y = Vij[(long)b * nv + c] / (dc - ev[b]);
            sX[sk][r] = x;
            sY[sk][r] = y;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kFnoK; kk += 4) {
            const int k = kk + l4;
            const double x0 = sX[k][wa + l15], x1 = sX[k][wa + 16 + l15];
            const double y0 = sY[k][wb + l15], y1 = sY[k][wb + 16 + l15];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(x0, y0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(x0, y1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(x1, y0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(x1, y1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }
    double* __restrict__ P = part + (split * ntp + tp) * (kFnoT * kFnoT);
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int q = 0; q < 4; ++q) P[(wa + 16 * x + l4 + 4 * q) * kFnoT + wb + 16 * y + l15] = acc[x][y][q];
    if (do_e) {
        sE[t] = esum;
        __syncthreads();
        if (t == 0) {
            double s = 0.0;
            for (int q = 0; q < 256; ++q) s += sE[q];
            epart[split * nt + ta] = s;
        }
    }
}

// D[a][b] = 2 sum_split part[split][tile][ra][rb] (the element (max, min) of (a, b) in the tile (max, min) of their row tiles), e = the
// partial energies summed split by split, row tile by row tile
__global__ void __launch_bounds__(256) fno_density_finish_kernel(const double* __restrict__ part, const double* __restrict__ epart,
                                                                 int nv, int nt, long nsplit, double* __restrict__ D,
                                                                 double* __restrict__ e) {
    const long ntp = (long)nt * (nt + 1) / 2;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx == 0) {
        double s = 0.0;
        for (long q = 0; q < nsplit * nt; ++q) s += epart[q];
        e[0] = s;
    }
    if (idx >= (long)nv * nv) return;
    const int a = (int)(idx / nv), b = (int)(idx - (long)a * nv);
    int ta = a / kFnoT, tb = b / kFnoT, ra = a - ta * kFnoT, rb = b - tb * kFnoT;
    if (ta < tb || (ta == tb && ra < rb)) {       // the lower triangle: D is exactly symmetric
        int x = ta; ta = tb; tb = x;
        x = ra; ra = rb; rb = x;
    }
    const long tp = (long)ta * (ta + 1) / 2 + tb, off = (long)ra * kFnoT + rb;
    double s = 0.0;
    for (long q = 0; q < nsplit; ++q) s += part[(q * ntp + tp) * (kFnoT * kFnoT) + off];
    D[idx] = 2.0 * s;
}

struct FnoPlan {
    int nt;
    long ntp, nchunk, kc_tot, kc_per, nsplit;
};
FnoPlan fno_plan(int noa, int nv) {
    FnoPlan p;
    p.nt = (nv + kFnoT - 1) / kFnoT;
    p.ntp = (long)p.nt * (p.nt + 1) / 2;
    p.nchunk = (nv + kFnoK - 1) / kFnoK;
    p.kc_tot = (long)noa * noa * p.nchunk;
    // about 1024 blocks (4 per CU) whatever the size; a function of (noa, nv) only, so two calls, on any device, sum alike
    long want = std::max<long>(1, std::min<long>(std::min<long>((1024 + p.ntp - 1) / p.ntp, p.kc_tot), 65535));
    p.kc_per = (p.kc_tot + want - 1) / want;
    p.nsplit = (p.kc_tot + p.kc_per - 1) / p.kc_per;
    return p;
}

}  // namespace

namespace dev {

int64_t fno_density_partial_doubles(int noa, int nv) {
    const FnoPlan p = fno_plan(noa, nv);
    return p.nsplit * p.ntp * (kFnoT * kFnoT) + p.nsplit * p.nt;
}

void fno_density(const double* Vijab, const double* eps_o, const double* eps_v, int no, int nf, int nv, double* partial,
                 double* D, double* e, stream_t s) {
    if (!Vijab || !eps_o || !eps_v || !partial || !D || !e) throw std::runtime_error("fno_density: null operand");
    if (no < 1 || nv < 1 || nf < 0 || nf >= no) throw std::runtime_error("fno_density: bad shape or occupied window");
    const FnoPlan p = fno_plan(no - nf, nv);
    if (p.ntp > 0x7fffffffL) throw std::runtime_error("fno_density: grid too large");
    double* epart = partial + p.nsplit * p.ntp * (kFnoT * kFnoT);
    hipStream_t st = (hipStream_t)s;
    launch_kernel(fno_density_kernel, dim3((unsigned)p.ntp, (unsigned)p.nsplit), dim3(256), 0, st, Vijab, eps_o, eps_v, no, nf,
                 nv, p.nt, p.nchunk, p.kc_per, p.kc_tot, partial, epart);
    const long nblk = ((long)nv * nv + 255) / 256;
    launch_kernel(fno_density_finish_kernel, dim3((unsigned)nblk), dim3(256), 0, st, (const double*)partial,
                 (const double*)epart, nv, p.nt, p.nsplit, D, e);
}

}  // namespace dev

// ==== IP- / EA-EOM-CCSD (device_api.h; eom.cpp, IpEaSigma) ==============================================================
namespace {

constexpr int kIpeaMax = 16;
struct IpeaIn {          // the k <= 16 vectors of one call, by value
    const double* a[kIpeaMax];
    const double* b[kIpeaMax];
};
struct IpeaOut {
    double* a[kIpeaMax];
    double* b[kIpeaMax];
};

// Operand packing: block (bx, y, z) handles the plane y of vector z and a tile of 8 x by 32 w.  The direct element r2[x,y,w]
// and its exchange partner r2[y,x,w] are both read along w (rows of S doubles) and every output is written along w, so both
// sides are coalesced without a transposing stage; the LDS tile only carries the partner rows so that each is read once for
// the two outputs that need it.  in.a = r1_z, in.b = r2_z.
__global__ void __launch_bounds__(256) ipea_pack_kernel(IpeaIn in, int P, int S, int n1, int k, double* __restrict__ U1,
                                                        double* __restrict__ R, double* __restrict__ Rx, double* __restrict__ Rt,
                                                        double* __restrict__ Rn) {
    __shared__ double sB[8][33];
    const int z = blockIdx.z, y = blockIdx.y;
    const int nwt = (S + 31) / 32;
    const int xt = blockIdx.x / nwt, wt = blockIdx.x - xt * nwt;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int x = xt * 8 + ty, w = wt * 32 + tx;
    const double* __restrict__ r2 = in.b[z];
    const long PS = (long)P * S, n2 = PS * P;
    const bool ok = x < P && w < S;
    double a = 0.0;
    if (ok) {
        a = r2[(long)x * PS + (long)y * S + w];
        sB[ty][tx] = r2[(long)y * PS + (long)x * S + w];
    }
    __syncthreads();
    if (ok) {
        const double b = sB[ty][tx];
        const long o = (long)z * n2 + (long)x * PS + (long)y * S + w;
        R[o] = a;
        Rx[o] = b;
        Rt[o] = 2.0 * a - b;
        if (Rn) Rn[((long)x * P + y) * ((long)k * S) + (long)z * S + w] = a;
    }
    if (blockIdx.x == 0 && y == 0) {
        const double* __restrict__ r1 = in.a[z];
        for (int p = threadIdx.x; p < n1; p += 256) U1[(long)z * n1 + p] = r1[p];
    }
}

// Assembly: s2_z[x,y,w] = D[z,x,y,w] + E[z,y,x,w] + L[x,y,z,w]; all three read along w.  out.a = s1_z, out.b = s2_z.
__global__ void __launch_bounds__(256) ipea_assemble_kernel(IpeaOut out, int P, int S, int n1, int k, const double* __restrict__ D,
                                                            const double* __restrict__ E, const double* __restrict__ L,
                                                            const double* __restrict__ S1) {
    const int z = blockIdx.z, y = blockIdx.y;
    const int nwt = (S + 31) / 32;
    const int xt = blockIdx.x / nwt, wt = blockIdx.x - xt * nwt;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int x = xt * 8 + ty, w = wt * 32 + tx;
    const long PS = (long)P * S, n2 = PS * P;
    if (x < P && w < S) {
        const long o = (long)x * PS + (long)y * S + w;
        double s = D[(long)z * n2 + o] + E[(long)z * n2 + (long)y * PS + (long)x * S + w];
        if (L) s += L[((long)x * P + y) * ((long)k * S) + (long)z * S + w];
        out.b[z][o] = s;
    }
    if (blockIdx.x == 0 && y == 0) {
        double* __restrict__ s1 = out.a[z];
        for (int p = threadIdx.x; p < n1; p += 256) s1[p] = S1[(long)z * n1 + p];
    }
}

__global__ void __launch_bounds__(256) ipea_diagonals_kernel(const double* __restrict__ Loo, const double* __restrict__ Lvv, int kind,
                                                             int no, int nv, double* __restrict__ d1, double* __restrict__ d2,
                                                             long total) {
    const int P = kind ? nv : no, S = kind ? no : nv;
    const double* __restrict__ LP = kind ? Lvv : Loo;
    const double* __restrict__ LS = kind ? Loo : Lvv;
    const double sp = kind ? 1.0 : -1.0;        // IP: L_bb - L_ii - L_jj;  EA: L_aa + L_bb - L_jj
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int w = (int)(idx % S);
        const long xy = idx / S;
        const int y = (int)(xy % P), x = (int)(xy / P);
        d2[idx] = sp * (LP[(long)x * (P + 1)] + LP[(long)y * (P + 1)]) - sp * LS[(long)w * (S + 1)];
        if (idx < P) d1[idx] = sp * LP[idx * (P + 1)];
    }
}

// Davidson correction, stage 1: block (bx, n) owns the elements [bx * kIpeaChunk, (bx + 1) * kIpeaChunk) of root n; its threads
// stride through them, then the 256 partial sums are added pairwise in a fixed tree.  in.a = s_n, in.b = r_n, out.a = q_n.
constexpr long kIpeaChunk = 256 * 16;
struct IpeaW {
    double w[kIpeaMax];
};
__global__ void __launch_bounds__(256) ipea_correction_kernel(IpeaIn in, IpeaOut out, IpeaW ww, const double* __restrict__ d,
                                                              double shift, long n1, long off2, long len, long nblk,
                                                              double* __restrict__ ws) {
    __shared__ double sr[256], sn[256];
    const int n = blockIdx.y, t = threadIdx.x;
    const double* __restrict__ s = in.a[n];
    const double* __restrict__ r = in.b[n];
    double* __restrict__ q = out.a[n];
    const double w = ww.w[n];
    const long e0 = (long)blockIdx.x * kIpeaChunk, e1 = min(len, e0 + kIpeaChunk);
    double res = 0.0, nrm = 0.0;
    for (long e = e0 + t; e < e1; e += 256) {
        if (e >= n1 && e < off2) {
            q[e] = 0.0;
            continue;
        }
        const double re = r[e], x = s[e] - w * re;
        res += x * x;
        nrm += re * re;
        q[e] = x / (w - d[e] + shift);
    }
    sr[t] = res;
    sn[t] = nrm;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) {
            sr[t] += sr[t + h];
            sn[t] += sn[t + h];
        }
        __syncthreads();
    }
    if (t == 0) {
        ws[((long)n * nblk + blockIdx.x) * 2] = sr[0];
        ws[((long)n * nblk + blockIdx.x) * 2 + 1] = sn[0];
    }
}
// stage 2: one block per root; thread t sums the block partials t, t + 256, ... in order, then the same fixed tree
__global__ void __launch_bounds__(256) ipea_correction_final_kernel(const double* __restrict__ ws, long nblk, double* __restrict__ out) {
    __shared__ double sr[256], sn[256];
    const int n = blockIdx.x, t = threadIdx.x;
    double res = 0.0, nrm = 0.0;
    for (long b = t; b < nblk; b += 256) {
        res += ws[((long)n * nblk + b) * 2];
        nrm += ws[((long)n * nblk + b) * 2 + 1];
    }
    sr[t] = res;
    sn[t] = nrm;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) {
            sr[t] += sr[t + h];
            sn[t] += sn[t + h];
        }
        __syncthreads();
    }
    if (t == 0) {
        out[2 * n] = sr[0];
        out[2 * n + 1] = sn[0];
    }
}

// The adjoint of the operand packing: o2_z[x,y,w] = dR[z,x,y,w] + dRx[z,y,x,w] + 2 dRt[z,x,y,w] - dRt[z,y,x,w] + dRn[x,y,z,w]
// (dRn may be null), o1_z = dU1[z].  Same tiling as the assembly: block (bx, y, z) owns the plane y of vector z and 8 x by 32 w;
// the direct rows [z,x,y,:] and the partner rows [z,y,x,:] are both read along w and the output is written along w, so nothing
// is transposed through LDS and no element is written twice.  out.a = o1_z, out.b = o2_z.
__global__ void __launch_bounds__(256) ipea_unpack_kernel(IpeaOut out, int P, int S, int n1, int k, const double* __restrict__ dU1,
                                                          const double* __restrict__ dR, const double* __restrict__ dRx,
                                                          const double* __restrict__ dRt, const double* __restrict__ dRn) {
    const int z = blockIdx.z, y = blockIdx.y;
    const int nwt = (S + 31) / 32;
    const int xt = blockIdx.x / nwt, wt = blockIdx.x - xt * nwt;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int x = xt * 8 + ty, w = wt * 32 + tx;
    const long PS = (long)P * S, n2 = PS * P;
    if (x < P && w < S) {
        const long o = (long)x * PS + (long)y * S + w, p = (long)z * n2 + (long)y * PS + (long)x * S + w;
        double s = dR[(long)z * n2 + o] + dRx[p] + 2.0 * dRt[(long)z * n2 + o] - dRt[p];
        if (dRn) s += dRn[((long)x * P + y) * ((long)k * S) + (long)z * S + w];
        out.b[z][o] = s;
    }
    if (blockIdx.x == 0 && y == 0) {
        double* __restrict__ o1 = out.a[z];
        for (int p = threadIdx.x; p < n1; p += 256) o1[p] = dU1[(long)z * n1 + p];
    }
}

// Dyson amplitudes of k IP / EA roots (device_api.h, ipea_dyson_assemble): block z owns root z.  Stage 1 fills the
// amplitudes over the orbitals of the OTHER kind than the singles (IP: virtuals, EA: occupied) and keeps the right one in LDS;
// stage 2 reads it back for the T1 back-transformation of the singles' own orbitals.  Every element is one thread's sum in a
// fixed order.
struct DysonK {
    dev::DysonParts q;
    int no, nv, kind;
};
__global__ void __launch_bounds__(256) ipea_dyson_kernel(const DysonK k) {
    extern __shared__ double S[];             // the stage-1 right amplitudes [nv] (IP) / [no] (EA)
    const int no = k.no, nv = k.nv, n = no + nv, z = blockIdx.x, t = threadIdx.x;
    const double* __restrict__ t1 = k.q.t1;
    const double* __restrict__ lam1 = k.q.lam1;
    double* __restrict__ pl = k.q.psiL + (long)z * n;
    double* __restrict__ pr = k.q.psiR + (long)z * n;
    if (k.kind == 0) {
        const double* __restrict__ l1 = k.q.L1 + (long)z * no;
        const double* __restrict__ r1 = k.q.R1 + (long)z * no;
        for (int a = t; a < nv; a += 256) {
            double sl = k.q.B[(long)z * nv + a], sr = 0.0;
            for (int i = 0; i < no; ++i) {
                sl += l1[i] * t1[(long)a * no + i];
                sr += lam1[(long)a * no + i] * r1[i];
            }
            sr = 0.5 * sr + k.q.A[(long)z * nv + a];
            S[a] = sr;
            pl[no + a] = sl;
            pr[no + a] = sr;
        }
        __syncthreads();
        for (int j = t; j < no; j += 256) {
            double sr = r1[j] + 0.5 * k.q.C[(long)z * no + j];
            for (int i = 0; i < no; ++i) sr -= k.q.Yoo[(long)j * no + i] * r1[i];
            for (int a = 0; a < nv; ++a) sr -= t1[(long)a * no + j] * S[a];
            pl[j] = l1[j];
            pr[j] = sr;
        }
        return;
    }
    const double* __restrict__ l1 = k.q.L1 + (long)z * nv;
    const double* __restrict__ r1 = k.q.R1 + (long)z * nv;
    for (int i = t; i < no; i += 256) {
        double sl = -k.q.B[(long)z * no + i], sr = 0.0;
        for (int a = 0; a < nv; ++a) {
            sl -= t1[(long)a * no + i] * l1[a];
            sr += r1[a] * lam1[(long)a * no + i];
        }
        sr = -0.5 * sr - k.q.A[(long)z * no + i];
        S[i] = sr;
        pl[i] = sl;
        pr[i] = sr;
    }
    __syncthreads();
    for (int b = t; b < nv; b += 256) {
        double sr = r1[b] + 0.5 * k.q.C[(long)z * nv + b];
        for (int a = 0; a < nv; ++a) sr -= r1[a] * k.q.Yvv[(long)a * nv + b];
        for (int i = 0; i < no; ++i) sr += S[i] * t1[(long)b * no + i];
        pl[no + b] = l1[b];
        pr[no + b] = sr;
    }
}

void ipea_check(const char* who, int k, int P, int S) {
    if (k < 1 || k > kIpeaMax) throw std::runtime_error(std::string(who) + ": 1 <= k <= 16 vectors per call");
    if (P < 1 || S < 1 || P > 65535) throw std::runtime_error(std::string(who) + ": bad shape");
    const long nx = (long)((P + 7) / 8) * ((S + 31) / 32);
    if (nx > 0x7fffffffL) throw std::runtime_error(std::string(who) + ": grid too large");
}

}  // namespace

namespace dev {

void ipea_pack(int k, const double* const* r1, const double* const* r2, int P, int S, int n1, double* U1, double* R, double* Rx,
               double* Rt, double* Rn, stream_t s) {
    ipea_check("ipea_pack", k, P, S);
    if (!r1 || !r2 || !U1 || !R || !Rx || !Rt) throw std::runtime_error("ipea_pack: null operand");
    IpeaIn in{};
    for (int z = 0; z < k; ++z) {
        in.a[z] = r1[z];
        in.b[z] = r2[z];
    }
    const unsigned nx = (unsigned)(((P + 7) / 8) * ((S + 31) / 32));
    launch_kernel(ipea_pack_kernel, dim3(nx, (unsigned)P, (unsigned)k), dim3(256), 0, (hipStream_t)s, in, P, S, n1, k, U1, R, Rx, Rt,
                  Rn);
}

void ipea_assemble(int k, const double* D, const double* E, const double* L, const double* S1, int P, int S, int n1,
                   double* const* s1, double* const* s2, stream_t s) {
    ipea_check("ipea_assemble", k, P, S);
    if (!D || !E || !S1 || !s1 || !s2) throw std::runtime_error("ipea_assemble: null operand");
    IpeaOut out{};
    for (int z = 0; z < k; ++z) {
        out.a[z] = s1[z];
        out.b[z] = s2[z];
    }
    const unsigned nx = (unsigned)(((P + 7) / 8) * ((S + 31) / 32));
    launch_kernel(ipea_assemble_kernel, dim3(nx, (unsigned)P, (unsigned)k), dim3(256), 0, (hipStream_t)s, out, P, S, n1, k, D, E, L,
                  S1);
}

void ipea_unpack(int k, const double* dU1, const double* dR, const double* dRx, const double* dRt, const double* dRn, int P, int S,
                 int n1, double* const* o1, double* const* o2, stream_t s) {
    ipea_check("ipea_unpack", k, P, S);
    if (!dU1 || !dR || !dRx || !dRt || !o1 || !o2) throw std::runtime_error("ipea_unpack: null operand");
    IpeaOut out{};
    for (int z = 0; z < k; ++z) {
        if (!o1[z] || !o2[z]) throw std::runtime_error("ipea_unpack: null output");
        out.a[z] = o1[z];
        out.b[z] = o2[z];
    }
    const unsigned nx = (unsigned)(((P + 7) / 8) * ((S + 31) / 32));
    launch_kernel(ipea_unpack_kernel, dim3(nx, (unsigned)P, (unsigned)k), dim3(256), 0, (hipStream_t)s, out, P, S, n1, k, dU1, dR,
                  dRx, dRt, dRn);
}

void ipea_dyson_assemble(const DysonParts& q, int k, int kind, int no, int nv, stream_t s) {
    if (no < 1 || nv < 1 || k < 1 || (kind != 0 && kind != 1)) throw std::runtime_error("ipea_dyson_assemble: bad shape");
    const size_t lds = sizeof(double) * (size_t)(kind ? no : nv);
    if (lds > 64 * 1024) throw std::runtime_error("ipea_dyson_assemble: too many orbitals for the LDS row");
    if (!q.t1 || !q.lam1 || !q.Yoo || !q.Yvv || !q.L1 || !q.R1 || !q.A || !q.B || !q.C || !q.psiL || !q.psiR)
        throw std::runtime_error("ipea_dyson_assemble: null operand");
    const DysonK kk{q, no, nv, kind};
    launch_kernel(ipea_dyson_kernel, dim3((unsigned)k), dim3(256), lds, (hipStream_t)s, kk);
}

void ipea_diagonals(const double* Loo, const double* Lvv, int kind, int no, int nv, double* d1, double* d2, stream_t s) {
    if (!Loo || !Lvv || !d1 || !d2 || no < 1 || nv < 1) throw std::runtime_error("ipea_diagonals: bad argument");
    const long total = kind ? (long)nv * nv * no : (long)no * no * nv;
    launch_kernel(ipea_diagonals_kernel, dim3(grid_for(total, 256, 256 * 64)), dim3(256), 0, (hipStream_t)s, Loo, Lvv, kind, no, nv,
                  d1, d2, total);
}

int64_t ipea_correction_ws_doubles(int n, int64_t len) { return 2 * (int64_t)n * ((len + kIpeaChunk - 1) / kIpeaChunk); }

void ipea_correction(int n, const double* const* sv, const double* const* rv, const double* w_host, const double* d, double shift,
                     double* const* q, int64_t n1, int64_t off2, int64_t len, double* ws, double* out_dev, stream_t s) {
    if (n < 1 || n > kIpeaMax) throw std::runtime_error("ipea_correction: 1 <= n <= 16 roots per call");
    if (!sv || !rv || !w_host || !d || !q || !ws || !out_dev || len < 1 || n1 < 0 || off2 < n1 || off2 > len)
        throw std::runtime_error("ipea_correction: bad argument");
    const long nblk = (long)((len + kIpeaChunk - 1) / kIpeaChunk);
    if (nblk > 0x7fffffffL) throw std::runtime_error("ipea_correction: grid too large");
    IpeaIn in{};
    IpeaOut out{};
    IpeaW ww{};
    for (int z = 0; z < n; ++z) {
        in.a[z] = sv[z];
        in.b[z] = rv[z];
        out.a[z] = q[z];
        ww.w[z] = w_host[z];
    }
    hipStream_t st = (hipStream_t)s;
    launch_kernel(ipea_correction_kernel, dim3((unsigned)nblk, (unsigned)n), dim3(256), 0, st, in, out, ww, d, shift, (long)n1,
                  (long)off2, (long)len, nblk, ws);
    launch_kernel(ipea_correction_final_kernel, dim3((unsigned)n), dim3(256), 0, st, (const double*)ws, nblk, out_dev);
}

}  // namespace dev

// ==== CCSD Lambda equations and the one-particle density (device_api.h; eom.cpp, EomSigma::apply_left) =================
namespace {

// One block per virtual pair a >= b (the tiling of residual_assemble: every source is read with the thread index along its
// fastest index, the o x o tile in LDS carries the transposition), one extra block for the singles.  With
//   raw_abij = D_abij + cd Pd[(a,i),(b,j)] + Px[(a,j),(b,i)] + cx Pd[(a,j),(b,i)]
// the left sigma is  s2_abij = (raw_abij + raw_baji) / 2 + LS[P(ab)][P(ij)] + sgn(a-b) sgn(i-j) LA[Q(ab)][Q(ij)],  s1 = S1 (LS in
// the rows Lp of pitch lp_ld, LA by strictly-lower pairs in rows of pitch la_ld: the two halves of the packed ladder adjoint).  Without V_ijab that is what is written
// (out1, out2).  With it the block goes on to the Lambda update: eta2_abij = 2 V[i,j,a,b] - V[i,j,b,a] read from the stored
// [o,o,v,v] block (a strided gather of two numbers per element, both index orders from the same two loads),
//   res = eta + s,  out = lam - res / d,  err = -es res / d,  d2 = ev[a] + ev[b] - eo[i] - eo[j] - shift,  d1 = ev[a] - eo[i] - shift
// and ws[block] = sum of res^2 over the block's elements, added pairwise in a fixed tree.  Null partials and a null lam count as zero
// (the start lambda = -eta / d).
struct LambdaK {
    const double* D; const double* Pd; const double* Px; const double* Lp; const double* La; const double* S1;
    const double* Vijab; const double* eta1; const double* eo; const double* ev;
    const double* lam1; const double* lam2;
    double* out1; double* out2; double* err1; double* err2; double* ws;
    double cd, cx, shift, es;
    long lp_ld, la_ld;          // row pitches of Lp / La (the ladder halves of k >= 1 vectors lie side by side)
    int no, nv;
};

__device__ __forceinline__ double lambda_block_sum(double x, double* sr) {
    const int t = threadIdx.x;
    sr[t] = x;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) sr[t] += sr[t + h];
        __syncthreads();
    }
    return sr[0];
}

__global__ void __launch_bounds__(256) lambda_assemble_kernel(const LambdaK k) {
    extern __shared__ double S[];             // [no][no + 1]
    double* sr = S + (long)k.no * (k.no + 1);         // [256], behind the tile
    const int no = k.no, nv = k.nv;
    const bool update = k.Vijab != nullptr;
    const long npairs = (long)nv * (nv + 1) / 2;
    double acc = 0.0;
    if ((long)blockIdx.x == npairs) {         // the singles
        const long n1 = (long)nv * no;
        for (long e = threadIdx.x; e < n1; e += 256) {
            const double s = k.S1 ? k.S1[e] : 0.0;
            if (!update) {
                k.out1[e] = s;
                continue;
            }
            const int a = (int)(e / no), i = (int)(e - (long)a * no);
            const double res = k.eta1[e] + s, dl = -res / (k.ev[a] - k.eo[i] - k.shift);
            acc += res * res;
            k.err1[e] = k.es * dl;
            k.out1[e] = (k.lam1 ? k.lam1[e] : 0.0) + dl;
        }
        if (update) {
            const double tot = lambda_block_sum(acc, sr);
            if (threadIdx.x == 0) k.ws[npairs] = tot;
        }
        return;
    }
    const double* __restrict__ D = k.D;
    const double* __restrict__ Pd = k.Pd;
    const double* __restrict__ Px = k.Px;
    const double cd = k.cd, cx = k.cx;
    int a, b;
    unrank_pair(blockIdx.x, a, b);
    const int p = no + 1;
    const long o2 = (long)no * no, ov = (long)no * nv;
    const long ab = ((long)a * nv + b) * o2, ba = ((long)b * nv + a) * o2;
    const long tab = (long)a * no * ov + (long)b * no, tba = (long)b * no * ov + (long)a * no;
    for (int e = threadIdx.x; e < o2; e += 256) {             // sources read in (i,j) order
        const int i = e / no, j = e - i * no;
        double v = 0.0;
        if (D) {
            const long x = tab + (long)i * ov + j, y = tba + (long)i * ov + j;
            v = D[ab + e] + cd * Pd[x] + Px[y] + cx * Pd[y];
        }
        S[i * p + j] = v;
    }
    __syncthreads();
    if (D) {
        for (int e = threadIdx.x; e < o2; e += 256) {         // sources read in (j,i) order
            const int j = e / no, i = e - j * no;
            const long x = tba + (long)j * ov + i, y = tab + (long)j * ov + i;
            S[i * p + j] += D[ba + e] + cd * Pd[x] + Px[y] + cx * Pd[y];
        }
    }
    __syncthreads();
    const double* __restrict__ row = k.Lp ? k.Lp + ((long)a * (a + 1) / 2 + b) * k.lp_ld : nullptr;
    const double* __restrict__ rowa = (k.La && a != b) ? k.La + ((long)a * (a - 1) / 2 + b) * k.la_ld : nullptr;
    const double ea = update ? k.ev[a] + k.ev[b] - k.shift : 0.0;
    for (int e = threadIdx.x; e < o2; e += 256) {
        const int i = e / no, j = e - i * no;
        const int ih = max(i, j), il = min(i, j);
        double ls = 0.0, la = 0.0;
        if (row) {
            ls = row[(long)ih * (ih + 1) / 2 + il];
            if (rowa && i != j) la = rowa[(long)ih * (ih - 1) / 2 + il];
        }
        const double sgn = i > j ? 1.0 : -1.0;
        const double sab = 0.5 * S[i * p + j] + ls + sgn * la, sba = 0.5 * S[j * p + i] + ls - sgn * la;
        if (!update) {
            k.out2[ab + e] = sab;
            if (a != b) k.out2[ba + e] = sba;
            continue;
        }
        const long vo = (long)e * nv * nv;                    // V_ijab[i,j,:,:]
        const double vab = k.Vijab[vo + (long)a * nv + b], vba = k.Vijab[vo + (long)b * nv + a];
        const double d = ea - k.eo[i] - k.eo[j];
        const double r1 = 2.0 * vab - vba + sab, d1 = -r1 / d;
        acc += r1 * r1;
        k.err2[ab + e] = k.es * d1;
        k.out2[ab + e] = (k.lam2 ? k.lam2[ab + e] : 0.0) + d1;
        if (a != b) {
            const double r2 = 2.0 * vba - vab + sba, d2 = -r2 / d;
            acc += r2 * r2;
            k.err2[ba + e] = k.es * d2;
            k.out2[ba + e] = (k.lam2 ? k.lam2[ba + e] : 0.0) + d2;
        }
    }
    if (update) {
        const double tot = lambda_block_sum(acc, sr);
        if (threadIdx.x == 0) k.ws[blockIdx.x] = tot;
    }
}
// ... and one block adds the block sums: thread t takes t, t + 256, ... in order, then the same fixed tree
__global__ void __launch_bounds__(256) lambda_norm_kernel(const double* __restrict__ ws, long nblk, double* __restrict__ out) {
    __shared__ double sr[256];        // (a kernel of its own: no tile to share the LDS with)
    double x = 0.0;
    for (long b = threadIdx.x; b < nblk; b += 256) x += ws[b];
    const double tot = lambda_block_sum(x, sr);
    if (threadIdx.x == 0) out[0] = tot;
}

// gamma [n,n] (n = no + nv, occupied first) from Xvv[a,c] = sum l2[a,b,i,j] t2[c,b,i,j], Xoo[k,i] = sum l2[a,b,i,j] t2[a,b,k,j],
// Xov[j,b] = sum l1[a,i] (2 t2[a,b,i,j] - t2[a,b,j,i]) and l1, t1 [v,o]; one block per row of gamma:
//   g_oo[j,i] = -2 Xoo[j,i] - sum_a t1[a,j] l1[a,i] (+ ref on the diagonal)   g_ov[j,b] = Xov[j,b] + 2 t1[b,j] + sum_i g'_oo[j,i] t1[b,i] - 2 sum_a t1[a,j] Xvv[a,b]
//   g_vo[a,i] = l1[a,i]                                                        g_vv[a,b] = 2 Xvv[a,b] + sum_i l1[a,i] t1[b,i]
// (g'_oo without the reference term; the row of it is staged in LDS).  Every element is one thread's sum in a fixed order.
__global__ void __launch_bounds__(256) rdm1_assemble_kernel(const double* __restrict__ Xvv, const double* __restrict__ Xoo,
                                                            const double* __restrict__ Xov, const double* __restrict__ l1,
                                                            const double* __restrict__ t1, int no, int nv, double ref,
                                                            double* __restrict__ g) {
    extern __shared__ double row[];           // [no]
    const int n = no + nv, r = blockIdx.x, t = threadIdx.x;
    double* __restrict__ out = g + (long)r * n;
    if (r < no) {
        const int j = r;
        for (int i = t; i < no; i += 256) {
            double s = -2.0 * Xoo[(long)j * no + i];
            for (int a = 0; a < nv; ++a) s -= t1[(long)a * no + j] * l1[(long)a * no + i];
            row[i] = s;
            out[i] = s + (i == j ? ref : 0.0);
        }
        __syncthreads();
        for (int b = t; b < nv; b += 256) {
            double s = Xov[(long)j * nv + b] + 2.0 * t1[(long)b * no + j];
            for (int i = 0; i < no; ++i) s += row[i] * t1[(long)b * no + i];
            for (int a = 0; a < nv; ++a) s -= 2.0 * t1[(long)a * no + j] * Xvv[(long)a * nv + b];
            out[no + b] = s;
        }
        return;
    }
    const int a = r - no;
    for (int i = t; i < no; i += 256) out[i] = l1[(long)a * no + i];
    for (int b = t; b < nv; b += 256) {
        double s = 2.0 * Xvv[(long)a * nv + b];
        for (int i = 0; i < no; ++i) s += l1[(long)a * no + i] * t1[(long)b * no + i];
        out[no + b] = s;
    }
}

// ==== transition densities of the EE-EOM-CCSD roots (device_api.h, tdm1_assemble) =====================================
// grid (n, k, 2): row r of gammaL (blockIdx.z == 0) or gammaR (1) of root z, occupied rows first.  Both sides are the coefficients
// C of the T1-dressed Fock matrix followed by the back-transformation of rdm1_assemble:
//   g_oo[j,i] = C_oo[j,i] - sum_a t1[a,j] C_vo[a,i]      g_ov[j,b] = C_ov[j,b] + sum_i g_oo[j,i] t1[b,i] - sum_a t1[a,j] C_vv[a,b]
//   g_vo[a,i] = C_vo[a,i]                                 g_vv[a,b] = C_vv[a,b] + sum_i C_vo[a,i] t1[b,i]
// left:  C_vo = l1, C_oo = -2 Xoo, C_vv = 2 Xvv, C_ov = Xov.
// right, s = <lambda, r> = sum lam1 r1 + trace Zvv (every block adds it up in the same fixed order):
//   C_vo = Le - s lam1                                    C_oo[j,i] = -sum_a r1[a,j] lam1[a,i] - 2 Zoo[j,i] + 2 s Yoo[j,i]
//   C_vv[a,b] = sum_i lam1[a,i] r1[b,i] + 2 Zvv[a,b] - 2 s Yvv[a,b]
//   C_ov[j,b] = 2 r1[b,j] + Zov[j,b] + Eov[j,b] - s Yov[j,b] - 2 sum_i Yoo[j,i] r1[b,i] - 2 sum_a Yvv[a,b] r1[a,j]
// Every element is one thread's sum in a fixed order; the block of row 0 of the right side writes r0[z] = -s.
struct Tdm1K {
    dev::Tdm1Parts q;
    int no, nv;
};

__global__ void __launch_bounds__(256) tdm1_assemble_kernel(const Tdm1K k) {
    extern __shared__ double S[];             // row [no], row2 [no], the 256 partial sums
    const int no = k.no, nv = k.nv, n = no + nv, r = blockIdx.x, z = blockIdx.y, t = threadIdx.x;
    double* row = S;
    double* row2 = S + no;
    double* sr = S + 2 * no;
    const long n1 = (long)nv * no;
    const double* __restrict__ t1 = k.q.t1;
    if (blockIdx.z == 0) {
        const double* __restrict__ l1 = k.q.L1 + (long)z * n1;
        const double* __restrict__ Xvv = k.q.Xvv + (long)z * nv * nv;
        const double* __restrict__ Xoo = k.q.Xoo + (long)z * no * no;
        const double* __restrict__ Xov = k.q.Xov + (long)z * n1;
        double* __restrict__ out = k.q.gl + ((long)z * n + r) * n;
        if (r < no) {
            const int j = r;
            for (int i = t; i < no; i += 256) {
                double s = -2.0 * Xoo[(long)j * no + i];
                for (int a = 0; a < nv; ++a) s -= t1[(long)a * no + j] * l1[(long)a * no + i];
                row[i] = s;
                out[i] = s;
            }
            __syncthreads();
            for (int b = t; b < nv; b += 256) {
                double s = Xov[(long)j * nv + b];
                for (int i = 0; i < no; ++i) s += row[i] * t1[(long)b * no + i];
                for (int a = 0; a < nv; ++a) s -= 2.0 * t1[(long)a * no + j] * Xvv[(long)a * nv + b];
                out[no + b] = s;
            }
            return;
        }
        const int a = r - no;
        for (int i = t; i < no; i += 256) out[i] = l1[(long)a * no + i];
        for (int b = t; b < nv; b += 256) {
            double s = 2.0 * Xvv[(long)a * nv + b];
            for (int i = 0; i < no; ++i) s += l1[(long)a * no + i] * t1[(long)b * no + i];
            out[no + b] = s;
        }
        return;
    }
    const double* __restrict__ lam1 = k.q.lam1;
    const double* __restrict__ r1 = k.q.R1 + (long)z * n1;
    const double* __restrict__ Le = k.q.Le + (long)z * n1;
    const double* __restrict__ Zvv = k.q.Zvv + (long)z * nv * nv;
    const double* __restrict__ Zoo = k.q.Zoo + (long)z * no * no;
    const double* __restrict__ Zov = k.q.Zov + (long)z * n1;
    const double* __restrict__ Eov = k.q.Eov + (long)z * n1;
    const double* __restrict__ Yvv = k.q.Yvv;
    const double* __restrict__ Yoo = k.q.Yoo;
    const double* __restrict__ Yov = k.q.Yov;
    double* __restrict__ out = k.q.gr + ((long)z * n + r) * n;
    double acc = 0.0;
    for (long e = t; e < n1; e += 256) acc += lam1[e] * r1[e];
    for (int a = t; a < nv; a += 256) acc += Zvv[(long)a * nv + a];
    const double s = lambda_block_sum(acc, sr);
    if (r == 0 && t == 0) k.q.r0[z] = -s;
    if (r < no) {
        const int j = r;
        for (int i = t; i < no; i += 256) {
            double c = -2.0 * Zoo[(long)j * no + i] + 2.0 * s * Yoo[(long)j * no + i], w = 0.0;
            for (int a = 0; a < nv; ++a) {
                const double la = lam1[(long)a * no + i], ta = t1[(long)a * no + j];
                c -= r1[(long)a * no + j] * la + ta * (Le[(long)a * no + i] - s * la);
                w += ta * la;
            }
            row[i] = c;
            row2[i] = w;
            out[i] = c;
        }
        __syncthreads();
        for (int b = t; b < nv; b += 256) {
            double c = 2.0 * r1[(long)b * no + j] + Zov[(long)j * nv + b] + Eov[(long)j * nv + b] - s * Yov[(long)j * nv + b];
            for (int i = 0; i < no; ++i)
                c += row[i] * t1[(long)b * no + i] - (2.0 * Yoo[(long)j * no + i] + row2[i]) * r1[(long)b * no + i];
            for (int a = 0; a < nv; ++a)
                c -= 2.0 * Yvv[(long)a * nv + b] * r1[(long)a * no + j]
                     + 2.0 * t1[(long)a * no + j] * (Zvv[(long)a * nv + b] - s * Yvv[(long)a * nv + b]);
            out[no + b] = c;
        }
        return;
    }
    const int a = r - no;
    for (int i = t; i < no; i += 256) out[i] = Le[(long)a * no + i] - s * lam1[(long)a * no + i];
    for (int b = t; b < nv; b += 256) {
        double c = 2.0 * (Zvv[(long)a * nv + b] - s * Yvv[(long)a * nv + b]);
        for (int i = 0; i < no; ++i) {
            const double la = lam1[(long)a * no + i];
            c += la * r1[(long)b * no + i] + (Le[(long)a * no + i] - s * la) * t1[(long)b * no + i];
        }
        out[no + b] = c;
    }
}

}  // namespace

namespace dev {

int64_t lambda_assemble_ws_doubles(int nv) { return (int64_t)nv * (nv + 1) / 2 + 1; }

constexpr size_t lambda_assemble_lds(size_t no) { return sizeof(double) * (no * (no + 1) + 256); }   // the tile, 256 partial sums behind it
static_assert(lambda_assemble_lds(PYMES_NOCC_MAX_LAMBDA) <= 64 * 1024 && lambda_assemble_lds(PYMES_NOCC_MAX_LAMBDA + 1) > 64 * 1024 &&
              PYMES_NOCC_MAX_LAMBDA <= PYMES_NOCC_MAX_FUSED, "PYMES_NOCC_MAX_LAMBDA is the largest nocc whose tile and partial sums fit 64 KB");
bool lambda_assemble_ok(int no) { return no >= 1 && no <= PYMES_NOCC_MAX_LAMBDA; }

void lambda_assemble(const LambdaParts& q, int no, int nv, stream_t s) {
    if (no < 1 || nv < 1) throw std::runtime_error("lambda_assemble: bad shape");
    const size_t lds = lambda_assemble_lds(no);
    if (!lambda_assemble_ok(no)) throw std::runtime_error("lambda_assemble: nocc too large for the LDS tile");
    if (!q.out1 || !q.out2) throw std::runtime_error("lambda_assemble: null output");
    if (q.D && (!q.Pd || !q.Px || !q.S1)) throw std::runtime_error("lambda_assemble: incomplete partial results");
    if (!q.D && (q.Pd || q.Px || q.S1 || q.Lp || q.La)) throw std::runtime_error("lambda_assemble: partial results without the direct one");
    if ((q.Lp && q.lp_ld < (int64_t)no * (no + 1) / 2) || (q.La && q.la_ld < (int64_t)no * (no - 1) / 2))
        throw std::runtime_error("lambda_assemble: bad row pitch of the ladder halves");
    const bool update = q.Vijab != nullptr;
    if ((q.La && !q.Lp) || (!q.lam1 != !q.lam2)) throw std::runtime_error("lambda_assemble: inconsistent operands");
    if (update && (!q.eta1 || !q.eo || !q.ev || !q.err1 || !q.err2 || !q.ws || !q.norm_dev))
        throw std::runtime_error("lambda_assemble: null operand of the update");
    const long npairs = (long)nv * (nv + 1) / 2;
    if (npairs + 1 > 0x7fffffffL) throw std::runtime_error("lambda_assemble: grid too large");
    const LambdaK k{q.D, q.Pd, q.Px, q.Lp, q.La, q.S1, q.Vijab, q.eta1, q.eo, q.ev, q.lam1, q.lam2, q.out1, q.out2, q.err1, q.err2,
                    q.ws, q.cd, q.cx, q.shift, q.err_scale, (long)q.lp_ld, (long)q.la_ld, no, nv};
    hipStream_t st = (hipStream_t)s;
    launch_kernel(lambda_assemble_kernel, dim3((unsigned)(npairs + 1)), dim3(256), lds, st, k);
    if (update) launch_kernel(lambda_norm_kernel, dim3(1), dim3(256), 0, st, (const double*)q.ws, npairs + 1, q.norm_dev);
}

void rdm1_assemble(const double* Xvv, const double* Xoo, const double* Xov, const double* l1, const double* t1, int no, int nv,
                   double ref, double* g, stream_t s) {
    if (!Xvv || !Xoo || !Xov || !l1 || !t1 || !g) throw std::runtime_error("rdm1_assemble: null operand");
    if (no < 1 || nv < 1 || (size_t)no * sizeof(double) > 64 * 1024) throw std::runtime_error("rdm1_assemble: bad shape");
    launch_kernel(rdm1_assemble_kernel, dim3((unsigned)(no + nv)), dim3(256), sizeof(double) * no, (hipStream_t)s, Xvv, Xoo, Xov,
                  l1, t1, no, nv, ref, g);
}

void tdm1_assemble(const Tdm1Parts& q, int k, int no, int nv, stream_t s) {
    if (no < 1 || nv < 1 || k < 1 || k > 65535) throw std::runtime_error("tdm1_assemble: bad shape");
    const size_t lds = sizeof(double) * (2 * (size_t)no + 256);
    if (lds > 64 * 1024) throw std::runtime_error("tdm1_assemble: nocc too large for the LDS rows");
    if (!q.t1 || !q.lam1 || !q.L1 || !q.R1 || !q.Xvv || !q.Xoo || !q.Xov || !q.Yvv || !q.Yoo || !q.Yov || !q.Zvv || !q.Zoo ||
        !q.Zov || !q.Le || !q.Eov || !q.gl || !q.gr || !q.r0)
        throw std::runtime_error("tdm1_assemble: null operand");
    const Tdm1K kk{q, no, nv};
    launch_kernel(tdm1_assemble_kernel, dim3((unsigned)(no + nv), (unsigned)k, 2u), dim3(256), lds, (hipStream_t)s, kk);
}

}  // namespace dev

// ==== the CCSD two-particle density (device_api.h, rdm2_assemble / rdm2_contract; eom.cpp, lambda_rdm2) ================
namespace {

// Gamma_ijab in the [v,v,o,o] layout, one block per virtual pair a >= b with the o x (o + 1) tile of lambda_assemble.  With
//   g[i,j,a,b] = G[a,b,i,j] + Tt[a,b,i,j] + t[a,i] (2 t[b,j] + D2[b,j]) - t[b,i] (t[a,j] + Cv[a,j])
// (the coefficient of V_ijab[i,j,a,b]: the sum of the products, the energy term, the outer products of the dressed-Fock part)
// out[a,b,i,j] = out[b,a,j,i] = (g[i,j,a,b] + g[j,i,b,a]) / 2.  Pass 1 reads the tiles (a,b) of G and Tt in (i,j) order, pass 2
// the tiles (b,a) in (j,i) order, pass 3 writes both tiles of the output along their fastest index; the LDS tile carries the
// transposition.  Every element is one thread's sum in a fixed order.
struct Rdm2K {
    const double* G; const double* Tt; const double* t1; const double* D2; const double* Cv;
    double* out;
    int no, nv;
};

__global__ void __launch_bounds__(256) rdm2_assemble_kernel(const Rdm2K k) {
    extern __shared__ double S[];             // [no][no + 1]
    const int no = k.no, nv = k.nv;
    int a, b;
    unrank_pair(blockIdx.x, a, b);
    const int p = no + 1;
    const long o2 = (long)no * no;
    const long ab = ((long)a * nv + b) * o2, ba = ((long)b * nv + a) * o2;
    const double* __restrict__ G = k.G;
    const double* __restrict__ Tt = k.Tt;
    const double* __restrict__ ta = k.t1 + (long)a * no;
    const double* __restrict__ tb = k.t1 + (long)b * no;
    const double* __restrict__ da = k.D2 + (long)a * no;
    const double* __restrict__ db = k.D2 + (long)b * no;
    const double* __restrict__ ca = k.Cv + (long)a * no;
    const double* __restrict__ cb = k.Cv + (long)b * no;
    for (int e = threadIdx.x; e < o2; e += 256) {             // sources read in (i,j) order
        const int i = e / no, j = e - i * no;
        S[i * p + j] = G[ab + e] + Tt[ab + e] + ta[i] * (2.0 * tb[j] + db[j]) - tb[i] * (ta[j] + ca[j]);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < o2; e += 256) {             // sources read in (j,i) order
        const int j = e / no, i = e - j * no;
        S[i * p + j] += G[ba + e] + Tt[ba + e] + tb[j] * (2.0 * ta[i] + da[i]) - ta[j] * (tb[i] + cb[i]);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < o2; e += 256) {
        const int r = e / no, c = e - r * no;
        k.out[ab + e] = 0.5 * S[r * p + c];
        if (a != b) k.out[ba + e] = 0.5 * S[c * p + r];
    }
}

// ws[block] = w x the sum of G[e] W[e] over the block's 4096 consecutive elements: thread t takes t, t + 256, ... in order, then
// the fixed tree of lambda_block_sum; rdm2_contract_finish (the second pass of lambda_norm) adds the block sums in order.
constexpr int kRdm2Chunk = 4096;

__global__ void __launch_bounds__(256) rdm2_contract_kernel(const double* __restrict__ G, const double* __restrict__ W, long n,
                                                            double w, double* __restrict__ ws) {
    __shared__ double sr[256];
    const long base = (long)blockIdx.x * kRdm2Chunk;
    double acc = 0.0;
    for (int q = 0; q < kRdm2Chunk / 256; ++q) {
        const long e = base + q * 256 + threadIdx.x;
        if (e < n) acc += G[e] * W[e];
    }
    const double tot = lambda_block_sum(acc, sr);
    if (threadIdx.x == 0) ws[blockIdx.x] = w * tot;
}

// The packed form: sum_abij X[a,b,i,j] R[a,b,i,j] for an exchange-symmetric X [v,v,o,o] and R given pair-packed as ladder_sym
// leaves it — rows P(a,b), a >= b, of length o^2: LS[P(ij)] in the first o (o + 1) / 2 columns, LA[Q(ij)] behind them,
// R[a,b,i,j] = LS + sgn(a-b) sgn(i-j) LA.  One block per row: the tile X[a,b,:,:] is staged in LDS (read along j), column P(i,j)
// meets X_abij + X_abji and column Q(i,j) meets X_abij - X_abji; an off-diagonal pair counts twice (its tile (b,a) is the
// transpose).  ws[row] = the row's sum, fixed tree.
__global__ void __launch_bounds__(256) rdm2_contract_packed_kernel(const double* __restrict__ X, const double* __restrict__ L,
                                                                   int no, int nv, double* __restrict__ ws) {
    extern __shared__ double S[];             // [no][no + 1], the 256 partial sums behind it
    const int p = no + 1;
    double* sr = S + (long)no * p;
    int a, b;
    unrank_pair(blockIdx.x, a, b);
    const long o2 = (long)no * no, opp = (long)no * (no + 1) / 2;
    const double* __restrict__ x = X + ((long)a * nv + b) * o2;
    const double* __restrict__ row = L + (long)blockIdx.x * o2;
    for (int e = threadIdx.x; e < o2; e += 256) {
        const int i = e / no, j = e - i * no;
        S[i * p + j] = x[e];
    }
    __syncthreads();
    double acc = 0.0;
    for (int c = threadIdx.x; c < o2; c += 256) {
        int i, j;
        if (c < opp) {
            unrank_pair(c, i, j);
            acc += row[c] * (i == j ? S[i * p + i] : S[i * p + j] + S[j * p + i]);
        } else if (a != b) {
            unrank_pair(c - opp, i, j);       // Q(i', j) with i' = i + 1 > j
            ++i;
            acc += row[c] * (S[i * p + j] - S[j * p + i]);
        }
    }
    const double tot = lambda_block_sum(acc, sr);
    if (threadIdx.x == 0) ws[blockIdx.x] = (a == b ? 1.0 : 2.0) * tot;
}

}  // namespace

namespace dev {

constexpr size_t rdm2_tile_lds(size_t no) { return sizeof(double) * (no * (no + 1) + 256); }        // the largest of the two kernels
static_assert(rdm2_tile_lds(PYMES_NOCC_MAX_LAMBDA) <= 64 * 1024, "the tile of rdm2_contract_packed fits 64 KB up to PYMES_NOCC_MAX_LAMBDA");
bool rdm2_assemble_ok(int no) { return no >= 1 && no <= PYMES_NOCC_MAX_LAMBDA; }

void rdm2_assemble(const Rdm2Parts& q, int no, int nv, stream_t s) {
    if (no < 1 || nv < 1) throw std::runtime_error("rdm2_assemble: bad shape");
    if (!rdm2_assemble_ok(no)) throw std::runtime_error("rdm2_assemble: nocc too large for the LDS tile");
    if (!q.G || !q.Tt || !q.t1 || !q.D2 || !q.Cv || !q.out) throw std::runtime_error("rdm2_assemble: null operand");
    if (q.out == q.G || q.out == q.Tt) throw std::runtime_error("rdm2_assemble: the output aliases an operand");
    const long npairs = (long)nv * (nv + 1) / 2;
    if (npairs > 0x7fffffffL) throw std::runtime_error("rdm2_assemble: grid too large");
    const Rdm2K k{q.G, q.Tt, q.t1, q.D2, q.Cv, q.out, no, nv};
    launch_kernel(rdm2_assemble_kernel, dim3((unsigned)npairs), dim3(256), sizeof(double) * no * (no + 1), (hipStream_t)s, k);
}

int64_t rdm2_contract_sums(int64_t n) { return (n + kRdm2Chunk - 1) / kRdm2Chunk; }

void rdm2_contract(const double* G, const double* W, int64_t n, double w, double* ws, stream_t s) {
    if (!G || !W || !ws || n < 1) throw std::runtime_error("rdm2_contract: bad argument");
    const int64_t nblk = rdm2_contract_sums(n);
    if (nblk > 0x7fffffffL) throw std::runtime_error("rdm2_contract: grid too large");
    launch_kernel(rdm2_contract_kernel, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)s, G, W, (long)n, w, ws);
}

void rdm2_contract_packed(const double* X, const double* L, int no, int nv, double* ws, stream_t s) {
    if (!X || !L || !ws || no < 1 || nv < 1) throw std::runtime_error("rdm2_contract_packed: bad argument");
    if (!rdm2_assemble_ok(no)) throw std::runtime_error("rdm2_contract_packed: nocc too large for the LDS tile");
    const long npairs = (long)nv * (nv + 1) / 2;
    if (npairs > 0x7fffffffL) throw std::runtime_error("rdm2_contract_packed: grid too large");
    launch_kernel(rdm2_contract_packed_kernel, dim3((unsigned)npairs), dim3(256), rdm2_tile_lds(no), (hipStream_t)s, X, L, no, nv, ws);
}

void rdm2_contract_finish(const double* ws, int64_t nsums, double* out_dev, stream_t s) {
    if (!ws || !out_dev || nsums < 1) throw std::runtime_error("rdm2_contract_finish: bad argument");
    launch_kernel(lambda_norm_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, ws, (long)nsums, out_dev);
}

}  // namespace dev

// ==== EOM-CCSD linear response: the property vectors and the solver's dots / update (device_api.h) =======================
namespace {

constexpr int kRespChunk = 8;            // operators whose accumulators a thread holds while it reads T once
struct RespOut {                         // the k <= 64 outputs of one call, by value
    double* p[dev::kResponseOps];
};
struct RespDoublesK {
    const double* T; const double* M; const double* N; const double* u; const double* w; const double* scal;
    int no, nv, k;
};

// Block (a v + b, chunk): thread t owns the elements e = (i, j) = t, t + 256, ... of the o x o tile of (a, b), for the operators
// z0 .. z0 + 7.  With T exchange-symmetric, S[b,a,j,i] = sum_c M[b,c] T[a,c,i,j] - sum_k N[k,j] T[a,b,i,k]: the four sums are kept
// apart and added at the end, so that the element (b,a,j,i) adds the same four numbers (A1 <-> A2, B1 <-> B2) and the same
// outer products (R1 <-> R2): out is exchange-symmetric to the bit when T is.  Explicit fma only (no contraction of the rest).
__global__ void __launch_bounds__(256) response_doubles_kernel(const RespDoublesK q, const RespOut out) {
#pragma clang fp contract(off)
    const int no = q.no, nv = q.nv;
    const long oo = (long)no * no, vv = (long)nv * nv, vo = (long)nv * no;
    const int a = (int)(blockIdx.x / (unsigned)nv), b = (int)(blockIdx.x % (unsigned)nv);
    const int z0 = (int)blockIdx.y * kRespChunk, nz = min(kRespChunk, q.k - z0);
    const double* __restrict__ T = q.T;
    const double* __restrict__ M = q.M + (long)z0 * vv;
    const double* __restrict__ N = q.N + (long)z0 * oo;
    const double* __restrict__ Tab = T + ((long)a * nv + b) * oo;
    for (long e = threadIdx.x; e < oo; e += 256) {
        const int i = (int)(e / no), j = (int)(e % no);
        double A1[kRespChunk], A2[kRespChunk], B1[kRespChunk], B2[kRespChunk];
#pragma unroll
        for (int z = 0; z < kRespChunk; ++z) A1[z] = A2[z] = B1[z] = B2[z] = 0.0;
        for (int c = 0; c < nv; ++c) {
            const double x1 = T[((long)c * nv + b) * oo + e];       // T[c,b,i,j]
            const double x2 = T[((long)a * nv + c) * oo + e];       // T[a,c,i,j] = T[c,a,j,i]
#pragma unroll
            for (int z = 0; z < kRespChunk; ++z)
                if (z < nz) {
                    A1[z] = fma(M[z * vv + (long)a * nv + c], x1, A1[z]);
                    A2[z] = fma(M[z * vv + (long)b * nv + c], x2, A2[z]);
                }
        }
        for (int k = 0; k < no; ++k) {
            const double y1 = Tab[(long)k * no + j];                // T[a,b,k,j]
            const double y2 = Tab[(long)i * no + k];                // T[a,b,i,k] = T[b,a,k,i]
#pragma unroll
            for (int z = 0; z < kRespChunk; ++z)
                if (z < nz) {
                    B1[z] = fma(N[z * oo + (long)k * no + i], y1, B1[z]);
                    B2[z] = fma(N[z * oo + (long)k * no + j], y2, B2[z]);
                }
        }
        const double tab = Tab[e];
#pragma unroll
        for (int z = 0; z < kRespChunk; ++z)
            if (z < nz) {
                double r = (A1[z] + A2[z]) - (B1[z] + B2[z]);
                if (q.u) {
                    const double* __restrict__ u = q.u;
                    const double* __restrict__ w = q.w + (long)(z0 + z) * vo;
                    const double R1 = u[(long)a * no + i] * w[(long)j * nv + b] - 0.5 * (u[(long)a * no + j] * w[(long)i * nv + b]);
                    const double R2 = u[(long)b * no + j] * w[(long)i * nv + a] - 0.5 * (u[(long)b * no + i] * w[(long)j * nv + a]);
                    r += R1 + R2;
                }
                if (q.scal) r += q.scal[z0 + z] * tab;
                out.p[z0 + z][((long)a * nv + b) * oo + e] = r;
            }
    }
}

struct RespSinglesK {
    dev::ResponseSingles q;
    int no, nv;
};
// One block per operator z.  g0: thread t adds its strided terms of the four blocks in order, then the fixed tree.
__global__ void __launch_bounds__(256) response_singles_kernel(const RespSinglesK k, const RespOut xi1, const RespOut eta1) {
    __shared__ double sr[256];
    const int no = k.no, nv = k.nv, z = blockIdx.x, t = threadIdx.x;
    const long oo = (long)no * no, vv = (long)nv * nv, vo = (long)nv * no;
    const double* __restrict__ Ooo = k.q.Ooo + z * oo;
    const double* __restrict__ Oov = k.q.Oov + z * vo;
    const double* __restrict__ Ovo = k.q.Ovo + z * vo;
    const double* __restrict__ Ovv = k.q.Ovv + z * vv;
    const double* __restrict__ lam1 = k.q.lam1;
    const double* __restrict__ Yoo = k.q.Yoo;
    const double* __restrict__ Yvv = k.q.Yvv;
    const double* __restrict__ Yov = k.q.Yov;
    const double* __restrict__ X1 = k.q.XI1 + z * vo;
    const double* __restrict__ L2X = k.q.L2X + z * vo;
    double s = 0.0;
    for (long e = t; e < vo; e += 256) s += lam1[e] * Ovo[e];
    for (long e = t; e < oo; e += 256) s -= 2.0 * Yoo[e] * Ooo[e];
    for (long e = t; e < vv; e += 256) s += 2.0 * Yvv[e] * Ovv[e];
    for (long e = t; e < vo; e += 256) s += Yov[e] * Oov[e];
    sr[t] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) sr[t] += sr[t + h];
        __syncthreads();
    }
    const double g0 = sr[0];
    if (t == 0) {
        k.q.g0[z] = g0;
        k.q.mg0[z] = -g0;
    }
    double* __restrict__ x1 = xi1.p[z];
    double* __restrict__ e1 = eta1.p[z];
    for (long e = t; e < vo; e += 256) {
        const int c = (int)(e / no), m = (int)(e % no);
        double r = 2.0 * Oov[(long)m * nv + c] + 2.0 * L2X[e] - g0 * lam1[e];
        for (int i = 0; i < no; ++i) r -= lam1[(long)c * no + i] * Ooo[(long)m * no + i];
        for (int a = 0; a < nv; ++a) r += Ovv[(long)a * nv + c] * lam1[(long)a * no + m];
        for (int j = 0; j < no; ++j) r -= 2.0 * Yoo[(long)j * no + m] * Oov[(long)j * nv + c];
        for (int b = 0; b < nv; ++b) r -= 2.0 * Yvv[(long)c * nv + b] * Oov[(long)m * nv + b];
        e1[e] = r;
        x1[e] = X1[e];
    }
}

// ---- the solver's two passes.  Block (bx, s) owns the elements [bx * kRespElems, (bx + 1) * kRespElems) of system s ---------------
constexpr long kRespElems = 256 * 8;
struct Cx {
    double re, im;
};
__device__ __forceinline__ Cx resp_cmul(const Cx a, const Cx b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ double resp_ld(const double* p, long e) { return p ? p[e] : 0.0; }
// q = z p - ap at element e
__device__ __forceinline__ Cx resp_q(const dev::ResponseSystem& S, long e) {
    const Cx p{S.p[0][e], resp_ld(S.p[1], e)}, z{S.z[0], S.z[1]};
    const Cx zp = resp_cmul(z, p);
    return {zp.re - S.ap[0][e], zp.im - resp_ld(S.ap[1], e)};
}
// The dots: a thread keeps q of its kRespPer elements in registers and adds one accumulator pair at a time; each pair is summed
// over the block in a fixed order (block_sum: the wave's shuffle tree, then the four waves in order) — nothing but four doubles of LDS,
// whatever the number of stored directions.
constexpr int kRespPer = (int)(kRespElems / 256);
__global__ void __launch_bounds__(256) response_dots_kernel(const dev::ResponseSystem* __restrict__ sys, long n1, long off2, long len,
                                                            long nblk, double* __restrict__ ws) {
    __shared__ double sh[8];
    const int s = blockIdx.y, t = threadIdx.x;
    const dev::ResponseSystem& S = sys[s];
    const int nh = S.nh;
    const long e0 = (long)blockIdx.x * kRespElems;
    double* __restrict__ dst = ws + ((long)s * nblk + blockIdx.x) * dev::kResponseDots;
    Cx q[kRespPer];
    bool ok[kRespPer];
    double qq = 0.0, cr = 0.0, ci = 0.0;
#pragma unroll
    for (int m = 0; m < kRespPer; ++m) {
        const long e = e0 + t + 256L * m;
        ok[m] = e < len && !(e >= n1 && e < off2);
        q[m] = Cx{0.0, 0.0};
        if (ok[m]) {
            q[m] = resp_q(S, e);
            const double rr = S.r[0][e], ri = resp_ld(S.r[1], e);
            qq += q[m].re * q[m].re + q[m].im * q[m].im;
            cr += q[m].re * rr + q[m].im * ri;
            ci += q[m].re * ri - q[m].im * rr;
        }
    }
    for (int j = 0; j < nh; ++j) {
        double ar = 0.0, ai = 0.0;
#pragma unroll
        for (int m = 0; m < kRespPer; ++m)
            if (ok[m]) {
                const long e = e0 + t + 256L * m;
                const double hr = S.hq[j][0][e], hi = resp_ld(S.hq[j][1], e);
                ar += hr * q[m].re + hi * q[m].im;
                ai += hr * q[m].im - hi * q[m].re;
            }
        ar = block_sum(ar, sh);
        ai = block_sum(ai, sh);
        if (t == 0) {
            dst[2 * j] = ar;
            dst[2 * j + 1] = ai;
        }
    }
    qq = block_sum(qq, sh);
    cr = block_sum(cr, sh);
    ci = block_sum(ci, sh);
    if (t == 0) {
        dst[2 * nh] = qq;
        dst[2 * nh + 1] = 0.0;
        dst[2 * nh + 2] = cr;
        dst[2 * nh + 3] = ci;
    }
}

__global__ void __launch_bounds__(256) response_update_kernel(const dev::ResponseSystem* __restrict__ sys, const double* __restrict__ d,
                                                              double floor, long n1, long off2, long len, long nblk,
                                                              double* __restrict__ ws) {
    __shared__ double sh[8];
    const int s = blockIdx.y, t = threadIdx.x;
    const dev::ResponseSystem& S = sys[s];
    const int nh = S.nh;
    const bool cplx = S.r[1] != nullptr, step = S.p[0] != nullptr;
    const Cx alpha{S.alpha[0], S.alpha[1]};
    const double inv = S.inv;
    double nrm = 0.0;
    const long e0 = (long)blockIdx.x * kRespElems, e1 = min(len, e0 + kRespElems);
    for (long e = e0 + t; e < e1; e += 256) {
        if (e >= n1 && e < off2) {
            S.pn[0][e] = 0.0;
            if (cplx) S.pn[1][e] = 0.0;
            continue;
        }
        Cx r{S.r[0][e], resp_ld(S.r[1], e)};
        if (step) {
            Cx p{S.p[0][e], resp_ld(S.p[1], e)}, q = resp_q(S, e);
            for (int j = 0; j < nh; ++j) {
                const Cx g{S.g[j][0], S.g[j][1]};
                const Cx gp = resp_cmul(g, Cx{S.hp[j][0][e], resp_ld(S.hp[j][1], e)}), gq = resp_cmul(g, Cx{S.hq[j][0][e], resp_ld(S.hq[j][1], e)});
                p.re -= gp.re; p.im -= gp.im;
                q.re -= gq.re; q.im -= gq.im;
            }
            p.re *= inv; p.im *= inv;
            q.re *= inv; q.im *= inv;
            const Cx ap = resp_cmul(alpha, p), aq = resp_cmul(alpha, q);
            r.re -= aq.re; r.im -= aq.im;
            S.x[0][e] += ap.re;
            S.r[0][e] = r.re;
            S.p[0][e] = p.re;
            S.ap[0][e] = q.re;
            if (cplx) {
                S.x[1][e] += ap.im;
                S.r[1][e] = r.im;
                S.p[1][e] = p.im;
                S.ap[1][e] = q.im;
            }
        }
        double x = S.z[0] - d[e];
        const double y = S.z[1];
        if (x * x + y * y < floor * floor) x = copysign(floor, x);
        const double den = x * x + y * y;
        S.pn[0][e] = (r.re * x + r.im * y) / den;
        if (cplx) S.pn[1][e] = (r.im * x - r.re * y) / den;
        nrm += r.re * r.re + r.im * r.im;
    }
    nrm = block_sum(nrm, sh);
    if (t == 0) ws[(long)s * nblk + blockIdx.x] = nrm;
}

// stage 2 of both: one block per system; thread t adds the block partials t, t + 256, ... of one accumulator in order, then
// block_sum.  The dots (sys given) have 2 (nh + 2) accumulators per system, the rest of its row stays as it is; the update has one.
__global__ void __launch_bounds__(256) response_final_kernel(const double* __restrict__ ws, long nblk,
                                                             const dev::ResponseSystem* __restrict__ sys, int stride,
                                                             double* __restrict__ out) {
    __shared__ double sh[8];
    const int s = blockIdx.x, t = threadIdx.x;
    const int nacc = sys ? 2 * (sys[s].nh + 2) : 1;
    for (int m = 0; m < nacc; ++m) {
        double v = 0.0;
        for (long b = t; b < nblk; b += 256) v += ws[((long)s * nblk + b) * stride + m];
        v = block_sum(v, sh);
        if (t == 0) out[(long)s * stride + m] = v;
    }
}

long resp_blocks(int64_t len) { return (long)((len + kRespElems - 1) / kRespElems); }

}  // namespace

namespace dev {

void response_doubles(const double* T, const double* M, const double* N, const double* u, const double* w, const double* scal,
                      int k, int no, int nv, double* const* out, stream_t s) {
    if (no < 1 || nv < 1 || nv > 46340) throw std::runtime_error("response_doubles: bad shape");
    if (k < 1 || k > kResponseOps) throw std::runtime_error("response_doubles: 1 <= k <= 64 operators per call");
    if (!T || !M || !N || !out || (u == nullptr) != (w == nullptr)) throw std::runtime_error("response_doubles: null operand");
    RespOut o{};
    for (int z = 0; z < k; ++z) {
        if (!out[z]) throw std::runtime_error("response_doubles: null output");
        o.p[z] = out[z];
    }
    const RespDoublesK q{T, M, N, u, w, scal, no, nv, k};
    launch_kernel(response_doubles_kernel, dim3((unsigned)(nv * nv), (unsigned)((k + kRespChunk - 1) / kRespChunk)), dim3(256), 0,
                  (hipStream_t)s, q, o);
}

void response_singles(const ResponseSingles& q, int k, int no, int nv, double* const* xi1, double* const* eta1, stream_t s) {
    if (no < 1 || nv < 1) throw std::runtime_error("response_singles: bad shape");
    if (k < 1 || k > kResponseOps) throw std::runtime_error("response_singles: 1 <= k <= 64 operators per call");
    if (!q.Ooo || !q.Oov || !q.Ovo || !q.Ovv || !q.lam1 || !q.Yoo || !q.Yvv || !q.Yov || !q.XI1 || !q.L2X || !q.g0 || !q.mg0 ||
        !xi1 || !eta1)
        throw std::runtime_error("response_singles: null operand");
    RespOut x{}, e{};
    for (int z = 0; z < k; ++z) {
        if (!xi1[z] || !eta1[z]) throw std::runtime_error("response_singles: null output");
        x.p[z] = xi1[z];
        e.p[z] = eta1[z];
    }
    const RespSinglesK kk{q, no, nv};
    launch_kernel(response_singles_kernel, dim3((unsigned)k), dim3(256), 0, (hipStream_t)s, kk, x, e);
}

int64_t response_ws_doubles(int n, int64_t len) { return (int64_t)n * resp_blocks(len) * kResponseDots; }

void response_dots(const ResponseSystem* sys_dev, int n, int64_t n1, int64_t off2, int64_t len, double* ws, double* out_dev,
                   stream_t s) {
    if (n < 1 || n > 65535) throw std::runtime_error("response_dots: 1 <= n <= 65535 systems per call");
    if (!sys_dev || !ws || !out_dev || len < 1 || n1 < 0 || off2 < n1 || off2 > len) throw std::runtime_error("response_dots: bad argument");
    const long nblk = resp_blocks(len);
    if (nblk > 0x7fffffffL) throw std::runtime_error("response_dots: grid too large");
    hipStream_t st = (hipStream_t)s;
    launch_kernel(response_dots_kernel, dim3((unsigned)nblk, (unsigned)n), dim3(256), 0, st, sys_dev, (long)n1, (long)off2, (long)len,
                  nblk, ws);
    launch_kernel(response_final_kernel, dim3((unsigned)n), dim3(256), 0, st, (const double*)ws, nblk, sys_dev, (int)kResponseDots,
                  out_dev);
}

void response_update(const ResponseSystem* sys_dev, int n, const double* d, double floor, int64_t n1, int64_t off2, int64_t len,
                     double* ws, double* out_dev, stream_t s) {
    if (n < 1 || n > 65535) throw std::runtime_error("response_update: 1 <= n <= 65535 systems per call");
    if (!sys_dev || !d || !ws || !out_dev || len < 1 || n1 < 0 || off2 < n1 || off2 > len || !(floor >= 0.0))
        throw std::runtime_error("response_update: bad argument");
    const long nblk = resp_blocks(len);
    if (nblk > 0x7fffffffL) throw std::runtime_error("response_update: grid too large");
    hipStream_t st = (hipStream_t)s;
    launch_kernel(response_update_kernel, dim3((unsigned)nblk, (unsigned)n), dim3(256), 0, st, sys_dev, d, floor, (long)n1, (long)off2,
                  (long)len, nblk, ws);
    launch_kernel(response_final_kernel, dim3((unsigned)n), dim3(256), 0, st, (const double*)ws, nblk,
                  (const ResponseSystem*)nullptr, 1, out_dev);
}

}  // namespace dev
