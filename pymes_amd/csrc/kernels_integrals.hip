// One-off integral builders behind device_api.h: the TCDUMP scatter and its mean-field foldings, the Hartree-Fock matrix,
// the FCIDUMP fill and the uniform-electron-gas integrals.  None of them runs inside a CCSD iteration.  Included at the end of
// kernels.hip (one code object for the library), not compiled on its own.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "device_api.h"
#include "device_util.h"
#include "launch.h"

namespace {

// ------------------------------------------------------------------------------------
// explicit 3-body operator: TCDUMP scatter (tcdump.py:52-56) and its mean-field foldings (contraction.py:17-95)
// L is dense [nb]^6 in chemists' order (or|ps|qt)
// ------------------------------------------------------------------------------------
__global__ void scatter_kernel(double* __restrict__ dst, const long* __restrict__ idx, const double* __restrict__ val,
                               long n) {
    for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < n; t += (long)gridDim.x * blockDim.x)
        dst[idx[t]] = val[t];                        // targets are unique (the host keeps the last of duplicates)
}

__device__ __forceinline__ double L6(const double* __restrict__ L, int nb, int a, int b, int c, int d, int e, int f) {
    return L[((((long)a * nb + b) * nb + c) * nb + d) * nb * nb + (long)e * nb + f];
}

// D[p,r,q,s] = -1/3 { -3 sum_i (L[p,q,r,i,i,s] + L[r,s,p,i,i,q]) + 6 sum_i L[p,q,r,s,i,i] }     (contraction.py:17-39)
__global__ void tc_single_kernel(const double* __restrict__ L, double* __restrict__ D, int nb, int no, long total) {
    for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
        long x = t;
        const int s = (int)(x % nb); x /= nb;
        const int q = (int)(x % nb); x /= nb;
        const int r = (int)(x % nb);
        const int p = (int)(x / nb);
        double acc = 0.0;
        for (int i = 0; i < no; ++i)
            acc += -3.0 * (L6(L, nb, p, q, r, i, i, s) + L6(L, nb, r, s, p, i, i, q)) + 6.0 * L6(L, nb, p, q, r, s, i, i);
        D[t] = -acc / 3.0;
    }
}

// S[p,q] = -1/6 sum_ij { 12 L[i,i,j,j,p,q] - 12 L[i,i,p,j,j,q] + 6 L[p,i,j,q,i,j] - 6 L[i,j,j,i,p,q] }   (contraction.py:41-65)
__global__ void tc_double_kernel(const double* __restrict__ L, double* __restrict__ S, int nb, int no) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nb * nb) return;
    const int p = t / nb, q = t - p * nb;
    double acc = 0.0;
    for (int i = 0; i < no; ++i)
        for (int j = 0; j < no; ++j)
            acc += 12.0 * L6(L, nb, i, i, j, j, p, q) - 12.0 * L6(L, nb, i, i, p, j, j, q) +
                   6.0 * L6(L, nb, p, i, j, q, i, j) - 6.0 * L6(L, nb, i, j, j, i, p, q);
    S[t] = -acc / 6.0;
}

// T0 = -1/6 sum_ijk { 8 L[i,i,j,j,k,k] - 12 L[i,j,j,i,k,k] + 4 L[i,j,j,k,k,i] }       (contraction.py:67-95)
__global__ void __launch_bounds__(256) tc_triple_kernel(const double* __restrict__ L, double* __restrict__ out, int nb, int no) {
    __shared__ double sh[256];
    double acc = 0.0;
    const long n3 = (long)no * no * no;
    for (long t = threadIdx.x; t < n3; t += blockDim.x) {
        const int k = (int)(t % no), j = (int)((t / no) % no), i = (int)(t / ((long)no * no));
        acc += 8.0 * L6(L, nb, i, i, j, j, k, k) - 12.0 * L6(L, nb, i, j, j, i, k, k) + 4.0 * L6(L, nb, i, j, j, k, k, i);
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = -sh[0] / 6.0;
}

// Hartree-Fock matrix from the packed blocks (hf.py:14-18): f[p,q] = h[p,q] + sum_i (2 V[p,i,q,i] - V[p,i,i,q]), i occupied.
// dir[tp*2+tq] = block (tp, occ, tq, occ), exc[tp*2+tq] = block (tp, occ, occ, tq); tp/tq = 1 for a virtual index.
struct HfBlocks { const double* dir[4]; const double* exc[4]; };
__global__ void hf_fock_kernel(const HfBlocks B, const double* __restrict__ h, double* __restrict__ f, int no, int nv) {
    const int n = no + nv;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * n) return;
    const int p = t / n, q = t - p * n;
    const int tp = p >= no, tq = q >= no;
    const long pl = tp ? p - no : p, ql = tq ? q - no : q, nq = tq ? nv : no;
    const double* __restrict__ D = B.dir[tp * 2 + tq];
    const double* __restrict__ X = B.exc[tp * 2 + tq];
    double acc = 0.0;
    for (long i = 0; i < no; ++i)
        acc += 2.0 * D[((pl * no + i) * nq + ql) * no + i] - X[((pl * no + i) * no + i) * nq + ql];
    f[t] = h[t] + acc;
}

// FCIDUMP lines -> dense V[n]^4 (fcidump.py:140-149): one thread per line writes the symmetry images in the
// reference's order.  A second kernel counts lines whose images do not all hold the line's value afterwards, i.e.
// files whose symmetry-related entries disagree (only there does the order of the lines matter).
__global__ void fcidump_fill_kernel(double* __restrict__ V, const double* __restrict__ val, const int* __restrict__ pqrs,
                                    long count, long n, int is_tc, int verify, unsigned long long* __restrict__ bad) {
    for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < count; t += (long)gridDim.x * blockDim.x) {
        const long p = pqrs[4 * t], q = pqrs[4 * t + 1], r = pqrs[4 * t + 2], s = pqrs[4 * t + 3];
        const double x = val[t];
        long tg[4];
        int m;
        if (is_tc) { tg[0] = ((q * n + p) * n + s) * n + r; tg[1] = ((p * n + q) * n + r) * n + s; m = 2; }
        else {
            tg[0] = ((p * n + q) * n + r) * n + s; tg[1] = ((r * n + q) * n + p) * n + s;
            tg[2] = ((r * n + s) * n + p) * n + q; tg[3] = ((p * n + s) * n + r) * n + q; m = 4;
        }
        if (!verify) {
            for (int i = 0; i < m; ++i) V[tg[i]] = x;
        } else {
            bool ok = true;
            for (int i = 0; i < m; ++i) ok = ok && (V[tg[i]] == x);
            if (!ok) atomicAdd(bad, 1ULL);
        }
    }
}

// ------------------------------------------------------------------------------------
// uniform electron gas integrals (ueg.py:265-596)
// ------------------------------------------------------------------------------------
struct UegK {
    int n_p, n_occ, imax, m, mode, n_ele, lat;
    double L, Omega, kc2g, gamma;
    const double* tab_s;      // correlator tables over m = |n|^2 (device_api.h UegParams); null: evaluated in place
    const double* tab_a;
    int tab_len;
    int kind;                 // 0 trunc, 1 gaskell, 2 gaskell_modified, 3 coulomb, 4 yukawa, 5 stg, 6 smooth
    double p0, p1, p2;
};
// u(k^2) for k = 2 pi n / L: x is the float k^2 the reference would pass, m = |n|^2 its integer shell;
// ARR = the reference calls the correlator with an ndarray there (else with a float)
template <bool ARR>
__device__ __forceinline__ double ueg_u(double x, long m, const UegK& u) {
    if (u.tab_a) return m < u.tab_len ? (ARR ? u.tab_a[m] : u.tab_s[m]) : 0.0;
    switch (u.kind) {
        case 1:                                                         // gaskell, ueg.py:836-883 (p0 = mu, p1 = cut)
            if (ARR) return x > u.p1 ? -0.0 : (x > 1e-12 ? -(u.p0 / x) : -0.0);
            return (x < u.p1 && x > 1e-12) ? -(u.p0 / x) : -0.0;
        case 2:                                                         // gaskell_modified, ueg.py:802-834 (p0 = cut)
            if (ARR) return x >= u.p0 ? -((4.0 * M_PI) / (x * x)) : -0.0;
            return (x < u.p0 && x > 1e-12) ? -0.0 : -((4.0 * M_PI) / (x * x));
        case 3: return x > 1e-12 ? u.p0 / x : 0.0;                      // coulomb, ueg.py:905-915 (p0 = -4 pi gamma)
        case 4: { const double b = x + u.p0; return fabs(b) > u.p1 ? (-4.0 * M_PI) / b : 0.0; }      // yukawa, :740-770
        case 5: { const double t = x + u.p0, b = t * t; return fabs(b) > u.p1 ? u.p2 / b : 0.0; }    // stg, :917-935
        case 6: {                                                       // smooth, ueg.py:885-903
            if (!(x > u.p2)) return 0.0;
            return (-4.0 * M_PI * (1.0 + erf((sqrt(x) - u.p0) / u.p1)) / 2.0) / (x * x);
        }
        default: break;
    }
    if (x <= u.kc2g) x = 0.0;                                           // trunc, ueg.py:772-800
    return x > 1e-12 ? (-4.0 * M_PI / (x * x)) * u.gamma : 0.0;
}
__device__ __forceinline__ double ueg_kp(int k, double L) { return ((double)(k * 2) * M_PI) / L; }   // planewave.py:15

// u_mat[d] = sum_k' (k'.(k-k')) u(k'^2) u((k-k')^2) / Omega, one block per momentum transfer d  (ueg.py:581-596)
__global__ void __launch_bounds__(256) ueg_nabla_kernel(const UegK u, const double* __restrict__ dk, const int* __restrict__ dint,
                                                        double* __restrict__ out) {
    __shared__ double sh[4];
    const double kx = dk[3 * blockIdx.x], ky = dk[3 * blockIdx.x + 1], kz = dk[3 * blockIdx.x + 2];
    const long dx = dint[3 * blockIdx.x], dy = dint[3 * blockIdx.x + 1], dz = dint[3 * blockIdx.x + 2];
    const int w = 2 * u.lat + 1;
    const long total = (long)w * w * w;
    double s = 0.0;
    for (long idx = threadIdx.x; idx < total; idx += blockDim.x) {
        const int c = (int)(idx % w), b = (int)((idx / w) % w), a = (int)(idx / ((long)w * w));
        const double x1 = 2.0 * M_PI * (a - u.lat) / u.L, y1 = 2.0 * M_PI * (b - u.lat) / u.L,
                     z1 = 2.0 * M_PI * (c - u.lat) / u.L;
        const double x2 = kx - x1, y2 = ky - y1, z2 = kz - z1;
        const long a1 = a - u.lat, b1 = b - u.lat, c1 = c - u.lat, a2 = dx - a1, b2 = dy - b1, c2 = dz - c1;
        s += (x1 * x2 + y1 * y2 + z1 * z2) * ueg_u<true>(x1 * x1 + y1 * y1 + z1 * z1, a1 * a1 + b1 * b1 + c1 * c1, u) *
             ueg_u<true>(x2 * x2 + y2 * y2 + z2 * z2, a2 * a2 + b2 * b2 + c2 * c2, u);
    }
    s = block_sum(s, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = s / u.Omega;
}

// per (p,r): the q-independent singly-contracted 3-body value (ueg.py:461-474, 518-573)
__global__ void ueg_effective_kernel(const UegK u, const int* __restrict__ kint, double* __restrict__ E) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= u.n_p * u.n_p) return;
    const int p = idx / u.n_p, r = idx - p * u.n_p;
    double kp[3], kr[3], dk[3];
    long di[3], md = 0;
    for (int c = 0; c < 3; ++c) {
        kp[c] = ueg_kp(kint[3 * p + c], u.L);
        kr[c] = ueg_kp(kint[3 * r + c], u.L);
        dk[c] = kr[c] - kp[c];
        di[c] = kint[3 * r + c] - kint[3 * p + c];
        md += di[c] * di[c];
    }
    const double dk2 = dk[0] * dk[0] + dk[1] * dk[1] + dk[2] * dk[2];
    const double udk_a = ueg_u<true>(dk2, md, u);      // inside contract_exchange_3_body: a 0-d array (ueg.py:536)
    const double udk_s = ueg_u<false>(dk2, md, u);     // in the main loop: a float (ueg.py:409, :461)
    double xr = 0.0, xp = 0.0, pk = 0.0;
    for (int n = 0; n < u.n_occ; ++n) {
        double o[3];
        for (int c = 0; c < 3; ++c) o[c] = ueg_kp(kint[3 * n + c], u.L);
        double a2 = 0, ad = 0, b2 = 0, bd = 0, v12 = 0, v11 = 0;
        long ma = 0, mb = 0, mv = 0;
        for (int c = 0; c < 3; ++c) {
            const double a = kr[c] - o[c], b = kp[c] - o[c], v1 = kr[c] - dk[c] - o[c];
            a2 += a * a; ad += a * dk[c];
            b2 += b * b; bd += b * dk[c];
            v12 += v1 * a; v11 += v1 * v1;
            const long ai = kint[3 * r + c] - kint[3 * n + c], bi = kint[3 * p + c] - kint[3 * n + c], vi = ai - di[c];
            ma += ai * ai; mb += bi * bi; mv += vi * vi;
        }
        xr += ad * udk_a * ueg_u<true>(a2, ma, u);
        xp += bd * udk_a * ueg_u<true>(b2, mb, u);
        pk += v12 * ueg_u<true>(v11, mv, u) * ueg_u<true>(a2, ma, u);
    }
    xr /= u.Omega; xp /= u.Omega; pk /= u.Omega;
    double val;
    if (fabs(dk2) > 0.0) val = -(double)u.n_ele * dk2 * udk_s * udk_s / u.Omega + 2.0 * xr - 2.0 * xp + 2.0 * pk;
    else val = 2.0 * pk;
    E[idx] = val / u.Omega;
}

// One orbital as the element functions below take it: its index, its integer vector and the float momentum 2 pi k / L the
// reference forms from it (ueg_kp) -- from the global table (ueg_orb) or from wherever a kernel has staged it.
struct UegOrb { int idx, k[3]; double kp[3]; };
__device__ __forceinline__ UegOrb ueg_orb(const UegK& u, const int* __restrict__ kint, int idx) {
    UegOrb o;
    o.idx = idx;
    for (int c = 0; c < 3; ++c) {
        o.k[c] = kint[3 * idx + c];
        o.kp[c] = ueg_kp(o.k[c], u.L);
    }
    return o;
}

// V_pqrs of one momentum-conserving element (ueg.py:404-507); umat / E: what ueg_prepare made for modes 1 / 2; d = k_r - k_p
__device__ __forceinline__ double ueg_element(const UegK& u, const double* __restrict__ umat, const int* __restrict__ umat_index,
                                              const double* __restrict__ E, const UegOrb& p, const UegOrb& r, const UegOrb& s,
                                              const int d[3]) {
    const long n = u.n_p;
    double dk[3], dk2 = 0.0;
    long md = 0;
    for (int c = 0; c < 3; ++c) {
        dk[c] = r.kp[c] - p.kp[c];
        dk2 += dk[c] * dk[c];
        md += (long)d[c] * d[c];
    }
    double w = 0.0;
    if (u.mode == 0) {
        if (fabs(dk2) > 0.0) w = 4.0 * M_PI / dk2 / u.Omega;
    } else if (u.mode == 3) {
        if (fabs(dk2) > 0.0) { const double x = ueg_u<false>(dk2, md, u); w = -(double)u.n_ele * dk2 * x * x / u.Omega / u.Omega; }
    } else if (u.mode == 1) {
        const int w4 = 4 * u.imax + 1;
        const double um = umat[umat_index[((long)(d[0] + 2 * u.imax) * w4 + (d[1] + 2 * u.imax)) * w4 + d[2] + 2 * u.imax]];
        if (fabs(dk2) > 0.0) {
            double rsdk = 0.0;
            for (int c = 0; c < 3; ++c) rsdk += (r.kp[c] - s.kp[c]) * dk[c];
            const double x = ueg_u<false>(dk2, md, u);
            w = (4.0 * M_PI / dk2 + um + dk2 * x - rsdk * x) / u.Omega;
        } else {
            w = um / u.Omega;
        }
    } else {
        w = E[(long)p.idx * n + r.idx];
    }
    return w;
}

// <pq|rs> as the list form defines it (include/pymes_amd.h, pymes_ueg_eval_2b_list): conservation decided in exact integer
// arithmetic (an entry that does not conserve the vector is 0); mode 2 already symmetrised, (E[p,r] + E[q,s]) / 2.  The one
// body of ueg_list_kernel and of the direct sector ladder (kernels_sector.hip), which therefore agree to the bit.
__device__ __forceinline__ double ueg_pair_element(const UegK& u, const double* __restrict__ umat,
                                                   const int* __restrict__ umat_index, const double* __restrict__ E,
                                                   const UegOrb& p, const UegOrb& q, const UegOrb& r, const UegOrb& s) {
    int d[3], e[3];
    bool ok = true;
    for (int c = 0; c < 3; ++c) {
        d[c] = r.k[c] - p.k[c];
        e[c] = s.k[c] - q.k[c];
        ok = ok && d[c] + e[c] == 0;
    }
    double w = 0.0;
    if (ok) {
        w = ueg_element(u, umat, umat_index, E, p, r, s, d);
        if (u.mode == 2) w = 0.5 * w + 0.5 * ueg_element(u, umat, umat_index, E, q, s, r, e);
    }
    return w;
}

// one thread per (p,q,r): s by momentum conservation through the flattened lookup (ueg.py:384-507)
__global__ void ueg_scatter_kernel(const UegK u, const int* __restrict__ kint, const int* __restrict__ map,
                                   const double* __restrict__ umat, const int* __restrict__ umat_index,
                                   const double* __restrict__ E, double* __restrict__ V) {
    const long idx = blockIdx.x * (long)blockDim.x + threadIdx.x;
    const long n = u.n_p;
    if (idx >= n * n * n) return;
    const int r = (int)(idx % n), q = (int)((idx / n) % n), p = (int)(idx / (n * n));
    int d[3], ks[3];
    for (int c = 0; c < 3; ++c) {
        d[c] = kint[3 * r + c] - kint[3 * p + c];
        ks[c] = kint[3 * q + c] - d[c];
    }
    const long loc = (long)u.m * u.m * (ks[0] + u.imax) + (long)u.m * (ks[1] + u.imax) + ks[2] + u.imax;
    if (loc < 0 || loc >= (long)u.m * u.m * u.m) return;     // only the flattened index is range-checked (:397)
    const int s = map[loc];
    if (s < 0 || s >= u.n_p) return;
    V[((long)(p * n + q) * n + r) * n + s] =
        ueg_element(u, umat, umat_index, E, ueg_orb(u, kint, p), ueg_orb(u, kint, r), ueg_orb(u, kint, s), d);
}

// one thread per listed (p,q,r,s): ueg_pair_element of the entry; one that names no orbital is NaN
__global__ void ueg_list_kernel(const UegK u, const int* __restrict__ kint, const double* __restrict__ umat,
                                const int* __restrict__ umat_index, const double* __restrict__ E, const int* __restrict__ pqrs,
                                long count, double* __restrict__ out) {
    const long t = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (t >= count) return;
    const int p = pqrs[4 * t], q = pqrs[4 * t + 1], r = pqrs[4 * t + 2], s = pqrs[4 * t + 3];
    if (p < 0 || q < 0 || r < 0 || s < 0 || p >= u.n_p || q >= u.n_p || r >= u.n_p || s >= u.n_p) { out[t] = nan(""); return; }
    out[t] = ueg_pair_element(u, umat, umat_index, E, ueg_orb(u, kint, p), ueg_orb(u, kint, q), ueg_orb(u, kint, r),
                              ueg_orb(u, kint, s));
}

// What the integral kernels read besides the orbitals' vectors, prepared once: the kernel parameters, the correlator tables,
// for mode 1 the u_mat table over the distinct momentum transfers with its index, for mode 2 E[p,r].  It lives until
// ueg_release: for one fill (the dense and the list builder) or as long as a ladder term (dev::UegLadderTerm).
struct UegPrepared {
    UegK u;
    double *umat = nullptr, *E = nullptr, *tabs = nullptr;
    int* uidx = nullptr;
    int64_t bytes = 0;          // device bytes held
};
void ueg_release(UegPrepared& s) {
    dev::dfree(s.umat); dev::dfree(s.E); dev::dfree(s.uidx); dev::dfree(s.tabs);
    s.umat = s.E = s.tabs = nullptr;
    s.uidx = nullptr;
    s.bytes = 0;
}
// Returns with the tables complete (the stream has drained): the temporaries of the u_mat build are gone.
UegPrepared ueg_prepare(const dev::UegParams& prm, const int* k_int_dev, hipStream_t st) {
    UegPrepared s;
    UegK& u = s.u;
    u.n_p = prm.n_p; u.n_occ = prm.n_ele / 2; u.imax = prm.imax; u.m = 2 * prm.imax + 1; u.mode = prm.mode;
    u.n_ele = prm.n_ele; u.lat = prm.lattice_cutoff; u.L = prm.L; u.Omega = prm.Omega; u.gamma = prm.gamma;
    const double kc = prm.k_cutoff * 2 * M_PI / prm.L;
    u.kc2g = kc * kc * (1 + 0.00001);
    u.tab_s = u.tab_a = nullptr;
    u.tab_len = 0;
    u.kind = prm.corr_kind; u.p0 = prm.corr_p[0]; u.p1 = prm.corr_p[1]; u.p2 = prm.corr_p[2];
    if (u.kind < 0 || u.kind > 6) throw std::runtime_error("ueg: unknown correlator kind");
    const long n = prm.n_p;
    double* dk_dev = nullptr;
    int* dint_dev = nullptr;
    try {
        if (prm.tab_array) {
            if (!prm.tab_scalar || prm.tab_len < 1) throw std::runtime_error("ueg: both correlator tables are needed");
            s.tabs = (double*)dev::dmalloc(sizeof(double) * 2 * prm.tab_len);
            s.bytes += sizeof(double) * 2 * prm.tab_len;
            HIP_CHECK(copy_async(s.tabs, prm.tab_scalar, sizeof(double) * prm.tab_len, hipMemcpyHostToDevice, st));
            HIP_CHECK(copy_async(s.tabs + prm.tab_len, prm.tab_array, sizeof(double) * prm.tab_len, hipMemcpyHostToDevice, st));
            u.tab_s = s.tabs; u.tab_a = s.tabs + prm.tab_len; u.tab_len = prm.tab_len;
        }
        std::vector<int> kint(3 * n);
        HIP_CHECK(copy_async(kint.data(), k_int_dev, sizeof(int) * 3 * n, hipMemcpyDeviceToHost, st));
        wait_idle(st);
        if (prm.mode == 1) {
            // distinct momentum transfers d = k_r - k_p, with the float d_k of their first (p,r) pair
            const int w4 = 4 * prm.imax + 1;
            std::vector<int> index((size_t)w4 * w4 * w4, -1);
            std::vector<double> dks;
            std::vector<int> dints;
            for (long p = 0; p < n; ++p)
                for (long r = 0; r < n; ++r) {
                    int d[3];
                    for (int c = 0; c < 3; ++c) {
                        d[c] = kint[3 * r + c] - kint[3 * p + c];
                        if (d[c] < -2 * prm.imax || d[c] > 2 * prm.imax) throw std::runtime_error("ueg: k outside the index map");
                    }
                    int& slot = index[((size_t)(d[0] + 2 * prm.imax) * w4 + (d[1] + 2 * prm.imax)) * w4 + d[2] + 2 * prm.imax];
                    if (slot < 0) {
                        slot = (int)(dks.size() / 3);
                        for (int c = 0; c < 3; ++c) dints.push_back(d[c]);
                        for (int c = 0; c < 3; ++c)
                            dks.push_back(((double)(kint[3 * r + c] * 2) * M_PI) / prm.L - ((double)(kint[3 * p + c] * 2) * M_PI) / prm.L);
                    }
                }
            const int nd = (int)(dks.size() / 3);
            s.umat = (double*)dev::dmalloc(sizeof(double) * nd);
            dk_dev = (double*)dev::dmalloc(sizeof(double) * 3 * nd);
            s.uidx = (int*)dev::dmalloc(sizeof(int) * index.size());
            dint_dev = (int*)dev::dmalloc(sizeof(int) * 3 * nd);
            s.bytes += sizeof(double) * nd + sizeof(int) * index.size();
            HIP_CHECK(copy_async(dint_dev, dints.data(), sizeof(int) * 3 * nd, hipMemcpyHostToDevice, st));
            HIP_CHECK(copy_async(dk_dev, dks.data(), sizeof(double) * 3 * nd, hipMemcpyHostToDevice, st));
            HIP_CHECK(copy_async(s.uidx, index.data(), sizeof(int) * index.size(), hipMemcpyHostToDevice, st));
            launch_kernel(ueg_nabla_kernel, dim3(nd), dim3(256), 0, st, u, dk_dev, dint_dev, s.umat);
        } else if (prm.mode == 2) {
            s.E = (double*)dev::dmalloc(sizeof(double) * n * n);
            s.bytes += sizeof(double) * n * n;
            launch_kernel(ueg_effective_kernel, dim3((unsigned)((n * n + 255) / 256)), dim3(256), 0, st, u, k_int_dev, s.E);
        }
        wait_idle(st);          // (the host lists above and the two temporaries are read by the stream until here)
    } catch (...) {
        dev::dfree(dk_dev); dev::dfree(dint_dev);
        ueg_release(s);
        throw;
    }
    dev::dfree(dk_dev); dev::dfree(dint_dev);
    return s;
}

}  // namespace

namespace dev {

void scatter(double* dst, const int64_t* idx_host, const double* val_host, int64_t n, stream_t s) {
    if (n <= 0) return;
    long* idx = nullptr;
    double* val = nullptr;
    HIP_CHECK(hipMalloc(&idx, sizeof(long) * n));
    if (hipMalloc(&val, sizeof(double) * n) != hipSuccess) { (void)free_device(idx); throw std::runtime_error("scatter: out of device memory"); }
    hipStream_t st = (hipStream_t)s;
    HIP_CHECK(copy_async(idx, idx_host, sizeof(long) * n, hipMemcpyHostToDevice, st));
    HIP_CHECK(copy_async(val, val_host, sizeof(double) * n, hipMemcpyHostToDevice, st));
    const hipError_t e = try_launch_kernel(scatter_kernel, dim3(grid_for(n)), dim3(256), 0, st, dst, idx, val, (long)n);
    (void)sync_stream(st);
    (void)free_device(idx);
    (void)free_device(val);
    HIP_CHECK(e);
}

void hf_fock(const double* const dir[4], const double* const exc[4], const double* h_dev, double* f_dev, int no, int nv,
             stream_t s) {
    HfBlocks B;
    for (int i = 0; i < 4; ++i) { B.dir[i] = dir[i]; B.exc[i] = exc[i]; }
    const int n = no + nv;
    launch_kernel(hf_fock_kernel, dim3((n * n + 255) / 256), dim3(256), 0, (hipStream_t)s, B, h_dev, f_dev, no, nv);
}

int64_t fcidump_fill(double* V, const double* val_host, const int32_t* pqrs_host, int64_t count, int n, bool is_tc,
                     stream_t s) {
    if (count <= 0) return 0;
    hipStream_t st = (hipStream_t)s;
    const int64_t chunk = 1 << 22;                      // lines per upload
    double* dval = nullptr;
    int* didx = nullptr;
    unsigned long long* dbad = nullptr;
    unsigned long long bad = 0;
    HIP_CHECK(hipMalloc(&dval, sizeof(double) * std::min(count, chunk)));
    if (hipMalloc(&didx, sizeof(int) * 4 * std::min(count, chunk)) != hipSuccess || hipMalloc(&dbad, sizeof(bad)) != hipSuccess) {
        (void)free_device(dval); (void)free_device(didx);
        throw std::runtime_error("fcidump_fill: out of device memory");
    }
    hipError_t err = set_async(dbad, 0, sizeof(bad), st);
    for (int pass = 0; pass < 2 && err == hipSuccess; ++pass)          // fill everything, then verify everything
        for (int64_t b0 = 0; b0 < count && err == hipSuccess; b0 += chunk) {
            const int64_t nb = std::min(chunk, count - b0);
            err = copy_async(dval, val_host + b0, sizeof(double) * nb, hipMemcpyHostToDevice, st);
            if (err == hipSuccess) err = copy_async(didx, pqrs_host + 4 * b0, sizeof(int) * 4 * nb, hipMemcpyHostToDevice, st);
            if (err != hipSuccess) break;
            err = try_launch_kernel(fcidump_fill_kernel, dim3(grid_for(nb)), dim3(256), 0, st, V, dval, didx, (long)nb, (long)n,
                                    is_tc ? 1 : 0, pass, dbad);
            if (err == hipSuccess) err = sync_stream(st);      // the staging buffers are reused
        }
    if (err == hipSuccess) err = copy_sync(&bad, dbad, sizeof(bad), hipMemcpyDeviceToHost);
    (void)free_device(dval); (void)free_device(didx); (void)free_device(dbad);
    HIP_CHECK(err);
    return (int64_t)bad;
}

void tc_single_contraction(const double* L, double* D, int nb, int no, stream_t s) {
    const long total = (long)nb * nb * nb * nb;
    launch_kernel(tc_single_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)s, L, D, nb, no, total);
}
void tc_double_contraction(const double* L, double* S, int nb, int no, stream_t s) {
    launch_kernel(tc_double_kernel, dim3((nb * nb + 255) / 256), dim3(256), 0, (hipStream_t)s, L, S, nb, no);
}
double tc_triple_contraction(const double* L, int nb, int no, stream_t s) {
    double* out = nullptr;
    HIP_CHECK(hipMalloc(&out, sizeof(double)));
    const hipError_t e1 = try_launch_kernel(tc_triple_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, L, out, nb, no);
    double h = 0.0;
    const hipError_t e2 = copy_async(&h, out, sizeof(double), hipMemcpyDeviceToHost, (hipStream_t)s);
    (void)sync_stream((hipStream_t)s);
    (void)free_device(out);
    HIP_CHECK(e1);
    HIP_CHECK(e2);
    return h;
}

// The dense builder and the list builder: ueg_prepare, then `fill(u, umat, uidx, E)` launches the kernel that writes the
// integrals, and everything is released once the stream has drained.
template <typename Fill>
static void ueg_prepare_and_fill(const UegParams& prm, const int* k_int_dev, hipStream_t st, Fill fill) {
    UegPrepared s = ueg_prepare(prm, k_int_dev, st);
    try {
        fill(s.u, s.umat, s.uidx, s.E);
        wait_idle(st);
    } catch (...) {
        ueg_release(s);
        throw;
    }
    ueg_release(s);
}

void ueg_two_body(const UegParams& prm, const int* k_int_dev, const int* index_map_dev, double* V_dev, stream_t s) {
    hipStream_t st = (hipStream_t)s;
    const long n = prm.n_p;
    HIP_CHECK(set_async(V_dev, 0, sizeof(double) * n * n * n * n, st));
    ueg_prepare_and_fill(prm, k_int_dev, st, [&](const UegK& u, const double* umat, const int* uidx, const double* E) {
        const long total = n * n * n;
        launch_kernel(ueg_scatter_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, u, k_int_dev, index_map_dev,
                      umat, uidx, E, V_dev);
    });
}

void ueg_two_body_list(const UegParams& prm, const int* k_int_dev, const int* pqrs_dev, int64_t count, double* out_dev, stream_t s) {
    if (count < 0) throw std::runtime_error("ueg: negative list length");
    if (count == 0) return;
    if (!k_int_dev || !pqrs_dev || !out_dev) throw std::runtime_error("ueg: null argument");
    if ((count + 255) / 256 > 0x7fffffffL) throw std::runtime_error("ueg: list too long for one call");
    hipStream_t st = (hipStream_t)s;
    ueg_prepare_and_fill(prm, k_int_dev, st, [&](const UegK& u, const double* umat, const int* uidx, const double* E) {
        launch_kernel(ueg_list_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, u, k_int_dev, umat, uidx, E,
                      pqrs_dev, (long)count, out_dev);
    });
}

// A ladder term (include/pymes_amd.h, pymes_ueg_ladder_term_create): the prepared state of one Hamiltonian piece, kept until
// ueg_ladder_term_free -- what pymes_sector_ladder_direct evaluates its V_abcd elements from.
struct UegLadderTerm {
    UegPrepared s;
};
UegLadderTerm* ueg_ladder_term_create(const UegParams& prm, const int* k_int_dev, stream_t s) {
    if (!k_int_dev) throw std::runtime_error("ueg: null argument");
    UegLadderTerm* t = new UegLadderTerm;
    try {
        t->s = ueg_prepare(prm, k_int_dev, (hipStream_t)s);
    } catch (...) {
        delete t;
        throw;
    }
    return t;
}
void ueg_ladder_term_free(UegLadderTerm* t) {
    if (!t) return;
    ueg_release(t->s);
    delete t;
}
void ueg_ladder_term_info(const UegLadderTerm* t, int64_t* bytes, int* n_p, double* L) {
    if (!t) throw std::runtime_error("ueg: null ladder term");
    if (bytes) *bytes = t->s.bytes;
    if (n_p) *n_p = t->s.u.n_p;
    if (L) *L = t->s.u.L;
}

}  // namespace dev
